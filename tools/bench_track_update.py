#!/usr/bin/env python3
"""First measurements of dsm_update_tracks (CompleteTracks / MergeTracks on the device).

The scene: `--images` cameras on a line looking along +z at a corridor of `--points` points (by default 2 000 and 10^6); every
point is seen by a run of 3 .. 7 consecutive images, every image is matched with the six that follow it (a fraction `--wrong`
of the matches points at a random feature).  Every ground-truth point is a point3D; then a third of the observations is
stripped from the tracks and a fraction `--split` of the points with four or more observations is split in two, as in
tests/track_update_scenes.py's random scenes.  Both step orders -- COMPLETE, MERGE (CompleteAndMergeTracks) and MERGE, COMPLETE
(AdjustLocalBundle's) -- over all points: one warm-up, then the median of `--repeats` calls with the report's phase times, the
claim rounds and the largest component, against the host build (libdsm_track_update_host.so) on one CPU thread of the same box.
The device's results must be the host build's bytes before any time is reported; exit status 3 otherwise."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagsfm_amd import capi  # noqa: E402

MERGE, COMPLETE = capi.TRACKS_MERGE, capi.TRACKS_COMPLETE
F, CX, CY, DIST, SPACING, REACH = 500.0, 320.0, 240.0, 8.0, 0.5, 7


def make_scene(n_images, n_points, seed, strip=1.0 / 3.0, split=0.3, wrong=0.05, noise=0.4):
    rng = np.random.default_rng(seed)
    L = rng.integers(3, REACH + 1, n_points)
    L = np.minimum(L, n_images)
    first = (rng.random(n_points) * (n_images - L + 1)).astype(np.int64)
    X = np.stack([(first + 0.5 * (L - 1)) * SPACING + rng.uniform(-0.5, 0.5, n_points), rng.uniform(-1.5, 1.5, n_points),
                  rng.uniform(-1.0, 1.0, n_points)], 1)
    ooff = np.concatenate([[0], np.cumsum(L)])
    n_obs = int(ooff[-1])
    opoint = np.repeat(np.arange(n_points), L)
    oimg = first[opoint] + (np.arange(n_obs) - ooff[opoint])
    depth = X[opoint, 2] + DIST
    xy = np.stack([F * (X[opoint, 0] - oimg * SPACING) / depth + CX, F * X[opoint, 1] / depth + CY], 1) + rng.normal(0, noise, (n_obs, 2))
    order = np.argsort(oimg, kind="stable")  # the features of an image: its observations in point order
    poff = np.concatenate([[0], np.cumsum(np.bincount(oimg, minlength=n_images))])
    feat_of_obs = np.empty(n_obs, np.int64)
    feat_of_obs[order] = np.arange(n_obs)
    idx = feat_of_obs - poff[oimg]
    # matches: every two images of a point's run
    ia, ib, fa, fb = [], [], [], []
    for da in range(REACH):
        for db in range(da + 1, REACH):
            p = np.nonzero(L > db)[0]
            a, b = ooff[p] + da, ooff[p] + db
            ia.append(oimg[a]), ib.append(oimg[b]), fa.append(idx[a]), fb.append(idx[b])
    ia, ib, fa, fb = (np.concatenate(x) for x in (ia, ib, fa, fb))
    bad = rng.random(len(fb)) < wrong
    fb = np.where(bad, (rng.random(len(fb)) * (poff[ib + 1] - poff[ib])).astype(np.int64), fb)
    key = ia * n_images + ib
    morder = np.argsort(key, kind="stable")
    key, ia, ib, fa, fb = key[morder], ia[morder], ib[morder], fa[morder], fb[morder]
    starts = np.nonzero(np.concatenate([[True], key[1:] != key[:-1]]))[0]
    pairs = np.stack([ia[starts], ib[starts]], 1)
    moff = np.concatenate([starts, [len(key)]])
    # the tracks: a third stripped (two stay), some points split in two
    keep = rng.random(n_obs) >= strip
    kept = np.bincount(opoint, keep, n_points)
    few = np.nonzero(kept < 2)[0]
    keep[ooff[few]] = keep[ooff[few] + 1] = True
    kobs = np.nonzero(keep)[0]
    kpoint = opoint[kobs]
    klen = np.bincount(kpoint, minlength=n_points)
    koff = np.concatenate([[0], np.cumsum(klen)])
    do_split = (klen >= 4) & (rng.random(n_points) < split)
    rank = np.arange(len(kobs)) - koff[kpoint]
    second = do_split[kpoint] & (rank >= klen[kpoint] // 2)
    new_index = np.cumsum(do_split) - 1 + n_points  # the second half's point
    tpoint = np.where(second, new_index[kpoint], kpoint)
    torder = np.argsort(tpoint, kind="stable")
    n_total = n_points + int(do_split.sum())
    toff = np.concatenate([[0], np.cumsum(np.bincount(tpoint, minlength=n_total))])
    xyz = np.concatenate([X, X[do_split]]) + np.where(np.concatenate([do_split, np.ones(int(do_split.sum()), bool)])[:, None],
                                                        rng.normal(0, 0.002, (n_total, 3)), 0.0)
    image_ids = np.arange(n_images, dtype=np.uint32) * 3 + 1
    tobs = np.stack([image_ids[oimg[kobs][torder]], idx[kobs][torder]], 1)
    ids = rng.permutation(n_total).astype(np.uint64) * 7 + 11
    return dict(camera_ids=np.array([7], np.uint32), cameras=[capi.simple_pinhole(F, CX, CY, 640, 480)], image_ids=image_ids,
                image_camera_ids=np.full(n_images, 7, np.uint32), registered=np.ones(n_images, np.uint8),
                qvec=np.tile([1.0, 0.0, 0.0, 0.0], (n_images, 1)),
                tvec=np.stack([-np.arange(n_images) * SPACING, np.zeros(n_images), np.full(n_images, DIST)], 1),
                points2D_offsets=poff.astype(np.uint32), points2D_xy=xy[order], pairs=image_ids[pairs].reshape(-1, 2),
                match_offsets=moff.astype(np.uint64), matches=np.stack([fa, fb], 1).astype(np.uint32), point3D_ids=ids, point3D_xyz=xyz,
                track_offsets=toff.astype(np.uint64), track_obs=tobs.astype(np.uint32))


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("point_ids", "xyz", "track_offsets", "track_obs", "modified", "step_counts"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--split", type=float, default=0.3)
    ap.add_argument("--wrong", type=float, default=0.05)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    t0 = time.time()
    s = make_scene(a.images, a.points, a.seed, split=a.split, wrong=a.wrong)
    out = {"images": a.images, "points3D": int(len(s["point3D_ids"])), "points2D": int(s["points2D_offsets"][-1]),
           "track_elements": int(s["track_offsets"][-1]), "pairs": int(len(s["pairs"])), "matches": int(s["match_offsets"][-1]),
           "scene_s": round(time.time() - t0, 2), "orders": {}}
    print(json.dumps({k: v for k, v in out.items() if k != "orders"}), flush=True)
    ctx = capi.Context(0)
    phases = ("setup_ms", "graph_ms", "complete_ms", "components_ms", "schedule_ms", "merge_ms", "download_ms", "device_ms")
    status = 0
    for name, steps in (("complete_merge", [COMPLETE, MERGE]), ("merge_complete", [MERGE, COMPLETE])):
        dev = ctx.update_tracks(s, steps)  # warm-up, and the result that is compared
        row = {}
        if not a.no_host:
            times = []
            for _ in range(a.repeats):
                t = time.perf_counter()
                host = capi.update_tracks_host(s, steps)
                times.append((time.perf_counter() - t) * 1e3)
            if result_bytes(host) != result_bytes(dev):
                print("MISMATCH: the device's result of %s is not the host build's bytes" % name, flush=True)
                status = 3
                continue
            row["host_ms"] = round(statistics.median(times), 2)
        runs, wall = [], []
        for _ in range(a.repeats):
            t = time.perf_counter()
            r = ctx.update_tracks(s, steps)["report"]
            wall.append((time.perf_counter() - t) * 1e3)
            runs.append(r)
        row["device_call_ms"] = round(statistics.median(wall), 2)
        for p in phases:
            row[p] = round(statistics.median(getattr(r, p) for r in runs), 3)
        rep = dev["report"]
        row.update(step_counts=[int(x) for x in dev["step_counts"]], points_out=int(len(dev["point_ids"])), complete_rounds=int(rep.complete_rounds),
                   complete_serial_steps=int(rep.complete_serial_steps), complete_trials=int(rep.complete_trials),
                   merge_trials=int(rep.merge_trials), merge_events=int(rep.num_merge_events), components=int(rep.num_components),
                   largest_component=int(rep.largest_component), correspondences=int(rep.num_correspondences))
        out["orders"][name] = row
        print(json.dumps({name: row}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(status)


if __name__ == "__main__":
    main()
