#!/usr/bin/env python3
"""First measurements of dsm_find_next_images and dsm_find_local_bundles.

The scene of tools/bench_initial_pair.py: `--clusters` clusters of `--images` images each (by default 32 x 60), every cluster a
ring of cameras around its own cloud, every image matched with its next `--neighbours` images; one problem per cluster.  Every
second image of a cluster is registered at its true pose, and a point of the cloud that two registered images see is a point of
the reconstruction, referenced by the observations of the registered images that see it.  dsm_find_next_images ranks the other
half; dsm_find_local_bundles is asked for the bundle of every registered image.  One warm-up, then the median of `--repeats`
calls, with the reports' stage times, against the host build (libdsm_next_images_host.so) on one CPU thread of the same box.
The device's results must be the host build's bytes; exit status 3 otherwise."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagsfm_amd import capi  # noqa: E402
from tests import initial_pair_scenes as scenes  # noqa: E402


def quat_of(R):
    """RotationMatrixToQuaternion for a proper rotation with a positive trace or not (Shepperd's method)."""
    t = np.trace(R)
    if t > 0:
        s = math.sqrt(t + 1.0) * 2
        return np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.zeros(4)
    q[0], q[1 + i], q[1 + j], q[1 + k] = (R[k, j] - R[j, k]) / s, 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
    return q


def build(clusters, images, points, neighbours, seed):
    b = scenes.Builder(seed)
    b.camera(scenes.pinhole())
    problems = []
    for c in range(clusters):
        X = scenes.cloud(b.rng, points) + np.array([20.0 * c, 0.0, 0.0])
        first = len(b.obs)
        for k in range(images):
            a = math.pi * (k + 1) / images
            center = np.array([20.0 * c + 6.0 * math.sin(a), 0.2 * math.cos(5 * a), -6.0 * math.cos(a)])
            R, t = scenes.look_at(center, target=(20.0 * c, 0.0, 0.0), roll=0.01 * k)
            lo = int(0.3 * points * k / max(images - 1, 1))
            b.image(R, t, X, range(lo, min(points, lo + int(0.7 * points))))
        for i in range(images):
            for j in range(i + 1, min(images, i + 1 + neighbours)):
                b.pair(first + i, first + j, wrong=0.1)
        idx = list(range(first, first + images))
        reg = [int((i - first) % 2 == 0) for i in idx]
        seen = {}
        for i, r in zip(idx, reg):
            if r:
                for p in b.obs[i][0]:
                    seen[p] = seen.get(p, 0) + 1
        obs = [np.array([p if r and seen.get(p, 0) >= 2 else -1 for p in b.obs[i][0]], np.int32) for i, r in zip(idx, reg)]
        problems.append(dict(image_ids=[i + 1 for i in idx], registered=reg, obs_point3D=obs, qvec=np.array([quat_of(b.poses[i][0]) for i in idx]),
                             tvec=np.array([b.poses[i][1] for i in idx]), point_xyz=X))
    s = b.scene(id_of=lambda i: i + 1)
    s["points2D_xy"] = np.maximum(s["points2D_xy"], 0.0)  # a candidate's coordinates must not be negative
    queries = [(c, i) for c, pr in enumerate(problems) for i, r in zip(pr["image_ids"], pr["registered"]) if r]
    return s, problems, queries


def timed(fn, repeats):
    fn()
    times, out = [], None
    for _ in range(repeats):
        t = time.perf_counter()
        out = fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), out


def next_bytes(results):
    return [(r["next_image_ids"], r["num_visible"].tobytes(), r["num_observations"].tobytes(), r["score"].tobytes()) for r in results]


def bundle_bytes(results):
    return [(r["bundle_image_ids"], r["overlap_image_ids"], r["overlap_shared"], np.asarray(r["overlap_tri_angle"]).tobytes()) for r in results]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--images", type=int, default=60)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--neighbours", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread baseline (and the comparison with it)")
    ap.add_argument("--out", default="", help="also write the JSON record to this file")
    a = ap.parse_args()
    t0 = time.perf_counter()
    s, problems, queries = build(a.clusters, a.images, a.points, a.neighbours, seed=30)
    rec = dict(clusters=a.clusters, images=a.images, pairs=int(len(s["pairs"])), matches=int(len(s["matches"])), queries=len(queries),
               observations=int(s["points2D_offsets"][-1]), build_s=round(time.perf_counter() - t0, 2))
    ctx = capi.Context(0)
    # (the call times include the binding's marshalling of the Python lists, the same on both sides)
    ms, out = timed(lambda: ctx.find_next_images(s, problems), a.repeats)
    rep = out["report"]
    rec["find_next_images"] = dict(call_ms=round(ms, 3), setup_ms=round(rep.setup_ms, 3), graph_ms=round(rep.graph_ms, 3),
                                   visibility_ms=round(rep.visibility_ms, 3), score_ms=round(rep.score_ms, 3), rank_ms=round(rep.rank_ms, 3),
                                   device_ms=round(rep.device_ms, 3), eligible=rep.num_eligible, batches=rep.num_batches)
    ms2, out2 = timed(lambda: ctx.find_local_bundles(s, problems, queries), a.repeats)
    rep2 = out2["report"]
    rec["find_local_bundles"] = dict(call_ms=round(ms2, 3), setup_ms=round(rep2.setup_ms, 3), tracks_ms=round(rep2.tracks_ms, 3),
                                     overlap_ms=round(rep2.overlap_ms, 3), angles_ms=round(rep2.angles_ms, 3), device_ms=round(rep2.device_ms, 3),
                                     copied=rep2.num_copied, chained=rep2.num_chained, angles=rep2.num_angles, filled=rep2.num_filled,
                                     min_tri_angle_margin=rep2.min_tri_angle_margin, batches=rep2.num_batches)
    if not a.no_host:
        hms, hout = timed(lambda: capi.next_images_host(s, problems), a.repeats)
        hms2, hout2 = timed(lambda: capi.local_bundles_host(s, problems, queries), a.repeats)
        rec["host"] = dict(find_next_images_ms=round(hms, 3), find_local_bundles_ms=round(hms2, 3))
        if next_bytes(out["results"]) != next_bytes(hout) or bundle_bytes(out2["results"]) != bundle_bytes(hout2[0]):
            print(json.dumps(dict(error="the device and the host build differ")))
            sys.exit(3)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
