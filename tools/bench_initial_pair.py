#!/usr/bin/env python3
"""First measurements of dsm_find_initial_pairs.

A synthetic scene of `--clusters` clusters of `--images` images each (by default 32 x 60): every cluster is a ring of cameras
around its own cloud, the first third of the ring a hair's breadth apart (so the best-ranked candidates of a cluster fail the
angle test and the search has to go on), every image matched with its next `--neighbours` images.  One problem per cluster.
For every speculation_window of `--windows`: one warm-up, then the median of `--repeats` calls, with the report's stage times
and counts.  The baseline is the same search on one CPU thread of the same box: the host build's candidate order
(libdsm_initial_pair_host.so) and the oracle's EstimateCalibrated for every pair the device tried, in trial order -- the pairs
the sequential search would have run.  The pairs found by the windows must be the same bytes; exit status 3 otherwise."""
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
from tests import initial_pair_ref as ref  # noqa: E402
from tests import initial_pair_scenes as scenes  # noqa: E402
from tests import oracle_lib  # noqa: E402


def build(clusters, images, points, neighbours, seed):
    b = scenes.Builder(seed)
    b.camera(scenes.pinhole())
    problems = []
    for c in range(clusters):
        X = scenes.cloud(b.rng, points) + np.array([20.0 * c, 0.0, 0.0])
        first = len(b.obs)
        for k in range(images):
            close = k < images // 3  # a bundle of near-coincident views: many matches, no baseline
            a = 0.002 * k if close else math.pi * (k - images // 3 + 1) / images
            center = np.array([20.0 * c + 6.0 * math.sin(a), 0.2 * math.cos(5 * a), -6.0 * math.cos(a)])
            R, t = scenes.look_at(center, target=(20.0 * c, 0.0, 0.0), roll=0.01 * k)
            lo = int(0.3 * points * k / max(images - 1, 1))
            b.image(R, t, X, range(lo, min(points, lo + int(0.7 * points))))
        for i in range(images):
            for j in range(i + 1, min(images, i + 1 + neighbours)):
                b.pair(first + i, first + j, wrong=0.1)
        problems.append(list(range(first, first + images)))
    s = b.scene(id_of=lambda i: i + 1)
    return s, [dict(image_ids=[i + 1 for i in p]) for p in problems]


def result_bytes(out):
    return [(r["image_id1"], r["image_id2"], bytes(r["two_view_geometry"]), r["tried_pairs"].tobytes(), r["new_xyz"].tobytes()) for r in out["results"]]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--images", type=int, default=60)
    ap.add_argument("--points", type=int, default=300)
    ap.add_argument("--neighbours", type=int, default=8)
    ap.add_argument("--windows", default="1,4,16,64")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--min-inliers", type=int, default=100)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread baseline")
    ap.add_argument("--out", default="", help="also write the JSON record to this file")
    a = ap.parse_args()
    t0 = time.perf_counter()
    s, problems = build(a.clusters, a.images, a.points, a.neighbours, seed=29)
    rec = dict(clusters=a.clusters, images=a.images, pairs=int(len(s["pairs"])), matches=int(len(s["matches"])),
               build_s=round(time.perf_counter() - t0, 2), windows={})
    ctx = capi.Context(0)
    first = None
    for w in [int(x) for x in a.windows.split(",")]:
        o = capi.default_initial_pair_options(init_min_num_inliers=a.min_inliers, speculation_window=w)
        ctx.find_initial_pairs(s, problems, o)
        times, out = [], None
        for _ in range(a.repeats):
            t = time.perf_counter()
            out = ctx.find_initial_pairs(s, problems, o)
            times.append((time.perf_counter() - t) * 1e3)
        rep = out["report"]
        rec["windows"][w] = dict(call_ms=round(statistics.median(times), 3), device_ms=round(rep.device_ms, 3), setup_ms=round(rep.setup_ms, 3),
                                 graph_ms=round(rep.graph_ms, 3), gather_ms=round(rep.gather_ms, 3), verify_ms=round(rep.verify_ms, 3),
                                 pose_ms=round(rep.pose_ms, 3), triangulate_ms=round(rep.triangulate_ms, 3), rounds=rep.num_rounds,
                                 batches=rep.num_batches, candidates=rep.num_candidates, verified=rep.num_verified,
                                 speculated=rep.num_speculated, found=sum(r["found"] for r in out["results"]),
                                 tried=sum(r["num_tried"] for r in out["results"]))
        if first is None:
            first = (result_bytes(out), out)
        elif result_bytes(out) != first[0]:
            print(json.dumps(dict(error="window %d changed a byte" % w)))
            sys.exit(3)
    if not a.no_host:
        orc = oracle_lib.load()
        o = capi.default_initial_pair_options(init_min_num_inliers=a.min_inliers)
        t = time.perf_counter()
        lists, _ = capi.initial_pair_host_candidates(s, problems, o)
        order_ms = (time.perf_counter() - t) * 1e3
        kw = dict(init_min_num_inliers=a.min_inliers)
        t = time.perf_counter()
        est_ms = 0.0
        for p, r in zip(problems, first[1]["results"]):
            v = ref.View(s, p)
            assert [tuple(int(x) for x in q) for q in r["tried_pairs"]] == lists[problems.index(p)][:r["num_tried"]]
            for id1, id2 in r["tried_pairs"]:
                m = np.array(v.find_correspondences_between_images(int(id1), int(id2)), np.uint32).reshape(-1, 2)
                cam1, cam2 = ref.forced_prior(v.camera[int(id1)]), ref.forced_prior(v.camera[int(id2)])
                to = capi.default_two_view_options(min_num_trials=30, max_error=o.init_max_error)
                te = time.perf_counter()
                orc.estimate_two_view_geometry(cam1, v.points(int(id1)), cam2, v.points(int(id2)), m, to, capi.pair_seed(int(id1), int(id2), 0))
                est_ms += (time.perf_counter() - te) * 1e3
        rec["host"] = dict(candidate_order_ms=round(order_ms, 3), estimate_ms=round(est_ms, 3), total_ms=round(order_ms + est_ms, 3),
                           python_overhead_s=round(time.perf_counter() - t - est_ms / 1e3, 2), options=kw)
    best = min(rec["windows"], key=lambda w: rec["windows"][w]["call_ms"])
    rec["fastest_window"] = best
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
