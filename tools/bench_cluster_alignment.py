#!/usr/bin/env python3
"""Cluster alignment (dsm_align_clusters; SfMAligner) on one MI355X over the seeded synthetic scene of
tests/cluster_alignment_ref.py: a 10 000-image sequence split into about 100 clusters (num_images_ub = 100) overlapping by
50 images, as step 5 leaves them, with 5 % wrong associations and 10 % dropped observations.

    python tools/bench_cluster_alignment.py [--images 10000] [--clusters 100] [--cpu-clusters 6] [--out profiles/r09_cluster_alignment.json]

Records the device time per call (HIP events inside the call, median of --reps calls after one warm-up) split into the join,
PROSAC and the refit, PROSAC trials per second (the trials the serial loop counts, over the PROSAC time), and separately the
CPU time of the numpy restatement (tests/cluster_alignment_ref.py, not the reference build) on the first --cpu-clusters
clusters, with the device's result on that subset compared to it."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402
from tests import cluster_alignment_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--clusters", type=int, default=100)
    ap.add_argument("--overlap", type=int, default=50)
    ap.add_argument("--points-per-image", type=int, default=400)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-clusters", type=int, default=6)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    clusters, planted = ref.scene(n_images=a.images, n_clusters=a.clusters, overlap=a.overlap, points_per_image=a.points_per_image,
                                  seed=2026)
    gen_s = time.perf_counter() - t0
    ctx = capi.Context(0)
    ctx.align_clusters(clusters)  # warm-up
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = ctx.align_clusters(clusters)
        runs.append((out["report"].as_dict(), time.perf_counter() - t0))
    reps = sorted(runs, key=lambda r: r[0]["device_ms"])
    rep, wall = reps[len(reps) // 2]
    s, R, t = ref.planted_relative(planted, 0, out["anchor"])
    res = {"metric": "cluster alignment (SfMAligner), device ms per call (measured)", "images": a.images, "clusters": a.clusters,
           "overlap": a.overlap, "observations": int(sum(len(c["obs"]) for c in clusters)),
           "points": int(sum(len(c["point_ids"]) for c in clusters)), "scene_generation_s": gen_s,
           "device_ms": rep["device_ms"], "join_ms": rep["join_ms"], "prosac_ms": rep["prosac_ms"], "refit_ms": rep["refit_ms"],
           "device_ms_all_reps": [r[0]["device_ms"] for r in runs], "call_wall_s": wall,
           "prosac_trials_per_s": rep["prosac_iterations"] / (rep["prosac_ms"] * 1e-3) if rep["prosac_ms"] > 0 else None,
           "report": rep, "in_component": int(out["in_component"].sum()), "anchor": out["anchor"],
           "cluster0_to_anchor_rotation_error": float(np.abs(out["R"][0] - R).max()),
           "byte_identical_repeats": len({json.dumps({k: v for k, v in r[0].items() if not k.endswith("_ms")}) for r in runs}) == 1}
    if a.cpu_clusters > 1:
        sub = clusters[:a.cpu_clusters]
        t0 = time.perf_counter()
        exp = ref.align(sub)
        cdt = time.perf_counter() - t0
        dev = ctx.align_clusters(sub)
        res["cpu_restatement"] = {"method": "tests/cluster_alignment_ref.py: numpy, batched LAPACK SVD, Python mt19937", "clusters": len(sub),
                                  "pairs": len(exp["pairs"]), "seconds": cdt, "device_ms_same_subset": dev["report"].device_ms,
                                  "prosac_iterations": int(sum(sum(p["iterations"]) for p in exp["pairs"])),
                                  "same_anchor": dev["anchor"] == exp["anchor"],
                                  "same_inliers_iterations": all(list(dp["num_inliers"]) == ep["inliers"] and list(dp["iterations"]) == ep["iterations"]
                                                                 for dp, ep in zip(dev["pairs"], exp["pairs"])),
                                  "min_margin": min([p["margin"] for p in exp["pairs"]] + [float("inf")])}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
