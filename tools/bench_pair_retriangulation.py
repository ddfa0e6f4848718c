#!/usr/bin/env python3
"""Re-triangulation of the under-reconstructed pairs (dsm_retriangulate_pairs; Retriangulate) on one MI355X:
the 10 000-image sequence of tools/bench_retriangulation.py with --remove of its existing points taken out, so that most
pairs fall below re_min_ratio.

    python tools/bench_pair_retriangulation.py [--images 10000] [--remove 0.67] [--reps 5] [--out FILE]

Records the device time per call (median of --reps calls after one warm-up; HIP events inside the call) split by stage, the
round count (the longest dependency chain of pairs is num_rounds, or num_rounds - 1 when only a gated pair sits in the last
round), the pairs per status and the correspondences per case, and whether the repeats returned the same bytes."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402
from tests import retriangulation_ref as ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--points-per-image", type=int, default=120)
    ap.add_argument("--remove", type=float, default=0.67)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    scene, _ = ref.make_scene(n_images=a.images, n_points=a.images * a.points_per_image // 4, track=(2, 6), noise=0.3, wrong=0.1,
                              existing=0.3, sequence=True, seed=2026)
    rng = np.random.default_rng(2027)
    gone = rng.random(len(scene["point3D_ids"])) < a.remove  # the points stay in the arrays; no point2D refers to them
    p3 = scene["points2D_point3D"]
    scene["points2D_point3D"] = np.where((p3 >= 0) & gone[np.maximum(p3, 0)], -1, p3).astype(np.int32)
    gen_s = time.perf_counter() - t0
    ctx = capi.Context(0)
    ctx.retriangulate_pairs(scene)  # warm-up
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = ctx.retriangulate_pairs(scene)
        runs.append((out["report"].as_dict(), time.perf_counter() - t0, out))
    order = sorted(range(len(runs)), key=lambda k: runs[k][0]["device_ms"])
    rep, wall, _ = runs[order[len(order) // 2]]
    keys = ("new_point_ids", "new_xyz", "new_track_obs", "continued_obs", "continued_point_ids", "touched_point_ids", "pair_status")
    res = {"metric": "pair re-triangulation, device ms per call (measured)", "images": a.images, "removed_share": a.remove,
           "points2D": int(scene["points2D_offsets"][-1]), "pairs": int(len(scene["pairs"])), "matches": int(len(scene["matches"])),
           "points3D_referenced": int(len(np.unique(scene["points2D_point3D"][scene["points2D_point3D"] >= 0]))),
           "scene_generation_s": gen_s, "device_ms_median": rep["device_ms"], "device_ms_all": [r[0]["device_ms"] for r in runs],
           "wall_ms_of_median": 1e3 * wall, "report_of_median": rep,
           "byte_identical_repeats": all(all(r[2][k].tobytes() == runs[0][2][k].tobytes() for k in keys) for r in runs)}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
