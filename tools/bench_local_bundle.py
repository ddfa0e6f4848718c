"""Times dsm_adjust_local_bundles on 64 problems shaped like the mapper's local bundle adjustment (6 config images, a few
thousand points, outside observations on the short tracks): median of 5 after a warm-up, HIP-event split.  Beside it the only
route the parent commit offers: the same 64 problems one by one through dsm_bundle_adjust.  Both sides use the trivial loss for
that comparison (dsm_bundle_adjust has no other); the batch is also timed with the default SOFT_L1.
Writes profiles/r15_local_bundle.json.  Usage: python tools/bench_local_bundle.py [--problems 64] [--points 3000]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dagsfm_amd import capi  # noqa: E402
from tests.local_bundle_scenes import local_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_local_bundle.json"))
    a = ap.parse_args()
    problems = [local_scene(1000 + b, 6, 6, n_points=a.points, min_track=2, max_track=6, noise=0.7) for b in range(a.problems)]
    n_obs = int(sum(len(p["obs_image"]) for p in problems))
    ctx = capi.Context(0)
    rec = {"problems": a.problems, "points_per_problem": a.points, "observations": n_obs, "repeats": a.repeats}
    for label, kind in (("trivial", capi.LOSS_TRIVIAL), ("soft_l1", capi.LOSS_SOFT_L1)):
        opt = capi.default_local_bundle_options(loss_function_type=kind)
        ctx.adjust_local_bundles(problems, opt, trace=False)  # warm-up
        walls, reps, outs = [], [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out = ctx.adjust_local_bundles(problems, opt, trace=False)
            walls.append((time.perf_counter() - t0) * 1e3)
            reps.append(out["report"].as_dict())
            outs.append(b"".join(p["xyz"].tobytes() for p in out["problems"]))
        k = int(np.argsort(walls)[len(walls) // 2])
        rec["batch_" + label] = {"wall_ms_median": walls[k], "wall_ms_all": walls, "report_of_median": reps[k],
                                 "identical_repeats": all(o == outs[0] for o in outs),
                                 "iterations": int(sum(p["result"].num_iterations for p in out["problems"])),
                                 "reduced_dim": int(out["problems"][0]["result"].reduced_dim)}
    # the parent's route: one dsm_bundle_adjust call per problem (camera_constant does not exist there; the scenes have none set
    # on a shared camera, so the two sides solve the same problems; a track of length 1 would be refused there: min_track is 2)
    bopt = capi.default_bundle_adjustment_options(max_num_iterations=25, gradient_tolerance=10.0)
    single = lambda p: {k: v for k, v in p.items() if k != "camera_constant"}
    ctx.bundle_adjust(single(problems[0]), bopt, trace=False)
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        its = 0
        for p in problems:
            its += ctx.bundle_adjust(single(p), bopt, trace=False)["report"].num_iterations
        walls.append((time.perf_counter() - t0) * 1e3)
    rec["one_by_one_dsm_bundle_adjust_trivial"] = {"wall_ms_median": float(np.median(walls)), "wall_ms_all": walls, "iterations": int(its)}
    rec["ratio_one_by_one_over_batch_trivial"] = rec["one_by_one_dsm_bundle_adjust_trivial"]["wall_ms_median"] / rec["batch_trivial"]["wall_ms_median"]
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
