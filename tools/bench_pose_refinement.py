#!/usr/bin/env python3
"""Measures dsm_refine_absolute_poses (**Measured**) on one device and prints / writes one JSON record.

  python tools/bench_pose_refinement.py [--problems 64] [--repeats 5] [--ref-subset 8] [--out profiles/NAME.json]

Two shapes: the batch of tools/bench_absolute_pose.py (--problems registrations, N from 30 to 3 000, 30 % outliers, 0.5 px noise;
the mask and the start a registration hands over, focal length and extra parameters free) and one problem of N = 800.  Per shape:
one warm-up, then the median of --repeats calls with min / max (host wall clock around the call and the call's own HIP events),
the iterations, and whether the repeats returned the same bytes.  Beside it the time of the sequential numpy restatement
(tests/pose_refinement_ref.py) on the first --ref-subset problems: numpy on the host, NOT the reference's C++ with Ceres."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dagsfm_amd import capi  # noqa: E402
from tests import pose_refinement_ref as ref  # noqa: E402
from tests import pose_refinement_scenes as sc  # noqa: E402

SIZES = (30, 60, 120, 200, 400, 800, 1500, 3000)  # tools/bench_absolute_pose.py's


def make(n_problems):
    return [sc.problem(9000 + i, SIZES[i % len(SIZES)], 0.3, 0.5, 0, 3, focal_error=0.02) for i in range(n_problems)]


def measure(ctx, problems, repeats):
    kw = sc.batch(problems)
    ctx.refine_absolute_poses(**kw)  # warm-up
    walls, reps, blobs = [], [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = ctx.refine_absolute_poses(**kw)
        walls.append((time.perf_counter() - t0) * 1e3)
        reps.append(out["report"])
        blobs.append(b"".join(bytes(r) for r in out["results"]))
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    return dict(problems=len(problems), points=int(reps[0].num_points), iterations=int(reps[0].num_iterations),
                wall_ms=stat(walls), device_ms=stat([q.device_ms for q in reps]), upload_ms=stat([q.upload_ms for q in reps]),
                solve_ms=stat([q.solve_ms for q in reps]), download_ms=stat([q.download_ms for q in reps]),
                setup_ms=stat([q.setup_ms for q in reps]), successes=int(sum(r.success for r in out["results"])),
                identical_bytes=len(set(blobs)) == 1, min_margin=[float(m) for m in reps[0].min_margin])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-subset", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    info = ctx.device_info()
    batch = make(a.problems)
    rec = dict(tool="bench_pose_refinement", device=dict(name=info.name.decode(), arch=info.arch.decode(), compute_units=int(info.compute_units), clock_mhz=info.clock_khz / 1e3),
               batch=measure(ctx, batch, a.repeats), single_n800=measure(ctx, [sc.problem(9100, 800, 0.3, 0.5, 0, 3, focal_error=0.02)], a.repeats))
    est = os.path.join(ROOT, "profiles", "r12_absolute_pose.json")
    if os.path.exists(est):  # context: the estimator on the batch of the same shape
        e = json.load(open(est))
        w = e.get("batch_sweep", {}).get("wall_ms", {}).get("median")
        if w:
            rec["estimator_batch_wall_ms"] = w
            rec["ratio_to_estimator"] = rec["batch"]["wall_ms"]["median"] / w
    t0 = time.perf_counter()
    for p in batch[:a.ref_subset]:
        ref.refine(*sc.args(p))
    rec["numpy_restatement"] = dict(problems=min(a.ref_subset, len(batch)), seconds=time.perf_counter() - t0,
                                    note="numpy on the host, not the reference's C++ with Ceres")
    rec["not_measured"] = ["per-kernel hardware counters", "the reference's C++ time (Ceres is not available)",
                           "the split between evaluation, J'J sums and the serial solve inside k_pr_refine"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
