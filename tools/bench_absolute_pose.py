#!/usr/bin/env python3
"""Measures dsm_estimate_absolute_poses (DESIGN.md 14 "Measured") on one device and prints / writes one JSON record.

  python tools/bench_absolute_pose.py [--problems 64] [--repeats 5] [--ref-subset 4] [--out profiles/NAME.json]

Three shapes: a batch shaped like a cluster-parallel mapper step (--problems problems x 31 factors, N from the synthetic
generator's grid, 30 % outliers), one problem with the sweep, one without.  Per shape: one warm-up, then the median of --repeats
calls with min / max (host wall clock around the call, and the call's own HIP-event split), the work counters per run, and whether
the repeats returned the same bytes.  Beside it the time of the sequential numpy restatement (tests/absolute_pose_ref.py) on the
first --ref-subset problems of the batch: numpy on the host, NOT the reference's C++."""
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
from tests import absolute_pose_ref as ref  # noqa: E402
from tests import absolute_pose_scenes as scenes  # noqa: E402

SIZES = (30, 60, 120, 200, 400, 800, 1500, 3000)


def make(n_problems, sweep):
    return [dict(zip(("cam", "xy", "X"), scenes.registration(9000 + i, SIZES[i % len(SIZES)], 0.3, 0.5, 0)[:3]), sweep=sweep)
            for i in range(n_problems)]


def call(ctx, problems):
    offs = np.concatenate([[0], np.cumsum([len(p["xy"]) for p in problems])]).astype(np.uint64)
    xy = np.concatenate([p["xy"] for p in problems])
    X = np.concatenate([p["X"] for p in problems])
    t0 = time.perf_counter()
    out = ctx.estimate_absolute_poses([p["cam"] for p in problems], [int(p["sweep"]) for p in problems], offs, xy, X)
    wall = (time.perf_counter() - t0) * 1e3
    return out, wall


def measure(ctx, problems, repeats):
    call(ctx, problems)  # warm-up
    walls, reps, blobs = [], [], []
    for _ in range(repeats):
        out, wall = call(ctx, problems)
        walls.append(wall)
        reps.append(out["report"])
        blobs.append(b"".join(bytes(r) for r in out["results"]) + out["inlier_mask"].tobytes())
    r = reps[0]
    stat = lambda v: dict(median=statistics.median(v), min=min(v), max=max(v))
    return dict(problems=len(problems), points=int(sum(len(p["xy"]) for p in problems)), runs=int(r.num_runs),
                wall_ms=stat(walls), device_ms=stat([q.device_ms for q in reps]), prepare_ms=stat([q.prepare_ms for q in reps]),
                ransac_ms=stat([q.ransac_ms for q in reps]), choice_ms=stat([q.choice_ms for q in reps]),
                setup_ms=stat([q.setup_ms for q in reps]), trials_per_run=r.num_trials / max(r.num_runs, 1),
                models_per_run=r.num_models / max(r.num_runs, 1), local_optimizations_per_run=r.num_local_optimizations / max(r.num_runs, 1),
                successes=int(sum(q.success for q in out["results"])), identical_bytes=len(set(blobs)) == 1,
                min_margin=[float(m) for m in r.min_margin])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ref-subset", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ctx = capi.Context(0)
    batch = make(a.problems, True)
    info = ctx.device_info()
    rec = dict(tool="bench_absolute_pose", device=dict(name=info.name.decode() or "(the runtime reports no marketing name)", arch=info.arch.decode(), compute_units=info.compute_units,
                                                       clock_mhz=info.clock_khz / 1e3, hbm_gb=info.total_memory / 1e9),
               batch_sweep=measure(ctx, batch, a.repeats), single_sweep=measure(ctx, make(6, True)[5:6], a.repeats),
               single_fixed=measure(ctx, make(6, False)[5:6], a.repeats))
    t0 = time.perf_counter()
    for b in range(min(a.ref_subset, len(batch))):
        p = batch[b]
        ref.estimate_absolute_pose(p["cam"], p["xy"], p["X"], True, problem=b)
    rec["numpy_restatement"] = dict(problems=min(a.ref_subset, len(batch)), seconds=time.perf_counter() - t0,
                                    note="sequential numpy on the host, not the reference's C++")
    rec["not_measured"] = ["per-kernel hardware counters", "the reference's C++ time"]
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
