#!/usr/bin/env python3
"""First measurements of dsm_patch_match: a synthetic slanted-plane scene, by default 1600 x 1200 with 10
source images at the reference's default options (photometric pass), in batches of 1, 4 and 16 problems.  Per batch: the
HIP-event stage times of dsm_get_patch_match_time and pixels x sweeps per second over the sweep stage and over the whole
call (host clock around the call, which ends in a stream synchronise).  Before timing, a 37 x 23 problem is held to
tests/patch_match_ref.py bit for bit, so that what is timed is what is specified.  One warm-up call per batch size.

    python tools/bench_patch_match.py [--size 1600x1200] [--sources 10] [--batches 1,4,16] [--iterations 5]
                                      [--schedule product|lanes] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagsfm_amd import capi  # noqa: E402
from tests import patch_match_cases as cases  # noqa: E402
from tests import patch_match_scenes as scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--sources", type=int, default=10)
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--schedule", default="product", choices=["product", "lanes"],
                    help="lanes: the check build's lane-per-column sweep (DSM_PATCH_MATCH_LANES), the cross-check schedule")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    if a.schedule == "lanes":
        os.environ["DSM_PATCH_MATCH_LANES"] = "1"
    ctx = capi.Context(0)  # the check build while a check-only switch is set

    small, _ = cases.scene("slanted", ((37, 23), (23, 37), (37, 23)))
    o = cases.options(window_radius=2, num_samples=3, filter=True, filter_min_num_consistent=1)
    cases.assert_same_bits(ctx.patch_match(small, [(0, [1, 2], 2.0, 8.0)], cases.capi_options(o))[0],
                           cases.reference(("bench", 0), small, (0, [1, 2], 2.0, 8.0), o), "bench parity")

    n_views = a.sources + 1
    images, _ = scenes.make_scene("slanted", w, h, n_views, seed=4)
    opts = capi.default_patch_match_options(geom_consistency=0, num_iterations=a.iterations)
    sweeps = 4 * a.iterations
    result = {"size": [w, h], "sources": a.sources, "iterations": a.iterations, "schedule": a.schedule, "batches": []}
    for nb in (int(v) for v in a.batches.split(",")):
        problems = [(k % n_views, [j for j in range(n_views) if j != k % n_views], 2.0, 8.0) for k in range(nb)]
        ctx.patch_match(images, problems[:1], opts, return_sel_prob=False)  # warm-up: code objects, buffers
        t0 = time.perf_counter()
        out = ctx.patch_match(images, problems, opts, return_sel_prob=False)
        wall = time.perf_counter() - t0
        ms = ctx.patch_match_time()
        px_sweeps = float(nb) * w * h * sweeps
        row = {"problems": nb, "stage_ms": ms, "call_s": wall, "pixel_sweeps_per_s_sweep_stage": px_sweeps / (ms["sweeps"] * 1e-3),
               "pixel_sweeps_per_s_call": px_sweeps / wall, "survivors": float(np.mean([(r["depth"] > 0).mean() for r in out]))}
        result["batches"].append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
