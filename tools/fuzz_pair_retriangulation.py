#!/usr/bin/env python3
"""Differential fuzz of the pair re-triangulation (dsm_retriangulate_pairs) against the sequential numpy
restatement (tests/pair_retriangulation_ref.py): seeded random scenes of awkward shapes -- two images, two-view tracks, no
existing point, everything existing, links dropped anywhere in a track, unregistered images, a bogus camera, pairs written as (image2, image1), match lists
that are not one-to-one, trial counters from an earlier call -- under random re_min_ratio / re_max_trials /
ignore_two_view_tracks.  A scene whose smallest margin is >= 1e-9 must agree decision for decision, any other in num_tris
within 2 % (the comparison of tests/test_pair_retriangulation_gpu.py).

  python tools/fuzz_pair_retriangulation.py [--cases 200] [--seed 1]

Test infrastructure: the restatement is the checker here, as in tests/."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402


def random_case(rng):
    from tests import pair_retriangulation_ref as ref
    n_images = int(rng.choice([2, 3, 4, 6, 9, 12]))
    lo = int(rng.integers(2, min(n_images, 5) + 1))
    hi = int(rng.integers(lo, min(n_images, 8) + 1))
    unreg = tuple(int(x) for x in rng.choice(n_images, int(rng.choice([0, 0, 1, 2])), replace=False)) if n_images > 2 else ()
    cams = [capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480)]
    if rng.random() < 0.3:
        cams.append(capi.camera(1, [480.0, 510.0, 320.0, 240.0], 640, 480))
    if rng.random() < 0.2:
        cams.append(capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480))  # bogus: focal ratio below 0.1
    s, _ = ref.make_scene(n_images=n_images, n_points=int(rng.choice([1, 10, 60, 300])), track=(lo, hi),
                          noise=float(rng.choice([0.0, 0.3, 2.0])), wrong=float(rng.choice([0.0, 0.1, 0.4])),
                          existing=float(rng.choice([0.0, 0.15, 0.5, 1.0])), cameras=cams, unregistered=unreg,
                          seed=int(rng.integers(1 << 30)))
    if rng.random() < 0.4:  # features without their point anywhere in a track: gate-only pairs share features with candidates
        p3 = s["points2D_point3D"]
        s["points2D_point3D"] = np.where(rng.random(len(p3)) < 0.35, -1, p3).astype(np.int32)
    K = len(s["pairs"])
    off = [int(x) for x in s["match_offsets"]]
    m = [s["matches"][off[k]:off[k + 1]].copy() for k in range(K)]
    pairs = s["pairs"].copy()
    for k in range(K):
        if len(m[k]) > 1 and rng.random() < 0.2:  # repeated features: the duplicate rule
            extra = m[k][rng.integers(len(m[k]), size=2)].copy()
            extra[1, 1] = m[k][int(rng.integers(len(m[k])))][1]
            m[k] = np.concatenate([m[k], extra])[rng.permutation(len(m[k]) + 2)]
        if rng.random() < 0.3:
            pairs[k] = pairs[k][::-1]
            m[k] = m[k][:, ::-1]
    order = rng.permutation(K)
    s["pairs"] = pairs[order].reshape(-1, 2)
    s["matches"] = np.concatenate([m[k] for k in order]).reshape(-1, 2).astype(np.uint32) if K else s["matches"]
    s["match_offsets"] = np.concatenate([[0], np.cumsum([len(m[k]) for k in order])]).astype(np.uint64)
    opts = dict(re_min_ratio=float(rng.choice([0.0, 0.2, 0.5, 0.95, 2.0])), re_max_trials=int(rng.choice([0, 1, 1, 2])),
                ignore_two_view_tracks=int(rng.integers(2)), re_max_angle_error=float(rng.choice([0.5, 5.0])))
    trials = rng.integers(0, 3, K).astype(np.uint32) if rng.random() < 0.4 else None
    return s, opts, trials


def run_fuzz(ctx, n_cases, seed, log=print):
    from tests import pair_retriangulation_ref as ref
    from tests.test_pair_retriangulation_gpu import compare
    bad = clear = 0
    for c in range(n_cases):
        s, opts, trials = random_case(np.random.default_rng([seed, c]))
        try:
            dev = ctx.retriangulate_pairs(s, capi.default_pair_retriangulation_options(**opts), re_num_trials=trials)
            clear += compare(dev, ref.retriangulate_pairs(s, options=opts, re_num_trials=trials))
        except (AssertionError, capi.DsmError) as e:
            bad += 1
            log("case %d (seed %d): %s %r" % (c, seed, type(e).__name__, str(e)[:300]))
    log("pair re-triangulation fuzz: %d cases, %d compared decision for decision, %d mismatches" % (n_cases, clear, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    sys.exit(1 if run_fuzz(capi.Context(0), a.cases, a.seed) else 0)


if __name__ == "__main__":
    main()
