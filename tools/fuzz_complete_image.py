#!/usr/bin/env python3
"""Differential fuzz of completing images (dsm_complete_images) against the sequential restatement
(tests/complete_image_ref.py): tools/fuzz_track_update.py's seeded reconstructions of awkward shapes (two images, short and long
tracks, observations stripped, points split, wrong matches, unregistered images, a bogus camera, match lists that are not
one-to-one, pairs in any order) with a random share of their points taken out whole, under random image lists (any order,
unregistered and bogus images included), step lists (none, both callers' orders), selections, thresholds, transitivity caps,
min_angle and ignore_two_view_tracks.  A case whose smallest margin is >= 1e-9 must agree (ids, track order, modified ids,
counts, both trial counts exactly; xyz within 1e-9 relative); any other is counted and not compared.

  python tools/fuzz_complete_image.py [--cases 300] [--seed 1] [--check]
  python tools/fuzz_complete_image.py --record-digests FILE

--check runs the check build.  --record-digests writes the digests tests/test_complete_image_gpu.py holds the entries that
existed before to (tests/golden/complete_image_parent_digests.json were recorded with the package of the commit before on the
import path).
Test infrastructure: the restatement is the checker here, as in tests/."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dagsfm_amd import capi  # noqa: E402
import fuzz_track_update  # noqa: E402


def random_case(rng):
    from tests import complete_image_scenes as scenes
    s, steps, selected, opts = fuzz_track_update.random_case(rng)
    s = scenes.without_points(s, float(rng.choice([0.0, 0.2, 0.5, 1.0])), int(rng.integers(1 << 30)))
    ids = np.asarray(s["point3D_ids"])
    if selected is not None:
        selected = np.array([i for i in selected if i in set(ids.tolist())], np.uint64)
    steps = [steps, [], [0, 1]][int(rng.integers(3))]
    images = np.asarray(s["image_ids"])
    listed = rng.permutation(images)[:int(rng.integers(0, len(images) + 1))]
    opts = dict(opts, ignore_two_view_tracks=int(rng.integers(2)), min_angle=float(rng.choice([0.0, 1.5, 4.0])))
    return s, listed, steps, selected, opts


def run_fuzz(ctx, n_cases, seed, log=print):
    from tests import complete_image_ref as ref
    from tests import complete_image_scenes as scenes
    bad = clear = points = completed = long_lists = 0
    for c in range(n_cases):
        s, listed, steps, selected, opts = random_case(np.random.default_rng([seed, c]))
        try:
            exp = ref.complete_images(s, listed, steps, selected, **opts)
            got = ctx.complete_images(s, listed, steps, selected, **opts)
            if ref.min_margin(exp) >= scenes.MIN_MARGIN:
                scenes.same_result(got, exp)
                clear += 1
                points += int(got["report"].num_new_points)
                completed += int(got["report"].num_completed_observations)
                long_lists += sum(1 for it in exp["items"] if it[2] > ref.EXHAUSTIVE)
        except (AssertionError, capi.DsmError) as e:
            bad += 1
            log("case %d (seed %d): %s %r" % (c, seed, type(e).__name__, str(e)[:300]))
    log("complete image fuzz: %d cases, %d compared (%d new points, %d completions, %d lists above 15), %d mismatches"
        % (n_cases, clear, points, completed, long_lists, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--record-digests")
    a = ap.parse_args()
    ctx = capi.Context(0, check=a.check)
    if a.record_digests:
        from tests import complete_image_scenes as scenes
        d = scenes.existing_entry_digests(ctx)
        d["_recorded_from"] = "the product library built from the commit before dsm_complete_images"
        with open(a.record_digests, "w") as f:
            json.dump(d, f, indent=1, sort_keys=True)
        print(json.dumps(d))
        return
    sys.exit(1 if run_fuzz(ctx, a.cases, a.seed) else 0)


if __name__ == "__main__":
    main()
