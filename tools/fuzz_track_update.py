#!/usr/bin/env python3
"""Differential fuzz of completing and merging tracks (dsm_update_tracks) against the sequential restatement
(tests/track_update_ref.py): seeded random reconstructions of awkward shapes -- two images, short and long tracks, observations
stripped anywhere, points split in two, wrong matches, unregistered images, a bogus camera, match lists that are not
one-to-one, pairs in any order -- under random step lists (both callers' orders, repeated steps), selections, thresholds and
transitivity caps.  A scene whose smallest margin is >= 1e-9 must agree exactly (ids, track order, modified ids, step counts,
trial counts, xyz bit for bit); any other is counted and not compared.

  python tools/fuzz_track_update.py [--cases 300] [--seed 1] [--host]

--host compares the host build (libdsm_track_update_host.so) instead of the device: no GPU needed.
Test infrastructure: the restatement is the checker here, as in tests/."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402


def random_case(rng):
    from tests import track_update_scenes as scenes
    n_images = int(rng.choice([2, 3, 4, 6, 9, 14]))
    unreg = tuple(int(x) for x in rng.choice(n_images, int(rng.choice([0, 0, 1, 2])), replace=False)) if n_images > 3 else ()
    s = scenes.random_scene(n_images, int(rng.choice([1, 10, 60, 250])), int(rng.integers(1 << 30)), strip=float(rng.choice([0.0, 0.3, 0.6])),
                            split=float(rng.choice([0.0, 0.3, 0.8])), wrong=float(rng.choice([0.0, 0.1, 0.4])), unregistered=unreg)
    if rng.random() < 0.25:  # a second camera, bogus (focal ratio below 0.1), on some images
        s["cameras"] = list(s["cameras"]) + [capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)]
        s["camera_ids"] = np.append(s["camera_ids"], np.uint32(99))
        cam = np.array(s["image_camera_ids"], np.uint32, copy=True)
        used = {int(i) for i in np.asarray(s["track_obs"]).reshape(-1, 2)[:, 0]}  # a track's image keeps its camera: the scene stays plausible
        for i, iid in enumerate(s["image_ids"]):
            if int(iid) not in used or rng.random() < 0.2:
                cam[i] = 99
        s["image_camera_ids"] = cam
    K = len(s["pairs"])
    off = [int(x) for x in s["match_offsets"]]
    m = [np.asarray(s["matches"])[off[k]:off[k + 1]].copy() for k in range(K)]
    for k in range(K):
        if len(m[k]) > 1 and rng.random() < 0.2:  # repeated features: the duplicate rule
            extra = m[k][rng.integers(len(m[k]), size=2)].copy()
            extra[1, 1] = m[k][int(rng.integers(len(m[k])))][1]
            m[k] = np.concatenate([m[k], extra])[rng.permutation(len(m[k]) + 2)]
    order = rng.permutation(K)
    if K:
        s["pairs"] = np.asarray(s["pairs"])[order].reshape(-1, 2)
        s["matches"] = np.concatenate([m[k] for k in order]).reshape(-1, 2).astype(np.uint32)
        s["match_offsets"] = np.concatenate([[0], np.cumsum([len(m[k]) for k in order])]).astype(np.uint64)
    steps = [[0, 1], [1, 0], [1], [0], [1, 0, 0, 1], [0, 1, 0]][int(rng.integers(6))]
    ids = np.asarray(s["point3D_ids"])
    selected = None if rng.random() < 0.5 or not len(ids) else rng.permutation(ids)[:int(rng.integers(0, len(ids) + 1))]
    opts = dict(complete_max_reproj_error=float(rng.choice([0.5, 4.0, 12.0])), merge_max_reproj_error=float(rng.choice([0.5, 4.0, 12.0])),
                complete_max_transitivity=int(rng.choice([1, 2, 5])))
    return s, steps, selected, opts


def run_fuzz(call, n_cases, seed, log=print):
    from tests import track_update_ref as ref
    from tests import track_update_scenes as scenes
    bad = clear = events = completed = 0
    for c in range(n_cases):
        s, steps, selected, opts = random_case(np.random.default_rng([seed, c]))
        try:
            exp = ref.update_tracks(s, steps, selected, **opts)
            got = call(s, steps, selected, opts)
            if ref.min_margin(exp) >= scenes.MIN_MARGIN:
                scenes.same_result(got, exp)
                clear += 1
                events += int(got["report"].num_merge_events)
                completed += int(got["report"].num_completed)
        except (AssertionError, capi.DsmError) as e:
            bad += 1
            log("case %d (seed %d): %s %r" % (c, seed, type(e).__name__, str(e)[:300]))
    log("track update fuzz: %d cases, %d compared exactly (%d merge events, %d completions), %d mismatches" % (n_cases, clear, events, completed, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=300)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    if a.host:
        call = lambda s, steps, sel, o: capi.update_tracks_host(s, steps, sel, **o)
    else:
        ctx = capi.Context(0)
        call = lambda s, steps, sel, o: ctx.update_tracks(s, steps, sel, **o)
    sys.exit(1 if run_fuzz(call, a.cases, a.seed) else 0)


if __name__ == "__main__":
    main()
