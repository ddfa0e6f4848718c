#!/usr/bin/env python3
"""Differential fuzz of the vocabulary training (dsm_retrieval_quantize, dsm_retrieval_train_embedding) against
tests/vocabulary_build_ref.py on ONE context: many small seeded descriptor sets with awkward shapes -- 2 .. 40 modes, runs of
identical rows (zero potentials, emptied clusters), sizes around the 256-point chunk, branching 2 .. 64, 0 .. 11 iterations and
"until convergence", word counts at and off (branching - 1) * K + 1 -- each clustered by the whole chip, by workgroups and at the
default switch.  Words, centres, every node of the tree (float bits), the permutation and the number of draws must be
identical; the thresholds of the embedding trained on the result must be the restatement's bits.

  python tools/fuzz_vocabulary.py [--cases 40] [--seed 1]

Test infrastructure: the restatement is the checker here, as in tests/."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402
from tests import vocabulary_build_ref as ref  # noqa: E402
from tests import vocabulary_build_scenes as scenes  # noqa: E402

SCHEDULES = (1, 2 ** 31 - 1, 0)


def run_fuzz(ctx, n_cases, seed, log=lambda *a: print(*a, flush=True)):
    bad = 0
    for c in range(n_cases):
        rng = np.random.default_rng([seed, c])
        b = int(rng.choice([2, 3, 4, 8, 16, 64]))
        n = int(rng.choice([b, b + 1, 2 * b - 2, 2 * b - 1, 2 * b, 100, 255, 256, 257, 700, 1500]))
        n = max(n, b)
        nw = int(rng.integers(b, n + 1))
        it = int(rng.choice([0, 1, 2, 11, -1]))
        spread = float(rng.choice([0.0, 3.0, 12.0]))
        d = scenes.modes(n, int(rng.integers(2, 41)), int(rng.integers(0, 2 ** 31)), spread=spread)
        if spread == 0.0 and it < 0:
            it = 11
        if rng.random() < 0.4:
            k = int(rng.integers(2, n + 1))
            d[rng.permutation(n)[:k]] = d[0]
            it = 11 if it < 0 else it  # the repair of an emptied cluster never lets such a set converge, in the reference either
        draws = [int(v) for v in rng.integers(0, ref.RAND_MAX + 1, 4)]  # a few edge draws in front of a random stream
        stream = [0, ref.RAND_MAX] + draws
        rec = ref.Recorder(lambda: stream.pop(0) if stream else int(rng.integers(0, ref.RAND_MAX + 1)))
        o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it)
        try:
            words, centres, nodes, indices = ref.quantize(d, nw, b, it, rand=rec)
        except ValueError:
            # identical points without an iteration: the reference never ends, the device must refuse
            try:
                ctx.retrieval_quantize(d, o, rand=ref.Replay(rec.draws + [0] * (4 * b)))
                bad += 1
                log("case %d: a clustering without end was not refused" % c)
            except capi.DsmError:
                pass
            continue
        tree = ref.tree_arrays(nodes)
        ok = True
        for wg in SCHEDULES:
            replay = ref.Replay(rec.draws)
            o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it, workgroup_node_max=wg)
            got_words, got_centres = ctx.retrieval_quantize(d, o, rand=replay, with_centers=True)
            got = ctx.vocabulary_tree()
            same = (replay.pos == len(rec.draws) and got_words.shape == words.shape and (got_words == words).all()
                    and ref.same_floats(got_centres.view(np.uint32), centres.view(np.uint32)) and len(got[0]) == len(tree[0])
                    and all((g == r).all() for g, r in zip(got[:3], tree[:3]))
                    and all(ref.same_floats(g, r) for g, r in zip(got[3:6], tree[3:])) and (got[6] == indices).all())
            ok = ok and same
        projection = np.linalg.qr(rng.normal(size=(128, 128)))[0][:64].astype(np.float32)
        thr, has = ctx.retrieval_train_embedding(d, words, projection)
        ref_thr, ref_has = ref.train_embedding(d, words, projection)
        ok = ok and (thr.view(np.uint32) == ref_thr.view(np.uint32)).all() and (has == ref_has).all()
        if not ok:
            bad += 1
            log("MISMATCH case %d: n %d words %d branching %d iterations %d" % (c, n, nw, b, it))
    log("fuzz_vocabulary: %d cases, %d mismatches" % (n_cases, bad))
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=40)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    sys.exit(1 if run_fuzz(capi.Context(0), args.cases, args.seed) else 0)


if __name__ == "__main__":
    main()
