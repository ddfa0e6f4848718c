#!/usr/bin/env python3
"""Records the reference's own VisualIndex::Quantize answers for the cases of tests/vocabulary_build_scenes.py:
CASES and the large case into tests/golden/vocab_quantize_v1.npz, EDGE_CASES into tests/golden/vocab_quantize_v2.npz.
Needs oracle/_ref/libflann_ref.so (make -C oracle ref, where the reference lies).

  python tools/make_vocabulary_golden.py            writes v2; v1 is recomputed and compared with the file, not rewritten
  python tools/make_vocabulary_golden.py --v1       writes v1 as well

Per case: options = (n, num_visual_words, branching, num_iterations, srand seed), the reference's count and words, the first 8
values of rand() after srand(seed), the SHA-256 of the input bytes, and the input itself for the cases of at most 1000 (v1) or
300 (v2) descriptors (the larger inputs are regenerated from their seed and held to the hash: all of them would pass the size the
golden files keep to).

The words of a cluster the last iteration emptied would be std::round(NaN) cast to uint8_t, which is undefined:
getMinVarianceClusters never picks a node with such children (a NaN variance loses every comparison), so none is recorded; the
tool checks that."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import flann_ref, vocabulary_build_ref as R, vocabulary_build_scenes as S  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def record(lib, cases, max_stored_rows):
    out = {}
    for name, (d, nw, b, it, seed) in cases:
        words = np.zeros((nw, 128), np.uint8)
        lib.flann_ref_seed(seed)
        count = lib.flann_ref_quantize(d.ctypes.data, len(d), nw, b, it, words.ctypes.data)
        R.srand(seed)
        out[name + "/rand8"] = np.array([R.libc_rand() for _ in range(8)], np.int64)
        out[name + "/options"] = np.array([len(d), nw, b, it, seed], np.int64)
        out[name + "/count"] = np.int64(count)
        out[name + "/words"] = words[:count].copy()
        out[name + "/input_sha256"] = np.frombuffer(hashlib.sha256(d.tobytes()).digest(), np.uint8)
        if len(d) <= max_stored_rows:
            out[name + "/input"] = d
        print("%-28s n %5d  words %3d -> %3d" % (name, len(d), nw, count))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--v1", action="store_true", help="write vocab_quantize_v1.npz as well (default: only compare with it)")
    args = ap.parse_args()
    lib = flann_ref.load()
    if lib is None:
        sys.exit("oracle/_ref/libflann_ref.so is missing: make -C oracle ref")
    v1 = record(lib, list(S.CASES.items()) + [(S.LARGE, S.large_case())], 1000)
    path1 = os.path.join(GOLDEN, "vocab_quantize_v1.npz")
    if args.v1:
        np.savez_compressed(path1, **v1)
        print(path1, os.path.getsize(path1), "bytes")
    else:
        have = np.load(path1)
        assert sorted(have.files) == sorted(v1), "vocab_quantize_v1.npz holds other keys than the cases give"
        for k, v in v1.items():
            assert have[k].dtype == np.asarray(v).dtype and (have[k] == v).all(), "vocab_quantize_v1.npz differs at " + k
        print(path1, "agrees with the reference, left as it is")
    v2 = record(lib, list(S.EDGE_CASES.items()), 300)
    for name in S.EDGE_NAN_CASES:  # no word of an emptied cluster: see above
        d, nw, b, it, seed = S.EDGE_CASES[name]
        R.srand(seed)
        words, centres, _, _ = R.quantize(d, nw, b, it)
        assert np.isfinite(centres).all() and len(words) == int(v2[name + "/count"]) and (words == v2[name + "/words"]).all(), name
    path2 = os.path.join(GOLDEN, "vocab_quantize_v2.npz")
    np.savez_compressed(path2, **v2)
    print(path2, os.path.getsize(path2), "bytes")


if __name__ == "__main__":
    main()
