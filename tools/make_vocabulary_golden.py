#!/usr/bin/env python3
"""Records the reference's own VisualIndex::Quantize answers for the cases of tests/vocabulary_build_scenes.py into
tests/golden/vocab_quantize_v1.npz.  Needs oracle/_ref/libflann_ref.so (make -C oracle ref, where the reference lies).

Per case: options = (n, num_visual_words, branching, num_iterations, srand seed), the reference's count and words, the first 8
values of rand() after srand(seed), the SHA-256 of the input bytes, and the input itself for the cases of at most 1000
descriptors (the larger inputs are regenerated from their seed and held to the hash: all of them would pass the size the
golden files keep to)."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import flann_ref, vocabulary_build_ref as R, vocabulary_build_scenes as S  # noqa: E402


def main():
    lib = flann_ref.load()
    if lib is None:
        sys.exit("oracle/_ref/libflann_ref.so is missing: make -C oracle ref")
    out = {}
    for name, (d, nw, b, it, seed) in list(S.CASES.items()) + [(S.LARGE, S.large_case())]:
        words = np.zeros((nw, 128), np.uint8)
        lib.flann_ref_seed(seed)
        count = lib.flann_ref_quantize(d.ctypes.data, len(d), nw, b, it, words.ctypes.data)
        R.srand(seed)
        out[name + "/rand8"] = np.array([R.libc_rand() for _ in range(8)], np.int64)
        out[name + "/options"] = np.array([len(d), nw, b, it, seed], np.int64)
        out[name + "/count"] = np.int64(count)
        out[name + "/words"] = words[:count].copy()
        out[name + "/input_sha256"] = np.frombuffer(hashlib.sha256(d.tobytes()).digest(), np.uint8)
        if len(d) <= 1000:
            out[name + "/input"] = d
        print("%-28s n %5d  words %3d -> %3d" % (name, len(d), nw, count))
    path = os.path.join(ROOT, "tests", "golden", "vocab_quantize_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
