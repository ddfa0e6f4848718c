#!/usr/bin/env python3
"""Writes tests/golden/fivept_ref_digests.npz and tests/golden/ref_misc_answers.npz: what the reference's own code, compiled
behind the shims of oracle/_ref (make -C oracle ref, only where the reference's sources exist), answers for the seeded inputs of
tests/test_fivept_reference_order.py, test_oracle_estimators.py (InlierSupportMeasurer) and test_retrieval.py
(HammingDistWeightFunctor).  The outputs are committed so that every machine checks the oracle against them.

    python tools/make_ref_golden.py"""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_fivept_reference_order as fivept  # noqa: E402
from tests import test_oracle_estimators as estimators  # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref")
OUT = os.path.join(ROOT, "tests", "golden")


def _lib(name):
    path = os.path.join(REF, name)
    assert os.path.exists(path), "build %s first (make -C oracle ref; needs the reference's sources)" % path
    return ctypes.CDLL(path)


def fivept_digests():
    ref = _lib("libfivept_ref.so")
    seen = hashlib.sha256()
    a, c = [], []
    for e, b in fivept.trial_inputs():
        seen.update(e.tobytes())
        seen.update(b.tobytes())
        a_ref = fivept._call(fivept._fn(ref, "ref_fivept_build_A"), e, 200)
        c_ref = fivept._call(fivept._fn(ref, "ref_fivept_coeffs"), b, 11)
        assert not np.isnan(a_ref).any() and not np.isnan(c_ref).any()
        a.append(np.frombuffer(fivept.digest(a_ref), np.uint8))
        c.append(np.frombuffer(fivept.digest(c_ref), np.uint8))
    np.savez_compressed(os.path.join(OUT, "fivept_ref_digests.npz"), a=np.array(a), c=np.array(c),
                        inputs=np.frombuffer(seen.digest(), np.uint8))


def misc_answers():
    ref = _lib("libmisc_ref.so")
    seen = hashlib.sha256()
    supports = []
    for r, thr in estimators.support_inputs():
        seen.update(r.tobytes())
        seen.update(np.float64(thr).tobytes())
        supports.append(estimators.inlier_support(ref, "ref_", r, thr))
    lhs, rhs = estimators.support_compare_sides(supports)
    compare = np.array([[estimators.inlier_support_compare(ref, "ref_", a, b) for b in rhs] for a in lhs], np.int32)
    ref.ref_hamming_weight.restype = ctypes.c_float
    ref.ref_hamming_weight.argtypes = [ctypes.c_uint32]
    ref.ref_max_hamming_distance.restype = ctypes.c_uint32
    np.savez_compressed(os.path.join(OUT, "ref_misc_answers.npz"),
                        support_count=np.array([s[0] for s in supports], np.uint64),
                        support_sum=np.array([s[1] for s in supports], np.float64), support_compare=compare,
                        support_inputs=np.frombuffer(seen.digest(), np.uint8),
                        hamming_weight=np.array([ref.ref_hamming_weight(h) for h in range(65)], np.float32),
                        max_hamming_distance=np.uint32(ref.ref_max_hamming_distance()))


if __name__ == "__main__":
    fivept_digests()
    misc_answers()
