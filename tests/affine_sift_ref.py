"""COLMAP's half of ExtractCovariantSiftFeaturesCPU with estimate_affine_shape = true, on top of VLFeat's own output as
tests/golden/covdet_vlfeat_affine_v1.npz stores it (tools/make_covdet_affine_golden.py).  The half itself -- the cut, the
keypoint rows, the pooling, the normalisations, the bytes -- does not depend on the option and is tests/covariant_sift_ref.py's;
this module adds the file, its stage names and the expected record of a case."""
import os

import numpy as np

from tests import covariant_sift_ref as base
from tests.affine_sift_scenes import FLOAT_CASES, OPTION_KEYS
from tests.covariant_sift_ref import L1_ROOT, L2, cut, describe, digest, keypoint_rows, patch_is_padded, pool, scale_list  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covdet_vlfeat_affine_v1.npz")
STAGES = ("adapted", "sorted")  # after vl_covdet_extract_affine_shape, after COLMAP's std::sort
INT_OPTIONS = base.INT_OPTIONS + ("estimate_affine_shape",)
_golden = {}


def golden(path=GOLDEN):
    """{case: {image, options (dict), counts, adapted_*, sorted_* (frames, os, scores), sorted_index, raw | digests}} -- loaded
    once, shared, read-only."""
    if path not in _golden:
        z = np.load(path)
        out = {}
        for key in z.files:
            case, field = key.split("/")
            a = z[key]
            a.setflags(write=False)
            out.setdefault(case, {})[field] = a
        for case in out.values():
            o = dict(zip(OPTION_KEYS, case["options"].tolist()))
            for k in INT_OPTIONS:
                o[k] = int(o[k])
            case["options"] = o
        _golden[path] = out
    return _golden[path]


def expected(case, name):
    """What dsm_extract_covariant_sift_affine and dsm_get_covariant_sift_raw return for golden()[name]: {n, keypoints, os,
    scores, raw or None, digests}."""
    n = int(case["counts"][4])
    out = {"n": n, "keypoints": keypoint_rows(case["sorted_frames"][:n]), "os": case["sorted_os"][:n], "scores": case["sorted_scores"][:n]}
    assert cut(case["sorted_os"], case["options"]["max_num_features"]) == n or len(case["sorted_os"]) == 0
    out["raw"] = case["raw"] if name in FLOAT_CASES else None
    out["digests"] = digest(case["raw"]) if name in FLOAT_CASES else case["digests"]
    return out
