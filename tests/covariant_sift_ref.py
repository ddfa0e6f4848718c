"""COLMAP's half of ExtractCovariantSiftFeaturesCPU (src/feature/sift.cc:475-594) in numpy, on top of VLFeat's own output as
tests/golden/covdet_vlfeat_v1.npz stores it (tools/make_covdet_golden.py): the cut at sift.cc:503-511 that keeps the crossing
(o, s) group whole, the keypoint rows (:494-501), the pooling scales in float (:530-553), the pooling (Eigen's
colwise().mean(): an in-order float sum over the scales, one float division), L1_ROOT / L2, the bytes and the UBC order
(tests/sift_ref.py has the last three).  The expected features of a case are the reference library's values carried through
this host half -- the same structure as the host half of dagsfm_amd/csrc/covariant_sift.hip.

patch_is_padded restates the level choice and the box test of vl_covdet_extract_patch_helper (covdet.c:2222-2304) so that the
tool can say which patches took the padded path.
"""
import hashlib
import math
import os

import numpy as np

from tests import sift_ref
from tests.covariant_sift_scenes import FLOAT_CASES, OPTION_KEYS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "covdet_vlfeat_v1.npz")
L1_ROOT, L2 = 0, 1
STAGES = ("detected", "suppressed", "oriented", "sorted")
INT_OPTIONS = OPTION_KEYS[:6]
_golden = {}


def golden(path=GOLDEN):
    """{case: {image, options (dict), counts, <stage>_frames, <stage>_os, <stage>_scores, sorted_index, raw | digests}} -- loaded once,
    shared, read-only."""
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


def scale_list(domain_size_pooling, dsp_min_scale, dsp_max_scale, dsp_num_scales):
    """The pooling scales as doubles (sift.cc:530-553): dsp_min_scale and dsp_scale_step are float variables."""
    if not domain_size_pooling:
        return [1.0]
    lo = np.float32(dsp_min_scale)
    step = np.float32((float(dsp_max_scale) - float(dsp_min_scale)) / int(dsp_num_scales))
    return [float(lo) + s * float(step) for s in range(int(dsp_num_scales))]


def pool(raw):
    """colwise().mean() of float32 [n, scales, 128]: the scales added in order, then one division by their number."""
    raw = np.asarray(raw, np.float32)
    acc = raw[:, 0, :].copy()
    for s in range(1, raw.shape[1]):
        acc = acc + raw[:, s, :]
    return (acc / np.float32(raw.shape[1])).astype(np.float32)


def cut(os_sorted, max_num_features):
    """The number of features sift.cc:493-513 keeps of the sorted list [n, 2] of (o, s)."""
    kept, prev = 0, 2 ** 31 - 1  # prev_octave_scale_idx starts at INT_MAX: the first feature differs from it
    for o, s in np.asarray(os_sorted).reshape(-1, 2).tolist():
        kept += 1
        idx = o * 1000 + s
        if idx != prev and kept >= max_num_features:
            break
        prev = idx
    return kept


def keypoint_rows(frames):
    """FeatureKeypoint rows (sift.cc:494-501): x + 0.5 and y + 0.5 in double, narrowed to float."""
    f = np.asarray(frames, np.float32).reshape(-1, 6)
    out = f.copy()
    out[:, 0] = (f[:, 0].astype(np.float64) + 0.5).astype(np.float32)
    out[:, 1] = (f[:, 1].astype(np.float64) + 0.5).astype(np.float32)
    return out


def describe(raw, domain_size_pooling, normalization):
    """uint8 [n, 128] in UBC order from VLFeat's raw descriptors float32 [n, scales, 128]."""
    raw = np.asarray(raw, np.float32)
    d = pool(raw) if domain_size_pooling else raw[:, 0, :]
    b = sift_ref.to_unsigned_byte(sift_ref.normalize(d.reshape(-1, 128), normalization))
    ubc = np.zeros_like(b)
    ubc[:, sift_ref.ubc_permutation()] = b
    return ubc


def digest(raw_rows):
    """One SHA-256 per feature over its [scales x 128] little-endian floats: uint8 [n, 32]."""
    raw_rows = np.ascontiguousarray(raw_rows, "<f4")
    return np.array([np.frombuffer(hashlib.sha256(r.tobytes()).digest(), np.uint8) for r in raw_rows], np.uint8).reshape(-1, 32)


def expected(case, name):
    """What dsm_extract_covariant_sift and dsm_get_covariant_sift_raw return for golden()[name], without the descriptor bytes
    where the case stores digests only: {n, keypoints, os, scores, raw or None, digests}."""
    n = int(case["counts"][4])
    out = {"n": n, "keypoints": keypoint_rows(case["sorted_frames"][:n]), "os": case["sorted_os"][:n], "scores": case["sorted_scores"][:n]}
    assert cut(case["sorted_os"], case["options"]["max_num_features"]) == n or len(case["sorted_os"]) == 0
    out["raw"] = case["raw"] if name in FLOAT_CASES else None
    out["digests"] = digest(case["raw"]) if name in FLOAT_CASES else case["digests"]
    return out


# ---- the patch geometry (covdet.c:2222-2304), for the tool's coverage conditions


def _geometry(width, height, first_octave, octave_resolution):
    last = int(math.floor(math.log2(min(width - 1.0, height - 1.0) / 15.0)))  # covdet.c:1699
    return dict(first=first_octave, last=last, R=octave_resolution, base=1.6 * math.pow(2.0, 1.0 / octave_resolution), smin=-1,
                smax=octave_resolution + 1)


def patch_is_padded(frame, scale, width, height, first_octave, octave_resolution, extent=7.5, sigma=1.0):
    """Whether vl_covdet_extract_patch_for_frame builds the padded copy for `frame` (x, y, a11, a12, a21, a22) times `scale`."""
    g = _geometry(width, height, first_octave, octave_resolution)
    x, y, a11, a12, a21, a22 = (float(np.float32(v)) for v in frame)
    a11, a12, a21, a22 = (float(np.float32(v * scale)) for v in (a11, a12, a21, a22))
    d = np.linalg.svd(np.array([[a11, a12], [a21, a22]]), compute_uv=False)
    factor = 1.0 / float(min(abs(d[0]), abs(d[1])))

    def level(o):
        s = int(math.floor(math.log2(sigma / (factor * g["base"])) - o))
        return max(g["smin"], min(s, g["smax"]))

    o = g["first"] + 1
    while o <= g["last"]:
        if factor * g["base"] * math.pow(2.0, o + level(o) / g["R"]) > sigma:
            o -= 1
            break
        o += 1
    o = min(o, g["last"])
    step = math.pow(2.0, o)
    w = (width >> o) if o >= 0 else (width << -o)
    h = (height >> o) if o >= 0 else (height << -o)
    A = [a11 / step, a21 / step, a12 / step, a22 / step]
    T = [x / step, y / step]
    xs = [A[0] * bx + A[2] * by + T[0] for bx, by in ((extent, -extent), (extent, extent), (-extent, extent), (-extent, -extent))]
    ys = [A[1] * bx + A[3] * by + T[1] for bx, by in ((extent, -extent), (extent, extent), (-extent, extent), (-extent, -extent))]
    x0i, y0i = math.floor(min(xs)) - 1, math.floor(min(ys)) - 1
    x1i, y1i = math.ceil(max(xs)) + 1, math.ceil(max(ys)) + 1
    return x0i < 0 or x1i > w - 1 or y0i < 0 or y1i > h - 1
