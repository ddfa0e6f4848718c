"""CPU-only: the public defaults of dsm_extract_covariant_sift, the golden file tests/golden/covdet_vlfeat_v1.npz (its
structure, the coverage conditions its cases are stored for, and -- where the reference tree is present -- that
tools/make_covdet_golden.py reproduces its bytes), and COLMAP's half in tests/covariant_sift_ref.py on hand-built records."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from tests import covariant_sift_ref as ref
from tests import covariant_sift_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE = "/root/reference"


def test_defaults_match_reference():
    # src/feature/sift.h:78-100
    from dagsfm_amd import capi
    o = capi.default_covariant_sift_options()
    assert (o.octave_resolution, o.first_octave, o.max_num_features, o.upright) == (3, -1, 8192, 0)
    assert (o.peak_threshold, o.edge_threshold) == (0.02 / 3, 10.0)
    assert (o.normalization, o.estimate_affine_shape) == (capi.SIFT_L1_ROOT, 0)
    assert (o.dsp_min_scale, o.dsp_max_scale, o.dsp_num_scales) == (1.0 / 6.0, 3.0, 10)
    assert o.domain_size_pooling == 1  # the entry restates the extractor this option selects
    assert ctypes_size(capi.CovariantSiftOptions) == 8 * 4 + 4 * 8


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_golden_file_structure():
    g = ref.golden()
    assert sorted(g) == sorted(name for name, _, _ in scenes.cases())
    assert os.path.getsize(ref.GOLDEN) <= 578734  # the largest golden file before this one
    for name, image, options in scenes.cases():
        c = g[name]
        assert (c["image"] == image).all() and c["options"] == {k: options[k] for k in scenes.OPTION_KEYS}
        counts = c["counts"].tolist()
        assert len(counts) == 6
        for stage, n in zip(ref.STAGES, (counts[0], counts[2], counts[3], counts[3])):
            assert c[stage + "_frames"].shape == (n, 6) and c[stage + "_frames"].dtype == np.float32
            assert c[stage + "_os"].shape == (n, 2) and c[stage + "_os"].dtype == np.int32
            assert c[stage + "_scores"].shape == (n, 3) and c[stage + "_scores"].dtype == np.float32
        assert counts[2] <= counts[0] and counts[0] - counts[2] <= counts[1]  # one feature can be counted as suppressed twice
        assert sorted(c["sorted_index"].tolist()) == list(range(counts[3]))
        assert (c["oriented_frames"][c["sorted_index"]] == c["sorted_frames"]).all()
        scales = options["dsp_num_scales"] if options["domain_size_pooling"] else 1
        assert counts[5] == scales and counts[4] == ref.cut(c["sorted_os"], options["max_num_features"])
        if name in scenes.FLOAT_CASES:
            assert c["raw"].shape == (counts[4], scales, 128) and c["raw"].dtype == np.float32 and "digests" not in c
        else:
            assert c["digests"].shape == (counts[4], 32) and c["digests"].dtype == np.uint8 and "raw" not in c
        # the sort is by (o, s) descending; upright leaves every orientation score at 0
        key = c["sorted_os"][:, 0].astype(np.int64) * 1000 + c["sorted_os"][:, 1]
        assert (np.diff(key) <= 0).all()
        if options["upright"]:
            assert not c["sorted_scores"][:, 2].any() and counts[3] == counts[2]


def test_golden_cases_cover_what_they_are_stored_for():
    g = ref.golden()
    assert any(c["counts"][1] >= 1 for c in g.values())  # a suppressed feature
    assert max(len(set(c["sorted_os"][:c["counts"][4], 0].tolist())) for c in g.values()) >= 3  # three octaves

    def copies(c):  # the copies of one detection share its centre and (o, s)
        keys = [tuple(f[:2].tolist()) + tuple(o.tolist()) for f, o in zip(c["oriented_frames"], c["oriented_os"])]
        return max([keys.count(k) for k in set(keys)] or [0])
    assert copies(g["checker17"]) == 4 and copies(g["checker64"]) == 4

    def padded(name):
        c = g[name]
        o = c["options"]
        h, w = c["image"].shape
        sc = ref.scale_list(o["domain_size_pooling"], o["dsp_min_scale"], o["dsp_max_scale"], o["dsp_num_scales"])
        flags = [ref.patch_is_padded(f, s, w, h, o["first_octave"], o["octave_resolution"]) for f in c["sorted_frames"][:c["counts"][4]] for s in sc]
        return sum(flags), len(flags)
    assert padded("checker17_dsp_off") == (4, 4)  # every patch takes the padded path
    some, total = padded("first0")
    assert 0 < some < total
    assert g["checker17"]["counts"].tolist()[2:] == [1, 4, 4, 10]
    assert g["flat40x30"]["counts"].tolist()[:5] == [0, 0, 0, 0, 0]
    assert g["maxf_octaves"]["counts"][0] < g["mid"]["counts"][0]
    assert g["maxf_groups"]["counts"][4] == scenes.MAXF_BETWEEN_GROUPS + 1 and g["maxf_inside"]["counts"][4] == scenes.MAXF_BETWEEN_GROUPS + 1


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "lib", "VLFeat")), reason="the reference tree is absent")
def test_golden_file_regenerates():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_covdet_golden.py"), "--reference", REFERENCE, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "identical to the committed file" in r.stdout


def f32(x):
    return struct.unpack("<f", struct.pack("<f", x))[0]


def test_scale_list_is_float():
    # sift.cc:530-553: float dsp_min_scale, float dsp_scale_step; the scale is double(min) + s * double(step)
    got = ref.scale_list(1, 1.0 / 6.0, 3.0, 10)
    lo, step = f32(1.0 / 6.0), f32((3.0 - 1.0 / 6.0) / 10)
    assert got == [lo + s * step for s in range(10)] and len(got) == 10
    assert got[0] != 1.0 / 6.0 and got[1] != 1.0 / 6.0 + (3.0 - 1.0 / 6.0) / 10  # the float rounding shows
    got = ref.scale_list(1, 0.3, 2.1, 7)
    assert got == [f32(0.3) + s * f32((2.1 - 0.3) / 7) for s in range(7)] and got[0] != 0.3
    assert ref.scale_list(0, 0.3, 2.1, 7) == [1.0]


def test_pooling_order():
    # an in-order float sum over the scales, then one division: (2^24 + 1) + 1 rounds differently from 1 + 1 + 2^24
    raw = np.zeros((2, 3, 128), np.float32)
    raw[0, :, 0] = [16777216.0, 1.0, 1.0]
    raw[1, :, 0] = [1.0, 1.0, 16777216.0]
    raw[:, :, 5] = [3.0, 4.0, 5.0]
    got = ref.pool(raw)
    assert got.dtype == np.float32 and got.shape == (2, 128)
    assert got[0, 0] == np.float32(16777216.0) / np.float32(3) and got[1, 0] == np.float32(16777218.0) / np.float32(3)
    assert got[0, 5] == np.float32(12.0) / np.float32(3) and not got[:, 1].any()


def test_both_normalisations_and_bytes():
    raw = np.zeros((1, 2, 128), np.float32)
    raw[0, 0, :4] = [0.25, 0.5, 0.0, 0.25]
    raw[0, 1, :4] = [0.75, 0.5, 0.0, 0.25]
    # pooled: 0.5 0.5 0 0.25; L1 root: sqrt(v / 1.25); L2: v / 0.75
    d1 = ref.describe(raw, 1, ref.L1_ROOT)[0]
    d2 = ref.describe(raw, 1, ref.L2)[0]
    ubc = [0, 7, 6, 5]  # VLFeat's bins 0 .. 3 of the first cell in UBC order
    want1 = [int(np.round(512 * np.sqrt(np.float32(v) / np.float32(1.25)))) for v in (0.5, 0.5, 0.0, 0.25)]
    want2 = [min(255, int(np.round(512 * np.float32(v) / np.float32(0.75)))) for v in (0.5, 0.5, 0.0, 0.25)]
    assert [int(d1[k]) for k in ubc] == [min(255, v) for v in want1]
    assert [int(d2[k]) for k in ubc] == want2
    assert d1.sum() == sum(min(255, v) for v in want1) and d1.dtype == np.uint8
    # without pooling the first scale alone counts
    d0 = ref.describe(raw, 0, ref.L2)[0]
    assert [int(d0[k]) for k in ubc] == [min(255, int(np.round(512 * v / np.sqrt(np.float32(0.375))))) for v in (0.25, 0.5, 0.0, 0.25)]


def test_cut_inside_and_between_groups():
    os_ = np.array([[1, 3]] + [[1, 2]] * 2 + [[0, 3]] * 3 + [[0, 1]] * 2, np.int32)  # groups of 1, 2, 3, 2: running totals 1 3 6 8
    assert ref.cut(os_, 8192) == 8
    assert ref.cut(os_, 3) == 4   # between two groups: the feature that opens the next group is pushed before the test
    assert ref.cut(os_, 5) == 7   # inside group (0, 3), which is kept whole -- and the opener of (0, 1) after it
    assert ref.cut(os_, 2) == 2   # the limit is reached by a feature that opens a group itself: the loop ends on it
    assert ref.cut(os_, 4) == 4
    assert ref.cut(os_, 1) == 1   # the first feature differs from INT_MAX
    assert ref.cut(os_, 7) == 7 and ref.cut(os_, 8) == 8
    assert ref.cut(np.zeros((0, 2), np.int32), 5) == 0
    rows = ref.keypoint_rows(np.array([[1.25, 2.5, 1, 0, 0, 1]], np.float32))
    assert rows.tolist() == [[1.75, 3.0, 1, 0, 0, 1]]
