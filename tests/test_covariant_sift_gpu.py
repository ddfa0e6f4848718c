"""GPU: dsm_extract_covariant_sift against VLFeat's own results (tests/golden/covdet_vlfeat_v1.npz, written by
tools/make_covdet_golden.py from both builds of the reference's VLFeat) carried through COLMAP's host half
(tests/covariant_sift_ref.py).  Every comparison is exact: keypoint rows and scores by their float bits, (o, s) and the count
as integers, raw descriptors by their float bits (or the SHA-256 over them where the golden file stores digests), descriptors
by their bytes, all in output order.  There is no tolerance anywhere in this file.

The cases are small and chosen where the stage can go wrong: a 17 x 17 image (one detection, four orientations, 40 items),
patches that all take the padded path and patches that do not, features in four octaves, suppressed detections, item counts
that are no multiple of a wave (4 x 10, 12 x 10, 113 x 3 ...), a flat image, every option, the three max_num_features cuts and
the error paths -- each followed by an exact call on the same context."""
import ctypes

import numpy as np
import pytest

from tests import covariant_sift_ref as ref
from tests import covariant_sift_scenes as scenes

pytestmark = pytest.mark.gpu

ALL_CASES = [name for name, _, _ in scenes.cases()]


@pytest.fixture(scope="module")
def ctx():
    from dagsfm_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def options_of(case, check=False, **kw):
    from dagsfm_amd import capi
    o = capi.default_covariant_sift_options(check=check)
    for k, v in case["options"].items():
        setattr(o, k, v)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_rows(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if len(got) == 0:
        return
    bad = np.nonzero((bits(got) != bits(want)).reshape(len(got), -1).any(axis=1))[0] if got.dtype == np.float32 else np.nonzero(
        (got != want).reshape(len(got), -1).any(axis=1))[0]
    assert len(bad) == 0, "%s differ in rows %s (of %d)" % (what, bad[:8], len(got))


def run_case(c, name, normalization=ref.L1_ROOT, **kw):
    """One golden case through the device, compared field by field; returns (keypoints, descriptors)."""
    case = ref.golden()[name]
    want = ref.expected(case, name)
    kp, desc = c.extract_covariant_sift(case["image"], options_of(case, check=c.check, normalization=normalization), **kw)
    assert len(kp) == want["n"], (len(kp), want["n"])
    assert_rows(kp, want["keypoints"], "keypoint rows")
    scales = int(case["counts"][5])
    raw = c.covariant_sift_raw(num_scales=scales)
    assert_rows(raw["octave_scale"], want["os"], "(o, s)")
    assert_rows(raw["scores"], want["scores"], "scores (peak, edge, orientation)")
    if want["raw"] is not None:
        assert_rows(raw["raw"].reshape(want["n"], -1), want["raw"].reshape(want["n"], -1), "raw descriptors")
        assert_rows(desc, ref.describe(want["raw"], case["options"]["domain_size_pooling"], normalization), "descriptor bytes")
    else:
        assert_rows(ref.digest(raw["raw"]), want["digests"], "raw descriptor digests")
        # the digests hold the floats: the bytes follow from the device's own (verified) floats through the host half
        assert_rows(desc, ref.describe(raw["raw"], case["options"]["domain_size_pooling"], normalization), "descriptor bytes")
    return kp, desc


@pytest.mark.parametrize("name", ALL_CASES)
def test_matches_vlfeat(ctx, name):
    """Every golden case, which covers upright, domain_size_pooling = 0, dsp_num_scales 1 / 3 / 4 / 10, first_octave -1 / 0,
    octave_resolution 2 / 3, the three max_num_features cuts, the 17 x 17 image and the flat one."""
    kp, _ = run_case(ctx, name)
    if name != "flat40x30":
        assert len(kp) > 0


def test_cases_are_what_they_are_stored_for():
    g = ref.golden()
    assert g["checker17"]["counts"][4] == 4 and g["checker17"]["counts"][5] == 10  # 40 items: under one wave of items
    assert g["scales3"]["counts"][4] * 3 % 64 != 0 and g["first0"]["counts"][4] * 10 % 64 != 0
    assert g["maxf_octaves"]["counts"][0] < g["mid"]["counts"][0]  # the detection loop stopped early
    assert g["maxf_groups"]["counts"][4] == scenes.MAXF_BETWEEN_GROUPS + 1 == g["maxf_inside"]["counts"][4]
    assert g["flat40x30"]["counts"][0] == 0


def test_l2_against_l1_root(ctx):
    a = run_case(ctx, "first0", normalization=ref.L1_ROOT)[1]
    b = run_case(ctx, "first0", normalization=ref.L2)[1]
    assert (a != b).any()
    run_case(ctx, "mid", normalization=ref.L2)


def test_keypoints_only_and_row_stride(ctx):
    from dagsfm_amd import capi
    case = ref.golden()["mid"]
    want = ref.expected(case, "mid")
    kp, desc = ctx.extract_covariant_sift(case["image"], options_of(case), descriptors=False)
    assert desc is None
    assert_rows(kp, want["keypoints"], "keypoint rows")
    assert_rows(ctx.covariant_sift_raw()["octave_scale"], want["os"], "(o, s)")
    with pytest.raises(capi.DsmError, match="dsm error 5"):  # no raw descriptors after a keypoints-only call
        ctx.covariant_sift_raw(num_scales=10)
    h, w = case["image"].shape
    wide = np.full((h, w + 13), 255, np.uint8)
    wide[:, :w] = case["image"]
    kp2, desc2 = ctx.extract_covariant_sift(wide, options_of(case), width=w)
    kp1, desc1 = run_case(ctx, "mid")
    assert_rows(kp2, kp1, "keypoint rows with row_stride > width")
    assert_rows(desc2, desc1, "descriptor bytes with row_stride > width")


def test_flat_image_then_exact_call(ctx):
    kp, desc = run_case(ctx, "flat40x30")
    assert kp.shape == (0, 6) and desc.shape == (0, 128)
    run_case(ctx, "checker17")


def test_capacity_one_below_the_count(ctx):
    from dagsfm_amd import capi
    case = ref.golden()["first0"]
    n = int(case["counts"][4])
    with pytest.raises(capi.DsmError) as e:
        ctx.extract_covariant_sift(case["image"], options_of(case), capacity=n - 1)
    assert e.value.status == 4 and e.value.num_features == n
    kp, desc = e.value.outputs
    assert not kp.any() and not desc.any()  # outputs untouched
    with pytest.raises(capi.DsmError, match="dsm error 5"):  # a failed call leaves no result behind
        ctx.covariant_sift_raw()
    run_case(ctx, "first0")


def _raw_call(c, image, o, width=None, stride=None):
    h, w = image.shape
    kp = np.zeros((64, 6), np.float32)
    n = ctypes.c_uint32(7)
    rc = c._L.dsm_extract_covariant_sift(c._h, ctypes.byref(o), np.ascontiguousarray(image).ctypes.data, w if width is None else width, h,
                                         w if stride is None else stride, 64, kp.ctypes.data, None, ctypes.byref(n))
    return rc, n.value, kp


@pytest.mark.parametrize("what", ["affine_shape", "aborting_shape", "check_rejects", "stride_below_width"])
def test_errors_then_exact_call(ctx, what):
    from dagsfm_amd import capi
    from tests import sift_scenes
    mid = ref.golden()["mid"]["image"]
    if what == "affine_shape":
        rc, n, kp = _raw_call(ctx, mid, capi.default_covariant_sift_options(estimate_affine_shape=1))
        assert rc == 1 and "not covered" in ctx._L.dsm_last_error(ctx._handle).decode()
    elif what == "aborting_shape":  # the reference dies on the assertion at scalespace.c:396
        rc, n, kp = _raw_call(ctx, sift_scenes.texture(12, 40, 3), capi.default_covariant_sift_options(first_octave=-1))
        assert rc == 4
        rc2, _, _ = _raw_call(ctx, sift_scenes.texture(30, 40, 3), capi.default_covariant_sift_options(first_octave=1))  # no octave at all: 29 < 15 * 2
        assert rc2 == 4
    elif what == "check_rejects":
        for bad in (dict(max_num_features=0), dict(octave_resolution=0), dict(peak_threshold=0.0), dict(edge_threshold=-1.0),
                    dict(dsp_min_scale=0.0), dict(dsp_max_scale=0.1), dict(dsp_num_scales=0), dict(normalization=2)):
            rc, n, kp = _raw_call(ctx, mid, capi.default_covariant_sift_options(**bad))
            assert rc == 1, bad
        # without domain_size_pooling the reference does not look at the dsp fields
        rc, n, kp = _raw_call(ctx, ref.golden()["first0"]["image"], options_of(ref.golden()["first0"], domain_size_pooling=0, dsp_num_scales=0))
        assert rc == 0 and n > 0
        run_case(ctx, "first0")
        return
    else:
        rc, n, kp = _raw_call(ctx, mid, capi.default_covariant_sift_options(), stride=mid.shape[1] - 1)
        assert rc == 1
    assert n == 0 and not kp.any()
    run_case(ctx, "first0")


def test_not_ready_before_any_call():
    from dagsfm_amd import capi
    c = capi.Context(0)
    try:
        with pytest.raises(capi.DsmError, match="dsm error 5"):
            c.covariant_sift_raw()
        with pytest.raises(capi.DsmError, match="dsm error 5"):
            c.covariant_sift_time()
        run_case(c, "checker17")
        t = c.covariant_sift_time()
        assert set(t) == set(c.COVARIANT_SIFT_STAGES) and all(v >= 0 for v in t.values()) and t["descriptors"] > 0
    finally:
        c.close()


def test_both_builds_agree():
    """The product and the check library give identical bytes on one case."""
    from dagsfm_amd import capi
    out = []
    for check in (False, True):
        c = capi.Context(0, check=check)
        try:
            out.append(run_case(c, "first0"))
        finally:
            c.close()
    assert_rows(out[0][0], out[1][0], "keypoint rows of the two builds")
    assert_rows(out[0][1], out[1][1], "descriptor bytes of the two builds")
