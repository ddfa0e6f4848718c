"""GPU: dsm_extract_covariant_sift_affine against VLFeat's own results (tests/golden/covdet_vlfeat_affine_v1.npz, written by
tools/make_covdet_affine_golden.py from both builds of the reference's VLFeat) carried through COLMAP's host half
(tests/affine_sift_ref.py).  Every comparison is exact: keypoint rows and scores by their float bits, (o, s) and the count as
integers, raw descriptors by their float bits (or the SHA-256 over them where the golden file stores digests), descriptors by
their bytes, the exit counts of the adaptation as integers.  There is no tolerance anywhere in this file.

The cases are at most 200 x 150 pixels: one feature (checker17) and 1024 (tex200x150, whose adaptation has a diverged feature,
seven at the iteration limit and rounds of every length down to a handful of features), patches of the moment kernel that
take the padded path and patches that do not, both pooling settings, first_octave 0, octave_resolution 2, upright, the flat
image, the three max_num_features cuts and the error paths -- each followed by an exact call on the same context."""
import ctypes

import numpy as np
import pytest

from tests import affine_sift_ref as ref
from tests import affine_sift_scenes as scenes
from tests import covariant_sift_ref as v1ref

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
    """One golden case through dsm_extract_covariant_sift_affine, compared field by field; returns (keypoints, descriptors)."""
    case = ref.golden()[name]
    want = ref.expected(case, name)
    kp, desc = c.extract_covariant_sift_affine(case["image"], options_of(case, check=c.check, normalization=normalization), **kw)
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


def check_stats(c, name):
    """affine_shape_stats() of the call just made against the counts of the reference's loop; returns the stats."""
    case = ref.golden()[name]
    n = int(case["counts"][3])
    s = c.affine_shape_stats()
    print(name, s)
    assert tuple(s["exits"][k] for k in c.AFFINE_SHAPE_EXITS) == scenes.EXITS[name]
    assert 1 <= s["rounds"] <= 14 and len(s["active"]) == 14
    assert s["active"][0] == n and all(a >= b for a, b in zip(s["active"], s["active"][1:]))
    assert all(a > 0 for a in s["active"][:s["rounds"]]) and not any(s["active"][s["rounds"]:])
    assert sum(s["exits"].values()) == n
    return s


@pytest.mark.parametrize("name", ALL_CASES)
def test_matches_vlfeat(ctx, name):
    """Every golden case; where the issue's table has the scene, the exits of the adaptation as well."""
    kp, _ = run_case(ctx, name)
    if name != "flat40x30":
        assert len(kp) > 0
    if name in scenes.EXITS:
        s = check_stats(ctx, name)
        if name == "checker64":
            assert s["active"][0] - s["active"][1] == scenes.CHECKER64_CONVERGED_AT_FIRST_TEST
        if name == "checker17":
            assert s["rounds"] == 6 and s["active"][:6] == [1] * 6  # converges after six moment computations
    elif name in ("flat40x30", "upright"):
        s = ctx.affine_shape_stats()  # no adaptation ran
        assert s["rounds"] == 0 and not any(s["active"]) and not any(s["exits"].values())


def test_l2_against_l1_root(ctx):
    a = run_case(ctx, "first0", normalization=ref.L1_ROOT)[1]
    b = run_case(ctx, "first0", normalization=ref.L2)[1]
    assert (a != b).any()
    run_case(ctx, "mid", normalization=ref.L2)


@pytest.mark.parametrize("name", ["mid", "checker17"])
@pytest.mark.parametrize("how", ["flag_off", "upright"])
def test_without_the_adaptation_equals_the_old_entry(ctx, name, how):
    """estimate_affine_shape = 0, and upright = 1 with the flag, return what dsm_extract_covariant_sift returns."""
    case = v1ref.golden()[name]
    scales = int(case["counts"][5])
    kw = dict(estimate_affine_shape=0) if how == "flag_off" else dict(upright=1)
    old_kp, old_desc = ctx.extract_covariant_sift(case["image"], options_of(case, **dict(kw, estimate_affine_shape=0)))
    old_raw = ctx.covariant_sift_raw(num_scales=scales)
    new_kp, new_desc = ctx.extract_covariant_sift_affine(case["image"], options_of(case, **dict(dict(estimate_affine_shape=1), **kw)))
    new_raw = ctx.covariant_sift_raw(num_scales=scales)
    assert len(old_kp) > 0
    assert_rows(new_kp, old_kp, "keypoint rows")
    assert_rows(new_desc, old_desc, "descriptor bytes")
    for k in ("octave_scale", "scores", "raw"):
        assert_rows(new_raw[k], old_raw[k], k)
    s = ctx.affine_shape_stats()
    assert s["rounds"] == 0 and not any(s["active"]) and not any(s["exits"].values())


def test_old_entry_still_refuses_then_exact_call(ctx):
    from dagsfm_amd import capi
    mid = ref.golden()["mid"]["image"]
    h, w = mid.shape
    kp = np.zeros((64, 6), np.float32)
    n = ctypes.c_uint32(7)
    o = capi.default_covariant_sift_options(estimate_affine_shape=1)
    rc = ctx._L.dsm_extract_covariant_sift(ctx._h, ctypes.byref(o), np.ascontiguousarray(mid).ctypes.data, w, h, w, 64, kp.ctypes.data, None,
                                           ctypes.byref(n))
    assert rc == 1 and "not covered" in ctx._L.dsm_last_error(ctx._handle).decode()
    assert n.value == 0 and not kp.any()
    run_case(ctx, "mid")
    check_stats(ctx, "mid")


def test_flat_image_then_exact_call(ctx):
    kp, desc = run_case(ctx, "flat40x30")
    assert kp.shape == (0, 6) and desc.shape == (0, 128)
    run_case(ctx, "checker17")


def test_capacity_one_below_the_count(ctx):
    from dagsfm_amd import capi
    case = ref.golden()["first0"]
    n = int(case["counts"][4])
    with pytest.raises(capi.DsmError) as e:
        ctx.extract_covariant_sift_affine(case["image"], options_of(case), capacity=n - 1)
    assert e.value.status == 4 and e.value.num_features == n
    kp, desc = e.value.outputs
    assert not kp.any() and not desc.any()  # outputs untouched
    with pytest.raises(capi.DsmError, match="dsm error 5"):  # a failed call leaves no result behind
        ctx.covariant_sift_raw()
    with pytest.raises(capi.DsmError, match="dsm error 5"):
        ctx.affine_shape_stats()
    run_case(ctx, "first0")
    check_stats(ctx, "first0")


def test_keypoints_only_and_row_stride(ctx):
    from dagsfm_amd import capi
    case = ref.golden()["mid"]
    want = ref.expected(case, "mid")
    kp, desc = ctx.extract_covariant_sift_affine(case["image"], options_of(case), descriptors=False)
    assert desc is None
    assert_rows(kp, want["keypoints"], "keypoint rows")
    assert_rows(ctx.covariant_sift_raw()["octave_scale"], want["os"], "(o, s)")
    check_stats(ctx, "mid")
    with pytest.raises(capi.DsmError, match="dsm error 5"):  # no raw descriptors after a keypoints-only call
        ctx.covariant_sift_raw(num_scales=10)
    h, w = case["image"].shape
    wide = np.full((h, w + 13), 255, np.uint8)
    wide[:, :w] = case["image"]
    kp2, desc2 = ctx.extract_covariant_sift_affine(wide, options_of(case), width=w)
    kp1, desc1 = run_case(ctx, "mid")
    assert_rows(kp2, kp1, "keypoint rows with row_stride > width")
    assert_rows(desc2, desc1, "descriptor bytes with row_stride > width")


def test_stats_not_ready_before_an_affine_call():
    from dagsfm_amd import capi
    c = capi.Context(0)
    try:
        with pytest.raises(capi.DsmError, match="dsm error 5"):
            c.affine_shape_stats()
        case = v1ref.golden()["checker17"]
        c.extract_covariant_sift(case["image"], options_of(case))  # the old entry is no such call
        with pytest.raises(capi.DsmError, match="dsm error 5"):
            c.affine_shape_stats()
        run_case(c, "checker17")
        check_stats(c, "checker17")
        t = c.covariant_sift_time()
        assert set(t) == set(c.COVARIANT_SIFT_STAGES) and all(v >= 0 for v in t.values()) and t["orientations"] > 0
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
            check_stats(c, "first0")
        finally:
            c.close()
    assert_rows(out[0][0], out[1][0], "keypoint rows of the two builds")
    assert_rows(out[0][1], out[1][1], "descriptor bytes of the two builds")
