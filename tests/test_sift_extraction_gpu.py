"""GPU: dsm_extract_sift against VLFeat's own results (tests/golden/sift_vlfeat_v1.npz, written by tools/make_sift_golden.py from
both builds of the reference's VLFeat) carried through COLMAP's host half (tests/sift_ref.py).  Every comparison is exact:
keypoints by their float bits, descriptors by their bytes, in order.

The cases are small on purpose and chosen where the kernels can go wrong: odd sizes that are no multiple of a block or a wave
(37 x 29, 65 x 63), a wide thin image whose filter half-width exceeds its height in the upper octaves (130 x 20), octaves that
shrink to a few pixels (16 x 16, four octaves), a constant image (no candidate: no launch of size zero), structure within 3
pixels of the borders only (one-sided gradients, clipped windows, the bound checks of sift.c:1976-1983), and every option.

The second half runs the cases of tests/golden/sift_vlfeat_v2.npz (sift_scenes.cases_v2(); tests/test_sift_extraction_v2_cpu.py
shows that each reaches the path it is stored for): first_octave -3, -2, 2 and 3, num_octaves -1, 0, 1 and 10, images whose
octaves fall under 3 and under 2 samples, a checkerboard and dots whose DoG samples and histogram bins tie, keypoints with four
orientations, a compaction chunk with many candidates, and the range errors."""
import ctypes

import numpy as np
import pytest

from tests import sift_ref

pytestmark = pytest.mark.gpu

DEFAULT_CASES = ["tex96x80", "tex64x48", "tex64x48_b", "odd37x29", "odd65x63", "thin130x20", "tiny16x16", "constant40x30", "border48x40"]
OPTION_CASES = ["first0", "first1", "res2", "res5", "upright", "single"]


@pytest.fixture(scope="module")
def ctx():
    from dagsfm_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def options_of(case, **kw):
    from dagsfm_amd import capi
    o = capi.default_sift_options()
    for k, v in case["options"].items():
        setattr(o, k, v)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def assert_same(got, want):
    (kp, d), (rkp, rd) = got, want
    assert kp.dtype == np.float32 and kp.shape == rkp.shape, (kp.shape, rkp.shape)
    assert (kp.view(np.uint32) == rkp.view(np.uint32)).all(), "keypoint bits differ in rows %s" % np.nonzero(
        (kp.view(np.uint32) != rkp.view(np.uint32)).any(axis=1))[0][:8]
    if rd is not None:
        assert d.dtype == np.uint8 and d.shape == rd.shape
        assert (d == rd).all(), "descriptor bytes differ in rows %s" % np.nonzero((d != rd).any(axis=1))[0][:8]


@pytest.mark.parametrize("name", DEFAULT_CASES + OPTION_CASES)
def test_matches_vlfeat(ctx, name):
    case = sift_ref.golden()[name]
    want = sift_ref.assemble(case)
    if name not in ("constant40x30",):
        assert len(want[0]) > 0
    assert_same(ctx.extract_sift(case["image"], options_of(case)), want)


EXTRA = {  # shapes and options the golden file does not store: the device against the numpy restatement (tests/sift_ref.py)
    "53x41": (lambda sc: sc.texture(53, 41, 9), {}),
    "257x19": (lambda sc: sc.texture(257, 19, 11), {}),                      # one lane past a 256-wide row tile; thinner than a 16-row tile
    "33x70_first0_res4": (lambda sc: sc.texture(33, 70, 12), dict(first_octave=0, octave_resolution=4, peak_threshold=0.02 / 4)),
    "48x48_res1": (lambda sc: sc.texture(48, 48, 13), dict(octave_resolution=1, peak_threshold=0.02)),  # half-width 45: above the image in octave 1
    "border31x23": (lambda sc: sc.border_only(31, 23, 14), {}),
}


@pytest.mark.parametrize("name", sorted(EXTRA))
def test_matches_restatement_on_other_shapes(ctx, name):
    from dagsfm_amd import capi
    from tests import sift_scenes
    make, opts = EXTRA[name]
    image = make(sift_scenes)
    full = dict(sift_scenes.DEFAULTS, **opts)
    assert_same(ctx.extract_sift(image, capi.default_sift_options(**full)), sift_ref.extract(image, full))


def test_stage_times_are_reported(ctx):
    case = sift_ref.golden()["tex64x48"]
    ctx.extract_sift(case["image"], options_of(case))
    t = ctx.sift_time()
    assert sorted(t) == sorted(ctx.SIFT_STAGES) and all(v >= 0 for v in t.values()) and t["smoothing"] > 0 and t["descriptors"] > 0


@pytest.mark.parametrize("max_num_orientations", [1, 4])
def test_max_num_orientations(ctx, max_num_orientations):
    case = sift_ref.golden()["tex96x80"]
    assert_same(ctx.extract_sift(case["image"], options_of(case, max_num_orientations=max_num_orientations)),
                sift_ref.assemble(case, max_num_orientations=max_num_orientations))


def test_l2_normalization(ctx):
    from dagsfm_amd import capi
    case = sift_ref.golden()["tex64x48"]
    assert_same(ctx.extract_sift(case["image"], options_of(case, normalization=capi.SIFT_L2)), sift_ref.assemble(case, normalization=sift_ref.L2))


@pytest.mark.parametrize("limit", [30, 1])
def test_max_num_features_cuts_levels(ctx, limit):
    case = sift_ref.golden()["tex64x48"]
    want = sift_ref.assemble(case, max_num_features=limit)
    assert limit < len(want[0]) < len(sift_ref.assemble(case)[0])
    assert_same(ctx.extract_sift(case["image"], options_of(case, max_num_features=limit)), want)


def test_row_stride_above_width(ctx):
    case = sift_ref.golden()["odd37x29"]
    h, w = case["image"].shape
    padded = np.full((h, w + 11), 201, np.uint8)
    padded[:, :w] = case["image"]
    assert_same(ctx.extract_sift(padded, options_of(case), width=w), sift_ref.assemble(case))


def test_keypoints_without_descriptors(ctx):
    case = sift_ref.golden()["odd65x63"]
    kp, d = ctx.extract_sift(case["image"], options_of(case), descriptors=False)
    assert d is None
    assert_same((kp, None), (sift_ref.assemble(case)[0], None))


def test_capacity_too_small_reports_the_count(ctx):
    from dagsfm_amd import capi
    case = sift_ref.golden()["tex64x48"]
    want = len(sift_ref.assemble(case)[0])
    with pytest.raises(capi.DsmError) as e:
        ctx.extract_sift(case["image"], options_of(case), capacity=want - 1)
    assert e.value.status == 4 and e.value.num_features == want
    assert_same(ctx.extract_sift(case["image"], options_of(case), capacity=want), sift_ref.assemble(case))


def test_large_small_large_on_one_context(ctx):
    """Stale scratch or a stale filter of the larger call would show in the smaller one, and the other way round."""
    g = sift_ref.golden()
    for name in ("tex96x80", "tiny16x16", "res5", "odd37x29", "tex96x80"):
        assert_same(ctx.extract_sift(g[name]["image"], options_of(g[name])), sift_ref.assemble(g[name]))


def test_invalid_options_are_an_error_status(ctx):
    """SiftExtractionOptions::Check (sift.cc:218-234) as a status, never an abort."""
    from dagsfm_amd import capi
    im = sift_ref.golden()["tiny16x16"]["image"]
    for bad in (dict(max_num_features=0), dict(octave_resolution=0), dict(peak_threshold=0.0), dict(edge_threshold=-1.0),
                dict(max_num_orientations=0), dict(normalization=2), dict(peak_threshold=float("nan"))):
        with pytest.raises(capi.DsmError) as e:
            ctx.extract_sift(im, capi.default_sift_options(**bad))
        assert e.value.status == 1, bad
    with pytest.raises(capi.DsmError) as e:
        ctx.extract_sift(im, capi.default_sift_options(first_octave=-9))
    assert e.value.status == 4
    n = ctypes.c_uint32(0)
    assert capi.lib(ctx.check).dsm_extract_sift(ctx._h, None, None, 16, 16, 16, 0, None, None, ctypes.byref(n)) == 1


def test_memory_budget_is_honoured_by_an_error(ctx):
    from dagsfm_amd import capi
    case = sift_ref.golden()["tex96x80"]
    ctx.set_memory_budget(100000)  # the first octave of 192 x 160 needs about 1.9 MB
    try:
        with pytest.raises(capi.DsmError) as e:
            ctx.extract_sift(case["image"], options_of(case))
        assert e.value.status == 4
    finally:
        ctx.set_memory_budget(0)
    assert_same(ctx.extract_sift(case["image"], options_of(case)), sift_ref.assemble(case))


def test_extracted_features_feed_the_matcher(ctx):
    """extract_sift on two images, handed to set_images and match_pairs, gives the matches the oracle matcher finds on the
    reference's features of the same images: the link to the existing stage."""
    from dagsfm_amd import capi
    from tests import oracle_lib
    g = sift_ref.golden()
    a, b = g["tex64x48"], g["tex64x48_b"]
    feats = [ctx.extract_sift(c["image"], options_of(c)) for c in (a, b)]
    want = [sift_ref.assemble(c) for c in (a, b)]
    m = capi.Context(0)
    try:
        m.set_images([f[1] for f in feats], [f[0][:, :2] for f in feats])
        m.match_pairs(np.array([[0, 1]], np.uint32))
        offs, got = m.matches()
    finally:
        m.close()
    ref = oracle_lib.load().match_sift_features_cpu(want[0][1], want[1][1])
    got = got[int(offs[0]):int(offs[1])]
    assert got.shape == ref.shape and (got == ref).all()


# ---------------------------------------------------------------------------------------------------------------------------
# tests/golden/sift_vlfeat_v2.npz

from tests import sift_scenes  # noqa: E402

V2_CASES = [name for name, _, _ in sift_scenes.cases_v2()]
V2_EMPTY = list(sift_scenes.ZERO_RESULT_V2) + ["octaves0"]


def tex64x48_is_exact(ctx):
    case = sift_ref.golden()["tex64x48"]
    assert_same(ctx.extract_sift(case["image"], options_of(case)), sift_ref.assemble(case))


@pytest.mark.parametrize("name", V2_CASES)
def test_matches_vlfeat_v2(ctx, name):
    case = sift_ref.golden_v2()[name]
    want = sift_ref.assemble(case)
    assert (len(want[0]) == 0) == (name in V2_EMPTY)
    assert_same(ctx.extract_sift(case["image"], options_of(case)), want)


@pytest.mark.parametrize("name", V2_EMPTY)
def test_zero_result_and_the_next_call(ctx, name):
    """Octaves under 3 samples are smoothed and skipped, one under 2 ends the loop, num_octaves = 0 never enters it: status 0,
    empty arrays, and nothing left behind that the next call on the context would see."""
    case = sift_ref.golden_v2()[name]
    kp, d = ctx.extract_sift(case["image"], options_of(case))  # a status other than 0 raises
    assert kp.shape == (0, 4) and kp.dtype == np.float32 and d.shape == (0, 128) and d.dtype == np.uint8
    tex64x48_is_exact(ctx)


@pytest.mark.parametrize("name", ["checker40x40", "dots40x40"])
def test_four_orientations(ctx, name):
    case = sift_ref.golden_v2()[name]
    counts = []
    for m in (1, 2, 3, 4):
        got = ctx.extract_sift(case["image"], options_of(case, max_num_orientations=m))
        assert_same(got, sift_ref.assemble(case, max_num_orientations=m))
        counts.append(len(got[0]))
    assert counts[2] < counts[3]  # a keypoint with four orientations: the fourth slot of the angles and of the jobs carries data


def test_l2_normalization_on_ties(ctx):
    from dagsfm_amd import capi
    case = sift_ref.golden_v2()["checker40x40"]
    assert_same(ctx.extract_sift(case["image"], options_of(case, normalization=capi.SIFT_L2, max_num_orientations=4)),
                sift_ref.assemble(case, normalization=sift_ref.L2, max_num_orientations=4))


def test_upright_on_ties(ctx):
    """No upright run of the checkerboard is stored, so the expected result is the restatement's (held to VLFeat on the stored
    checkerboard and on the stored upright run by the CPU tests)."""
    case = sift_ref.golden_v2()["checker40x40"]
    want = sift_ref.extract(case["image"], dict(case["options"], upright=1))
    assert len(want[0]) == len(case["ints"]) and (want[0][:, 3] == 0).all()
    assert_same(ctx.extract_sift(case["image"], options_of(case, upright=1)), want)


def level_counts(case):
    """[(octave, keypoints)] per DoG level of a stored record, in COLMAP's order."""
    levels, prev = [], None
    for o, _, _, s in case["ints"].tolist():
        if (o, s) != prev:
            levels.append([o, 0])
            prev = (o, s)
        levels[-1][1] += 1
    return levels


def test_max_num_features_cuts_first_octave_minus_two(ctx):
    """The cut counts keypoints from the coarsest level down and keeps the crossing level whole: a limit one below the keypoints
    from level i on makes level i the first one kept.  One limit puts the cut inside octave -2 (its first level goes, its last
    stays), the other between octaves -2 and -1.  Both come from the stored per-level counts."""
    case = sift_ref.golden_v2()["first-2_32x24"]
    levels = level_counts(case)
    octs = [o for o, _ in levels]
    after = [sum(n for _, n in levels[i + 1:]) for i in range(len(levels))]  # keypoints of the levels after level i
    assert octs.count(-2) >= 2 and octs[0] == -2 and octs[octs.count(-2)] == -1
    full = sift_ref.assemble(case)
    last_of_m2, first_of_m1 = octs.count(-2) - 1, octs.count(-2)
    for first_kept in (last_of_m2, first_of_m1):
        limit = after[first_kept - 1] - 1  # level first_kept crosses it; the level before it is not reached
        assert limit >= 1 and after[first_kept] <= limit
        assert sift_ref.level_cut([n for _, n in levels], limit) == first_kept
        want = sift_ref.assemble(case, max_num_features=limit)
        assert 0 < len(want[0]) < len(full[0])
        assert_same(ctx.extract_sift(case["image"], options_of(case, max_num_features=limit)), want)


def test_octave_changes_on_one_context(ctx):
    """Up- and downsampled first octaves, the float image kept in the DoG buffer, ties and an empty result, one after another:
    scratch of an earlier call must not show in a later one."""
    g1, g2 = sift_ref.golden(), sift_ref.golden_v2()
    for g, name in ((g2, "first-2_32x24"), (g1, "tex64x48"), (g2, "first2_253x191"), (g2, "checker40x40"), (g2, "line40x1"),
                    (g2, "first-2_32x24"), (g2, "first-3_sq16"), (g2, "rows40x2"), (g2, "first-2_sq20")):
        assert_same(ctx.extract_sift(g[name]["image"], options_of(g[name])), sift_ref.assemble(g[name]))


def test_stage_times_after_a_zero_result(ctx):
    """No octave of the 40 x 1 and 1 x 40 images is searched (80 x 2 is smoothed and skipped, 40 x 1 ends the loop), so `detect`
    is 0; 40 x 2 and 20 x 5 search their first octaves and find nothing.  A skipped octave's smoothing is not in the times."""
    tex64x48_is_exact(ctx)  # non-zero times to be cleared
    assert ctx.sift_time()["detect"] > 0
    for name in sift_scenes.ZERO_RESULT_V2:
        case = sift_ref.golden_v2()[name]
        ctx.extract_sift(case["image"], options_of(case))
        t = ctx.sift_time()
        assert sorted(t) == sorted(ctx.SIFT_STAGES) and all(np.isfinite(v) and v >= 0 for v in t.values()), (name, t)
        assert t["refine"] == 0 and t["orientations"] == 0 and t["descriptors"] == 0, (name, t)
        if name in ("line40x1", "line1x40"):
            assert t["detect"] == 0 and t["base"] == 0 and t["smoothing"] == 0, (name, t)


def test_row_stride_and_no_descriptors_at_first_octave_minus_two(ctx):
    case = sift_ref.golden_v2()["first-2_32x24"]
    h, w = case["image"].shape
    padded = np.full((h, w + 7), 77, np.uint8)
    padded[:, :w] = case["image"]
    want = sift_ref.assemble(case)
    assert_same(ctx.extract_sift(padded, options_of(case), width=w), want)
    kp, d = ctx.extract_sift(padded, options_of(case), width=w, descriptors=False)
    assert d is None
    assert_same((kp, None), (want[0], None))


def test_range_errors_leave_the_context_usable(ctx):
    from dagsfm_amd import capi
    im = sift_ref.golden()["tiny16x16"]["image"]
    column = np.full((40000, 1), 93, np.uint8)  # 1 x 40000: 80000 rows at first_octave = -1
    for image, bad in ((im, dict(first_octave=-5)), (im, dict(first_octave=17)), (im, dict(octave_resolution=65)),
                       (im, dict(num_octaves=65)), (column, dict(first_octave=-1))):
        with pytest.raises(capi.DsmError) as e:
            ctx.extract_sift(image, capi.default_sift_options(**bad))
        assert e.value.status == 4 and e.value.num_features == 0, bad
        tex64x48_is_exact(ctx)
    n = ctypes.c_uint32(5)
    kp = np.zeros((8, 4), np.float32)
    rows = np.ascontiguousarray(im)
    assert capi.lib(ctx.check).dsm_extract_sift(ctx._h, None, rows.ctypes.data, 16, 16, 15, 8, kp.ctypes.data, None, ctypes.byref(n)) == 1
    assert n.value == 0
    tex64x48_is_exact(ctx)


EXTRA_V2 = {  # further shapes at the new octaves, against the restatement
    "33x25_first-2": (lambda sc: sc.texture(33, 25, 17), dict(first_octave=-2)),  # odd and non-square: the scrambled second doubling
    "131x97_first2": (lambda sc: sc.coarse(131, 97, 3, 4), dict(first_octave=2)),  # 131 = 4 * 32 + 3, 97 = 4 * 24 + 1: d = 4 drops a remainder
    "21x21_res1_first-2": (lambda sc: sc.texture(21, 21, 16), dict(octave_resolution=1, peak_threshold=0.02, first_octave=-2)),
}
_extra_v2 = {}


def extra_v2(name):
    """(image, options, expected) of an EXTRA_V2 shape: the restatement runs once."""
    if name not in _extra_v2:
        make, opts = EXTRA_V2[name]
        image = make(sift_scenes)
        full = dict(sift_scenes.DEFAULTS, **opts)
        _extra_v2[name] = (image, full, sift_ref.extract(image, full))
    return _extra_v2[name]


@pytest.mark.parametrize("name", sorted(EXTRA_V2))
def test_matches_restatement_at_other_octaves(ctx, name):
    from dagsfm_amd import capi
    image, full, want = extra_v2(name)
    assert len(want[0]) >= 3
    assert_same(ctx.extract_sift(image, capi.default_sift_options(**full)), want)
