"""dsm_select_source_images on the CPU: the restatement tests/source_selection_ref.py against the reference's
own known answers, the host build of csrc/source_selection.h and csrc/exact_acos.h (libdsm_source_selection_host.so) against
the restatement bit for bit, dsm_acos against mpmath and the host libm, the small exact pieces at their edges, and the
patch-match.cfg side of the binding over the host build."""
import ctypes
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import source_selection_fixtures as fx
from tests import source_selection_ref as ref

f32 = np.float32


def _host(case_name, serial=False):
    _, model_name, kw = fx.case(case_name)
    m = fx.model(model_name)
    return capi.selection_host(m["R"], m["T"], m["xyz"], m["tracks"], serial=serial, **dict(kw))


# ---- known answers from the reference ----

def test_triangulation_angle_known_answers():
    """src/base/triangulation_test.cc:80-92.  BOOST_CHECK_CLOSE's 1e-8 there is a percentage, 1e-10 relative, which is inside
    the 1e-8 relative this project asks for; the tighter one is held."""
    c1, c2 = [0.0, 0.0, 0.0], [0.0, 1.0, 0.0]
    for X, want in (([0.0, 0.0, 100.0], 0.009999666687), ([0.0, 0.0, 50.0], 0.019997333973)):
        q = ref.item_quotient(c1, c2, X)
        a = abs(math.acos(q))
        got = min(a, math.pi - a)
        assert abs(got - want) <= 1e-10 * want
        assert abs(float(ref.triangulation_angle(c1, c2, X)) - want) <= 1e-7 * want  # the float narrowing of the same value
        a1, a2, ax = np.array(c1, f32), np.array(c2, f32), np.array(X, f32)
        bits = capi.selection_host_lib().dsm_ss_host_angle_bits(a1.ctypes.data, a2.ctypes.data, ax.ctypes.data)
        assert bits == int(np.array([ref.triangulation_angle(c1, c2, X)], f32).view(np.uint32)[0])


def test_percentile_known_answers():
    """The Percentile<int> cases of src/util/math_test.cc:97-111 (all fourteen of them)."""
    L = capi.selection_host_lib()
    cases = [([0], 0, 0), ([0], 50, 0), ([0], 100, 0), ([0, 1], 0, 0), ([0, 1], 50, 1), ([0, 1], 100, 1), ([0, 1, 2], 0, 0),
             ([0, 1, 2], 50, 1), ([0, 1, 2], 100, 2), ([0, 1, 1, 2], 0, 0), ([0, 1, 1, 2], 33, 1), ([0, 1, 1, 2], 50, 1), ([0, 1, 1, 2], 66, 1), ([0, 1, 1, 2], 100, 2)]
    assert len(cases) == 14
    for elems, p, want in cases:
        assert ref.percentile(elems, p) == want, (elems, p)
        assert sorted(elems)[L.dsm_ss_host_percentile_index(p, len(elems))] == want, (elems, p)


def test_percentile_index_of_75_is_the_closed_form():
    L = capi.selection_host_lib()
    for n in list(range(1, 300)) + [2 ** 24 + 1, 2 ** 31, 2 ** 32 - 1]:
        assert ref.percentile_index(75.0, n) == (3 * (n - 1) + 2) // 4 == L.dsm_ss_host_percentile_index(75.0, n), n
    for p in (0.0, 33.0, 50.0, 100.0, 12.5, 99.9):
        for n in range(1, 130):
            assert ref.percentile_index(p, n) == L.dsm_ss_host_percentile_index(p, n), (p, n)


# ---- dsm_acos ----

def _acos_args():
    rng = np.random.default_rng(2810)
    tiny = 2.0 ** -30
    return np.concatenate([rng.uniform(-1.0, 1.0, 6000), 1.0 - rng.uniform(0, tiny, 1500), -1.0 + rng.uniform(0, tiny, 1500),
                           rng.uniform(-tiny, tiny, 1500), 1.0 - 2.0 ** -rng.uniform(30, 53, 500), [1.0, -1.0, 0.0, -0.0, 0.5, -0.5,
                                                                                                   np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0)]])


def _dsm_acos(xs):
    f = capi.selection_host_lib().dsm_ss_host_acos
    return np.array([f(float(x)) for x in xs])


def test_acos_is_correctly_rounded():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.prec = 300
    xs = _acos_args()
    got = _dsm_acos(xs)
    want = np.array([float(mpmath.acos(mpmath.mpf(float(x)))) for x in xs])
    bad = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    assert len(bad) == 0, [(float(xs[k]).hex(), float(got[k]).hex(), float(want[k]).hex()) for k in bad[:5]]


def test_acos_against_the_host_libm():
    xs = _acos_args()
    got = _dsm_acos(xs)
    libm = np.array([math.acos(float(x)) for x in xs])
    ulp = np.abs(got.view(np.int64) - libm.view(np.int64))  # both are >= +0: the bit patterns are ordered
    assert ulp.max() <= 1
    assert (ulp == 0).mean() > 0.99


def test_acos_outside_its_domain_is_nan():
    for q in (np.nextafter(1.0, 2.0), np.nextafter(-1.0, -2.0), 1.5, -7.0, float("inf"), float("-inf"), float("nan")):
        assert math.isnan(capi.selection_host_lib().dsm_ss_host_acos(float(q))), q


# ---- the two acos contracts on the fixtures ----

@pytest.mark.parametrize("model_name", sorted(fx.MODELS))
def test_acos_contracts_coincide_on_every_item(model_name):
    """The restatement's math.acos and the device's dsm_acos give the same float angle on every item of every fixture.  An item
    that ever differs is a double-rounding case of the host's acos, to be adjudicated with mpmath -- not a reason to loosen this."""
    m = fx.model(model_name)
    f = capi.selection_host_lib().dsm_ss_host_acos
    n = 0
    for p, i, j, i1, i2, q in ref.items(m["R"], m["T"], m["xyz"], m["tracks"]):
        a = np.array([ref.angle_of_quotient(q)], f32).view(np.uint32)[0]
        b = np.array([ref.angle_of_quotient(q, acos=f)], f32).view(np.uint32)[0]
        both_nan = (a & 0x7fffffff) > 0x7f800000 and (b & 0x7fffffff) > 0x7f800000
        assert a == b or both_nan, "point %d, track elements %d and %d (images %d, %d): q = %s" % (p, i, j, i1, i2, float(q).hex())
        n += 1
    assert n > 0


# ---- the host build against the restatement ----

@pytest.mark.parametrize("case_name", fx.case_names())
@pytest.mark.parametrize("serial", [False, True], ids=["sorted", "serial"])
def test_host_build_equals_the_restatement(case_name, serial):
    want = fx.reference(case_name)
    got = _host(case_name, serial)
    assert fx.same(got, want) is None, fx.same(got, want)
    assert got["stats"] == {"items": want["items"], "pairs": want["n_pairs"], "nan_items": want["nan_items"]}


def test_only_the_collinear_model_has_nan_items():
    for name, model_name, _ in fx.cases():
        nan = fx.reference(name)["nan_items"]
        assert (nan > 0) == (model_name in fx.NAN_MODELS), name
    want = fx.reference("collinear_p100")
    a, b, count, angle = want["pairs"]
    assert [(int(x), int(y)) for x, y in zip(a, b)] == [(0, 1), (0, 2), (1, 2), (1, 3)]
    assert np.isnan(angle[0]) and np.isnan(angle[3]) and not np.isnan(angle[1])  # NaN orders last: it is the 100th percentile
    assert want["sources"][3] == [] and 1 not in want["sources"][0]            # and fails >= even at 0 degrees
    assert not np.isnan(fx.reference("collinear")["pairs"][3][0])               # the 75th percentile of (0, 1) is a number


def test_gate_thresholds_sit_either_side_of_the_pair():
    deg_equal, deg_above = fx.gate_thresholds()
    base, eq, above = fx.reference("gate"), fx.reference("gate_equal"), fx.reference("gate_above")
    k = [i for i in range(len(base["pairs"][0])) if (base["pairs"][0][i], base["pairs"][1][i]) == (0, 4)][0]
    angle = base["pairs"][3][k]
    assert ref.min_angle_rad(deg_equal) == angle and ref.min_angle_rad(deg_above) == np.nextafter(angle, f32(np.inf))
    assert 4 in eq["sources"][0] and 0 in eq["sources"][4]          # equality passes
    assert 4 not in above["sources"][0] and 0 not in above["sources"][4]  # the next float up fails
    assert base["sources"][0] == [4, 1, 2, 3]                       # equal counts: ascending index
    assert fx.reference("gate_mask")["sources"][0] == [1, 2, 3]
    assert fx.reference("gate_max1")["sources"][0] == [4] and fx.reference("gate_max0")["sources"] == [[]] * 6


# ---- the small pieces ----

def _decode(t):
    i, j = ctypes.c_uint64(0), ctypes.c_uint64(0)
    capi.selection_host_lib().dsm_ss_host_decode_item(t, ctypes.byref(i), ctypes.byref(j))
    return int(i.value), int(j.value)


def test_item_decode_round_trip():
    L = capi.selection_host_lib()
    t = 0
    for i in range(1, 363):  # L = 363: 65 703 items, past 2^16
        for j in range(i):
            assert _decode(t) == (i, j) and L.dsm_ss_host_encode_item(i, j) == t
            t += 1
    assert t == 363 * 362 // 2 == 65703


def test_item_decode_at_large_indices():
    L = capi.selection_host_lib()
    last = 2 ** 32 - 1  # the longest track has 2^32 - 1 elements: its last item is the largest triangular index, below 2^63
    top = last * (last - 1) // 2 + last - 1
    assert top < 2 ** 63
    for centre in (2 ** 32, 2 ** 40, 2 ** 53, 2 ** 62):
        i0 = (1 + math.isqrt(1 + 8 * centre)) // 2
        for i in (i0 - 1, i0, i0 + 1):
            for j in (0, 1, i - 1):
                t = i * (i - 1) // 2 + j
                assert _decode(t) == (i, j) and L.dsm_ss_host_encode_item(i, j) == t, (i, j)
    for t in (2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 40 - 1, 2 ** 40, 2 ** 40 + 1, top - 1, top):
        i, j = _decode(t)
        assert j < i and i * (i - 1) // 2 + j == t, t
    assert _decode(top) == (last, last - 1)


def test_depth_index_is_the_float_product():
    L = capi.selection_host_lib()
    differs = 0
    for size in (1, 2, 99, 100, 101, 200, 300, 16777217):
        for factor in (0.01, 0.99):
            want = int(f32(size) * f32(factor))
            assert ref.depth_index(size, factor) == want == L.dsm_ss_host_depth_index(size, factor), (size, factor)
            assert want < size
            differs += want != int(size * float(f32(factor)))  # the same factor, the product in double
    assert ref.depth_index(100, 0.01) == 1 and int(100 * float(f32(0.01))) == 0  # the float product rounds up to 1.0
    assert differs >= 1


def test_min_angle_rad():
    L = capi.selection_host_lib()
    for deg in (0.0, 1.0, 0.5, 3.0, 90.0, 71.96153437817702):
        assert L.dsm_ss_host_min_angle_rad(deg) == float(ref.min_angle_rad(deg))
    assert float(ref.min_angle_rad(1.0)) == float(f32(math.pi / 180))


# ---- consistency with capi.overlapping_images ----

@pytest.mark.parametrize("model_name", sorted(set(fx.MODELS) - set(fx.NAN_MODELS)))
def test_angle_zero_equals_overlapping_images(model_name):
    m = fx.model(model_name)
    for num in (3, 20):
        got = capi.selection_host(m["R"], m["T"], m["xyz"], m["tracks"], min_triangulation_angle=0.0, max_num_src_images=num)
        assert got["stats"]["nan_items"] == 0
        assert got["sources"] == capi.overlapping_images(m["tracks"], len(m["R"]), num)


# ---- errors ----

def test_host_build_refuses_bad_arguments():
    m = fx.model("gate")
    for kw in ({"max_num_src_images": -1}, {"triangulation_angle_percentile": 101.0}, {"triangulation_angle_percentile": float("nan")},
               {"min_triangulation_angle": float("nan")}):
        with pytest.raises(capi.DsmError):
            capi.selection_host(m["R"], m["T"], m["xyz"], m["tracks"], **kw)
    with pytest.raises(capi.DsmError, match="out of range"):
        capi.selection_host(m["R"], m["T"], m["xyz"], [[0, 6]] + m["tracks"][1:])
    empty = capi.selection_host(np.zeros((0, 9)), np.zeros((0, 3)), np.zeros((0, 3)), [])
    assert empty["sources"] == [] and empty["stats"]["items"] == 0


# ---- patch-match.cfg ----

NAMES = ["img%d.jpg" % i for i in range(6)]


def test_parse_patch_match_config():
    lines = ["# a comment", "", "  img0.jpg  ", "__auto__, 2", "img4.jpg", "   ", "# another", "__all__", "img2.jpg", "img0.jpg, img3.jpg,img4.jpg",
             "img5.jpg"]  # the last reference image has no specification: dropped
    assert capi.parse_patch_match_config(lines, NAMES) == [(0, ("auto", 2)), (4, ("all",)), (2, ("list", [0, 3, 4]))]
    with pytest.raises(capi.DsmError):
        capi.parse_patch_match_config(["nope.jpg", "__all__"], NAMES)
    with pytest.raises(capi.DsmError):
        capi.parse_patch_match_config(["img0.jpg", "img1.jpg, nope.jpg"], NAMES)
    # the file both writers of the reference emit
    both = capi.parse_patch_match_config([l for n in NAMES for l in (n, "__auto__, 20")], NAMES)
    assert both == [(i, ("auto", 20)) for i in range(6)]


def _problems(config, options=None):
    m = dict(fx.model("gate"), image_names=NAMES)
    return capi.Context.patch_match_problems(None, m, config, options, select=capi.selection_host)


def test_patch_match_problems_auto():
    want = fx.reference("gate")
    got = _problems([l for n in NAMES for l in (n, "__auto__, 20")])
    assert [p[0] for p in got] == [a for a in range(6) if want["sources"][a]]
    for ref_image, src, lo, hi in got:
        assert src == want["sources"][ref_image]
        assert (f32(lo), f32(hi)) == tuple(want["depth_ranges"][ref_image])
    # only the configured reference images may be sources (ReadProblems' ref_image_idxs.count), and N cuts the list
    got = _problems(["img0.jpg", "__auto__, 2", "img1.jpg", "__auto__, 2", "img2.jpg", "__auto__, 1", "img3.jpg", "__auto__, 0"])
    assert [(p[0], p[1]) for p in got] == [(0, [1, 2]), (1, [0]), (2, [0])]  # image 3: N = 0 leaves no source, dropped


def test_patch_match_problems_all_lists_and_depths():
    want = fx.reference("gate")
    got = _problems(["img4.jpg", "__all__", "img0.jpg", "img5.jpg, img1.jpg", "img2.jpg", "__all__"], {"depth_min": 0.5})
    assert [(p[0], p[1]) for p in got] == [(4, [0, 2]), (0, [5, 1]), (2, [0, 4])]  # __all__: the other reference images, ascending
    for ref_image, _, lo, hi in got:
        assert lo == 0.5 and f32(hi) == want["depth_ranges"][ref_image][1]
    got = _problems(["img0.jpg", "__all__"])  # the only reference image has nobody else: dropped
    assert got == []
    got = _problems(["img0.jpg", "img1.jpg"], {"depth_min": 1.0, "depth_max": 9.0})
    assert got == [(0, [1], 1.0, 9.0)]
    # a gate nobody passes: every __auto__ image is dropped
    assert _problems([l for n in NAMES for l in (n, "__auto__, 20")], {"min_triangulation_angle": 179.0}) == []
