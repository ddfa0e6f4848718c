"""CPU-only checks of the second SIFT golden file (tests/golden/sift_vlfeat_v2.npz, sift_scenes.cases_v2()): the
octaves, sizes and options the first file leaves out.  The file matches its recipe, the numpy restatement (tests/sift_ref.py)
reproduces every record of it bit for bit -- which is what lets the GPU tests use the restatement on shapes that are not stored --
and every case is shown to reach the path it was stored for."""
import os

import numpy as np
import pytest

from tests import sift_ref, sift_scenes

FIELDS = ("ints", "floats", "num_angles", "angles", "descriptors")


def octave_counts(case):
    """{octave: keypoints} of a stored record."""
    octs, n = np.unique(case["ints"][:, 0], return_counts=True)
    return dict(zip(octs.tolist(), n.tolist()))


def test_v2_file_matches_the_scenes():
    g = sift_ref.golden_v2()
    cases = sift_scenes.cases_v2()
    assert sorted(g) == sorted(name for name, _, _ in cases) and len(g) == len(cases)
    assert not set(g) & set(sift_ref.golden())
    for name, image, options in cases:
        assert g[name]["image"].dtype == np.uint8 and g[name]["image"].shape == image.shape and (g[name]["image"] == image).all(), name
        assert g[name]["options"] == options, name
        n = len(g[name]["ints"])
        assert g[name]["ints"].shape == (n, 4) and g[name]["floats"].shape == (n, 4) and g[name]["angles"].shape == (n, 4), name
        assert g[name]["num_angles"].shape == (n,), name
        assert g[name]["descriptors"].shape == (int(g[name]["num_angles"].sum()), 128), name
        assert max(image.shape) <= 256 and min(image.shape) <= 192
    assert os.path.getsize(sift_ref.GOLDEN_V2) < 1000000


@pytest.mark.parametrize("name", [n for n, _, _ in sift_scenes.cases_v2()])
def test_restatement_reproduces_vlfeat_bit_for_bit_v2(name):
    case = sift_ref.golden_v2()[name]
    got = sift_ref.vlfeat(case["image"], **case["options"])
    for field in FIELDS:
        a, b = got[field], case[field]
        assert a.dtype == b.dtype and a.shape == b.shape, (field, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), field


def test_negative_first_octaves_hold_keypoints():
    g = sift_ref.golden_v2()
    sq, ns, m3 = g["first-2_sq20"], g["first-2_32x24"], g["first-3_sq16"]
    assert sq["image"].shape[0] == sq["image"].shape[1] and ns["image"].shape[0] != ns["image"].shape[1]
    for case in (sq, ns):
        assert case["options"]["first_octave"] == -2 and len(case["ints"]) >= 10
        assert octave_counts(case).get(-2, 0) >= 1
    # the non-square image: octave -2 is the scrambled double upsampling itself, octave -1 is sampled from it
    assert len(octave_counts(ns)) >= 2 and min(octave_counts(ns).values()) >= 2
    assert m3["options"]["first_octave"] == -3 and 12 <= m3["image"].shape[0] <= 16 and len(m3["ints"]) >= 5
    assert octave_counts(m3).get(-3, 0) >= 1


def test_positive_first_octaves_hold_keypoints():
    g = sift_ref.golden_v2()
    f2, f3 = g["first2_253x191"], g["first3_253x191"]
    assert f2["options"]["first_octave"] == 2 and len(f2["ints"]) >= 10 and octave_counts(f2).get(2, 0) >= 1
    assert f3["options"]["first_octave"] == 3 and len(f3["ints"]) >= 3 and octave_counts(f3).get(3, 0) >= 1
    h, w = f2["image"].shape
    assert w % 4 and h % 4 and w % 8 and h % 8  # the sampling drops a remainder in both directions
    assert (f2["image"][:, 1:] != f2["image"][:, :-1]).mean() > 0.5  # neighbours differ: a sampling offset changes the samples


def test_num_octaves_cases():
    g, g1 = sift_ref.golden_v2(), sift_ref.golden()
    auto, none, one, many = g["octaves-1"], g["octaves0"], g["octaves1"], g["octaves10_16x16"]
    assert (auto["options"]["num_octaves"], none["options"]["num_octaves"], one["options"]["num_octaves"]) == (-1, 0, 1)
    assert (auto["image"] == g1["tex64x48"]["image"]).all()
    assert len(auto["ints"]) > 0
    for field in FIELDS:  # the automatic count gives the three octaves that hold keypoints at num_octaves = 4
        assert auto[field].dtype == g1["tex64x48"][field].dtype and auto[field].tobytes() == g1["tex64x48"][field].tobytes(), field
    assert len(none["ints"]) == 0 and len(none["descriptors"]) == 0
    assert sorted(octave_counts(one)) == [-1] and 0 < len(one["ints"]) < len(auto["ints"])
    n1 = len(one["ints"])
    for field in ("ints", "floats", "num_angles", "angles"):  # one octave is the first octave of the full run
        assert one[field].tobytes() == auto[field][:n1].tobytes(), field
    assert many["options"]["num_octaves"] == 10 and many["image"].shape == (16, 16) and len(many["ints"]) >= 1
    for field in FIELDS:  # octaves past the image's end add nothing
        assert many[field].tobytes() == g1["tiny16x16"][field].tobytes(), field


def test_small_octave_cases():
    g = sift_ref.golden_v2()
    assert sorted(g[n]["image"].shape for n in sift_scenes.ZERO_RESULT_V2) == [(1, 40), (2, 40), (5, 20), (40, 1)]
    for name in sift_scenes.ZERO_RESULT_V2:
        assert len(g[name]["ints"]) == 0 and g[name]["descriptors"].shape == (0, 128), name
        assert g[name]["image"].min() < g[name]["image"].max(), name  # not constant: the result is empty because of the size
    thin = g["thin44x10"]
    h, w = thin["image"].shape
    o_min, O = thin["options"]["first_octave"], thin["options"]["num_octaves"]
    sizes = [(sift_ref._shift(w, -oc), sift_ref._shift(h, -oc)) for oc in range(o_min, o_min + O)]
    skipped = [s for s in sizes if min(s) == 2]
    assert skipped and sizes.index(skipped[0]) > 0            # an octave under 3 rows inside the run: smoothed, not searched
    assert any(min(s) < 2 for s in sizes[sizes.index(skipped[-1]) + 1:])  # and one under 2 after it: the end of the loop
    first_small = min(i for i, s in enumerate(sizes) if min(s) < 3)
    early = sum(n for oc, n in octave_counts(thin).items() if oc - o_min < first_small)
    assert early >= 5 and early == len(thin["ints"])


def test_checkerboard_has_four_orientations():
    case = sift_ref.golden_v2()["checker40x40"]
    assert case["image"].shape == (40, 40)
    assert int((case["num_angles"] == 4).sum()) >= 1 and int(case["num_angles"].max()) == 4
    assert (case["angles"][case["num_angles"] == 4] != 0).all()  # the fourth slot carries data
    counts = [len(sift_ref.assemble(case, max_num_orientations=m)[0]) for m in (1, 2, 3, 4)]
    assert counts[0] < counts[1] < counts[2] < counts[3]


def dog_ties(case):
    """(tied, deciding): interior DoG samples above the 0.8 peak_threshold gate that equal one of their 26 neighbours, and those
    of them that are >= (or <=) all 26 -- no candidate under the source's strict test, one under a >= slip."""
    trace = []
    sift_ref.vlfeat(case["image"], trace=trace, **case["options"])
    gate = 0.8 * case["options"]["peak_threshold"]
    tied = deciding = 0
    for t in trace:
        D = t["dog"]
        h, w = D.shape[1:]
        for s in range(case["options"]["octave_resolution"]):
            v = D[s + 1, 1:-1, 1:-1]
            above = np.abs(v).astype(np.float64) >= gate
            eq = np.zeros(v.shape, bool)
            ge, le = np.ones(v.shape, bool), np.ones(v.shape, bool)
            for ds in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if ds or dy or dx:
                            u = D[s + 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                            eq |= v == u  # equal values: the neighbour exceeds the gate as well
                            ge &= v >= u
                            le &= v <= u
            tied += int((above & eq).sum())
            deciding += int((above & eq & (((v > 0) & ge) | ((v < 0) & le)) & ~t["flags"][s, 1:-1, 1:-1]).sum())
    return tied, deciding


def test_dog_ties():
    """The checkerboard's DoG holds equal neighbouring samples above the gate; on the dots some of them are extrema but for
    the tie, so >= in place of > in the 26-neighbour test would add candidates."""
    g = sift_ref.golden_v2()
    assert dog_ties(g["checker40x40"])[0] >= 1
    tied, deciding = dog_ties(g["dots40x40"])
    assert tied >= 1 and deciding >= 1
    assert len(g["dots40x40"]["ints"]) >= 10


def fullest_chunk(case):
    """The most set flags in one 256-flag chunk of an octave's candidates, in the (s, y, x) order the device compacts them in."""
    trace = []
    sift_ref.vlfeat(case["image"], trace=trace, **case["options"])
    fullest = 0
    for t in trace:
        f = t["flags"].ravel()
        f = np.concatenate([f, np.zeros(-len(f) % 256, bool)]).reshape(-1, 256)
        fullest = max(fullest, int(f.sum(axis=1).max()))
    return fullest


def test_dense_case_fills_a_compaction_chunk():
    """The binary noise and the low thresholds give no more than 2 and 5 candidates to a chunk (VLFeat's first smoothing leaves
    extrema several samples apart), so a narrow fine checkerboard is the dense case: 8 or more in one chunk."""
    g = sift_ref.golden_v2()
    assert fullest_chunk(g["dense18x48"]) >= 8
    assert len(g["dense18x48"]["ints"]) >= 100
    assert 1 <= fullest_chunk(g["noise64x48"]) and 1 <= fullest_chunk(g["lowthreshold"])
    assert len(g["lowthreshold"]["ints"]) > len(sift_ref.golden()["tex64x48"]["ints"])
    assert len(g["noise64x48"]["ints"]) >= 10
