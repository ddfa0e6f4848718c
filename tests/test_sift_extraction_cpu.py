"""CPU-only checks of SIFT extraction: the golden file of VLFeat's results, the host half that follows VLFeat in
ExtractSiftFeaturesCPU (tests/sift_ref.py), the declared symbols and the option defaults."""
import ctypes
import os
import re

import numpy as np

from tests import sift_ref, sift_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_golden_file_matches_the_scenes():
    """Every case of sift_scenes.cases() is stored with the image the recipe gives today and the options it names."""
    g = sift_ref.golden()
    cases = sift_scenes.cases()
    assert sorted(g) == sorted(name for name, _, _ in cases)
    for name, image, options in cases:
        assert g[name]["image"].dtype == np.uint8 and (g[name]["image"] == image).all(), name
        assert g[name]["options"] == options, name
        n = len(g[name]["ints"])
        assert g[name]["floats"].shape == (n, 4) and g[name]["angles"].shape == (n, 4) and g[name]["num_angles"].shape == (n,)
        assert g[name]["descriptors"].shape == (int(g[name]["num_angles"].sum()), 128)
    assert os.path.getsize(sift_ref.GOLDEN) < 1000000


import pytest


@pytest.mark.parametrize("name", [n for n, _, _ in sift_scenes.cases()])
def test_restatement_reproduces_vlfeat_bit_for_bit(name):
    """tests/sift_ref.py's numpy restatement of the VLFeat stage against VLFeat's own bytes: keypoint records, angles and float
    descriptors, for every image and option set in the golden file.  This is what pins the restatement to the reference."""
    case = sift_ref.golden()[name]
    got = sift_ref.vlfeat(case["image"], **case["options"])
    for field in ("ints", "floats", "num_angles", "angles", "descriptors"):
        a, b = got[field], case[field]
        assert a.dtype == b.dtype and a.shape == b.shape, (field, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), field


def test_golden_texture_is_rich_enough():
    """VLFeat finds keypoints in at least three octaves, on at least four DoG levels, at least 100 on the largest image."""
    big = sift_ref.golden()["tex96x80"]
    assert big["image"].shape == (80, 96)
    assert len(big["ints"]) >= 100
    assert len(set(big["ints"][:, 0].tolist())) >= 3
    assert len(set(map(tuple, big["ints"][:, [0, 3]].tolist()))) >= 4
    assert len(sift_ref.golden()["constant40x30"]["ints"]) == 0
    assert len(sift_ref.golden()["single"]["ints"]) == 1
    assert (sift_ref.golden()["upright"]["num_angles"] == 1).all() and (sift_ref.golden()["upright"]["angles"] == 0).all()


def test_ubc_permutation_on_hand_made_rows():
    """sift.cc:58-74: bin k of each of the 16 cells goes to (0, 7, 6, 5, 4, 3, 2, 1)[k]."""
    idx = sift_ref.ubc_permutation()
    assert sorted(idx.tolist()) == list(range(128))
    assert idx[:8].tolist() == [0, 7, 6, 5, 4, 3, 2, 1] and idx[120:].tolist() == [120, 127, 126, 125, 124, 123, 122, 121]
    case = {"ints": np.array([[0, 1, 1, 0]], np.int32), "floats": np.array([[1, 2, 0, 3]], np.float32), "num_angles": np.array([1], np.int32),
            "angles": np.zeros((1, 4)), "descriptors": np.zeros((1, 128), np.float32)}
    case["descriptors"][0, 9] = 1.0  # cell 1, bin 1 -> cell 1, bin 7
    kp, d = sift_ref.assemble(case, normalization=sift_ref.L2)
    assert kp.tolist() == [[1.5, 2.5, 3.0, 0.0]]
    assert d[0, 15] == 255 and d[0].sum() == 255  # round(512 * 1) truncated to 255


def test_unsigned_byte_conversion_on_hand_made_rows():
    """utils.cc:65-77: std::round (half away from zero), then the clamp to 0 .. 255; a NaN becomes 0."""
    v = np.array([[0.0, 0.5 / 512, 0.49999 / 512, 1.5 / 512, 2.5 / 512, 0.4990234375, 0.5, 1.0, -0.25, np.nan]], np.float32)
    assert sift_ref.to_unsigned_byte(v)[0].tolist() == [0, 1, 0, 2, 3, 255, 255, 255, 0, 0]
    # L1_ROOT: v / sum |v|, then the square root
    row = np.zeros((1, 128), np.float32)
    row[0, :4] = [1, 1, 1, 1]
    assert sift_ref.normalize(row, sift_ref.L1_ROOT)[0, :5].tolist() == [0.5, 0.5, 0.5, 0.5, 0.0]
    assert sift_ref.to_unsigned_byte(sift_ref.normalize(row, sift_ref.L1_ROOT))[0, :5].tolist() == [255, 255, 255, 255, 0]
    row[0, :4] = [3, 4, 0, 0]
    assert sift_ref.normalize(row, sift_ref.L2)[0, :3].tolist() == [np.float32(3) / np.float32(5), np.float32(4) / np.float32(5), 0.0]
    zero = np.zeros((1, 128), np.float32)
    assert (sift_ref.to_unsigned_byte(sift_ref.normalize(zero, sift_ref.L1_ROOT)) == 0).all()  # 0 / 0 -> NaN -> 0
    assert (sift_ref.normalize(zero, sift_ref.L2) == 0).all()  # Eigen's normalized() leaves a zero row


def test_max_num_features_keeps_the_crossing_level_whole():
    """sift.cc:387-398 counts keypoints from the coarsest level down and stops at the level that exceeds the limit."""
    assert sift_ref.level_cut([10, 20, 30], 100) == 0
    assert sift_ref.level_cut([10, 20, 30], 60) == 0   # 60 is not above 60
    assert sift_ref.level_cut([10, 20, 30], 59) == 0   # level 0 crosses and stays
    assert sift_ref.level_cut([10, 20, 30], 49) == 1   # 30 + 20 = 50 > 49: level 1 crosses and is kept whole
    assert sift_ref.level_cut([10, 20, 30], 29) == 2
    assert sift_ref.level_cut([10, 20, 30], 1) == 2    # the coarsest level is always kept
    assert sift_ref.level_cut([], 5) == 0
    case = sift_ref.golden()["tex64x48"]
    full, _ = sift_ref.assemble(case, max_num_orientations=1)
    cut, cut_desc = sift_ref.assemble(case, max_num_orientations=1, max_num_features=30)
    assert 30 < len(cut) < len(full)            # the crossing level makes it more than the limit
    assert (cut == full[len(full) - len(cut):]).all() and cut_desc.shape == (len(cut), 128)


def test_assembly_keeps_the_first_orientations():
    case = sift_ref.golden()["tex96x80"]
    assert case["num_angles"].max() >= 2
    for m in (1, 2, 4):
        kp, d = sift_ref.assemble(case, max_num_orientations=m)
        assert len(kp) == int(np.minimum(case["num_angles"], m).sum()) == len(d)
    kp1, _ = sift_ref.assemble(case, max_num_orientations=1)
    first = case["angles"][case["num_angles"] > 0, 0].astype(np.float32)
    assert (kp1[:, 3] == first).all()


def test_sift_symbols_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "dagsfm_mi355x.h")).read()
    for sym in ("dsm_sift_default_options", "dsm_extract_sift"):
        assert re.search(r"\b%s\s*\(" % sym, text), sym
    assert "typedef struct dsm_sift_options" in text
    from dagsfm_amd import capi
    for path in (capi.LIB_PATH, capi.CHECK_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "dsm_extract_sift") and hasattr(lib, "dsm_sift_default_options"), path


def test_default_sift_options_match_reference():
    # /root/reference/src/feature/sift.h: SiftExtractionOptions
    from dagsfm_amd import capi
    o = capi.default_sift_options()
    assert (o.num_octaves, o.octave_resolution, o.first_octave) == (4, 3, -1)
    assert (o.peak_threshold, o.edge_threshold) == (0.02 / 3, 10.0)
    assert (o.max_num_orientations, o.max_num_features, o.upright, o.normalization) == (2, 8192, 0, capi.SIFT_L1_ROOT)
    assert ctypes.sizeof(capi.SiftOptions) == 48
    assert capi.default_sift_options(upright=1).upright == 1


def test_invalid_arguments_without_a_context():
    """The entry never aborts: no context is an error status."""
    from dagsfm_amd import capi
    n = ctypes.c_uint32(7)
    assert capi.lib().dsm_extract_sift(None, None, None, 0, 0, 0, 0, None, None, ctypes.byref(n)) == 1
