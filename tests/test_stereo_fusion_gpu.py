"""dsm_fuse_stereo on the device: points, colours, normals and visibility equal to the restatement
(tests/stereo_fusion_ref.py) on the bits, in the product's schedule (speculate, claim, commit in rank order) and in the check
build's serial lane (DSM_FUSION_SERIAL), on the smallest shapes where it can go wrong: widths off a multiple of 64 and one
above a wave (65 x 9), sides that differ between images, lists that lead back into the current image, both limits firing on
most seeds, holes; then the lane capacities, unused and unlisted images, clusters below min_num_pixels, a bitmap of another
size, the memory budget, every invalid argument, the empty call and the stage times."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import stereo_fusion_cases as cases
from tests import stereo_fusion_ref as ref

pytestmark = pytest.mark.gpu

SCHEDULES = ["product", "serial"]


def _schedule(monkeypatch, schedule):
    if schedule == "serial":
        monkeypatch.setenv("DSM_FUSION_SERIAL", "1")  # the check build's one lane, seed after seed


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("name", cases.TABLE + ("slanted_bitmap_2x", "slanted_pairs"))
def test_case_equals_the_restatement(dsm, monkeypatch, name, schedule):
    _schedule(monkeypatch, schedule)
    images, overlap, options = cases.case(name)
    want = cases.expected(name)
    # the conditions under which the case shows anything
    assert len(want["points"]) >= 100
    if name in cases.DEFAULT_CASES:
        assert max(len(v) for v in want["visibility"]) >= 3
    if name == "step_max_pixels":
        assert want["stats"]["breaks"] >= 1
    if name == "slanted_depth_limit":
        assert want["stats"]["depth_hits"] >= 1
    got = dsm.stereo_fusion(images, overlap, **options)
    assert cases.same_result(got, want)
    times = dsm.stereo_fusion_time()
    assert tuple(times) == capi.STEREO_FUSION_STAGES and times["rounds"] >= len(images)
    if schedule == "serial":
        assert times["traversals"] == want["stats"]["traversals"]
    else:
        assert times["traversals"] >= want["stats"]["traversals"] and times["rounds"] > len(images)
        assert all(times[k] > 0 for k in ("upload", "traversal", "claims_commit", "medians", "download"))


@pytest.mark.parametrize("lane_capacity", [1, 3, 0, 2 ** 31 - 1])
def test_lane_capacity_changes_no_byte(dsm, lane_capacity):
    images, overlap, options = cases.case("slanted")
    got = dsm.stereo_fusion(images, overlap, lane_capacity=lane_capacity, **options)
    assert cases.same_result(got, cases.expected("slanted"))


def test_lane_capacity_below_the_clusters_with_both_limits(dsm):
    for name in ("step_max_pixels", "slanted_depth_limit"):
        images, overlap, options = cases.case(name)
        got = dsm.stereo_fusion(images, overlap, lane_capacity=2, **options)
        assert cases.same_result(got, cases.expected(name)), name


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_unused_and_unlisted_images(dsm, monkeypatch, schedule):
    _schedule(monkeypatch, schedule)
    images, overlap, _ = cases.case("step_noise_holes")
    part = [dict(im) for im in images]
    part[0] = {"used": False}  # image 0 unused: the loop still starts there
    part[3]["used"] = False
    lists = [[1, 2], [0, 2, 3], [3, 1], [0], []]  # image 4 is named in no list and lists nobody
    want = ref.fuse([dict(im, used=False, depth=np.zeros((0, 0), np.float32)) if not im["used"] else im for im in part], lists,
                    {"min_num_pixels": 2})
    assert len(want["points"]) > 0 and {i for v in want["visibility"] for i in v} == {1, 2}
    got = dsm.stereo_fusion(part, lists, min_num_pixels=2)
    assert cases.same_result(got, want)


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_min_num_pixels_above_every_cluster(dsm, monkeypatch, schedule):
    _schedule(monkeypatch, schedule)
    images, overlap, _ = cases.case("slanted")
    points, colours, normals, vis = dsm.stereo_fusion(images, overlap, min_num_pixels=9999)
    assert points.shape == (0, 3) and colours.shape == (0, 3) and normals.shape == (0, 3) and vis == []
    # every mask was consumed: a traversal per cluster and not one more (the restatement's count, masks persisting)
    want = ref.fuse(images, overlap, {"min_num_pixels": 9999})
    assert all((m == (im["depth"] > 0)).all() for m, im in zip(want["masks"], images))
    if schedule == "serial":
        assert dsm.stereo_fusion_time()["traversals"] == want["stats"]["traversals"]


def test_bitmap_smaller_than_its_scale_promises(dsm):
    images, overlap, _ = cases.case("slanted")
    cut = [dict(im) for im in images]
    cut[0]["rgb"] = np.ascontiguousarray(images[0]["rgb"][:12, :20])
    wide = np.zeros((23, 50, 3), dtype=np.uint8)  # a row stride above 3 x width
    wide[:, :37] = images[2]["rgb"]
    cut[2]["rgb"] = wide[:, :37]
    want = ref.fuse(cut, overlap)
    assert want["colours"].tobytes() != cases.expected("slanted")["colours"].tobytes()
    assert cases.same_result(dsm.stereo_fusion(cut, overlap), want)


def test_memory_budget_of_one_byte_is_refused(dsm):
    images, overlap, _ = cases.case("slanted")
    dsm.set_memory_budget(1)
    try:
        with pytest.raises(capi.DsmError) as e:
            dsm.stereo_fusion(images, overlap)
        assert e.value.rc == 4  # DSM_ERR_OUT_OF_RANGE
    finally:
        dsm.set_memory_budget(0)
    assert cases.same_result(dsm.stereo_fusion(images, overlap), cases.expected("slanted"))


def test_invalid_arguments_leave_the_outputs_untouched(dsm):
    images, overlap, _ = cases.case("slanted")
    assert cases.same_result(dsm.stereo_fusion(images, overlap), cases.expected("slanted"))

    def refused(ims, lists, **kw):
        with pytest.raises(capi.DsmError) as e:
            dsm.stereo_fusion(ims, lists, **kw)
        assert e.value.rc == 1, (kw, str(e.value))  # DSM_ERR_INVALID_ARGUMENT

    for bad in ({"min_num_pixels": 0}, {"min_num_pixels": -1}, {"min_num_pixels": 4, "max_num_pixels": 3}, {"max_traversal_depth": 0},
                {"max_reproj_error": -1.0}, {"max_depth_error": -1.0}, {"max_normal_error": -1.0}, {"max_reproj_error": float("nan")},
                {"max_depth_error": float("nan")}, {"max_normal_error": float("nan")}, {"lane_capacity": -1}):
        refused(images, overlap, **bad)
    refused(images, [[0, 1]] + overlap[1:])        # its own image
    refused(images, [[4]] + overlap[1:])           # out of range
    for key, value in (("depth", np.zeros((0, 37), np.float32)), ("row_stride", 3 * 37 - 1)):
        broken = [dict(im) for im in images]
        broken[1][key] = value
        if key == "depth":
            broken[1]["normal"] = np.zeros((3, 0, 37), np.float32)
        refused(broken, overlap)
    big = [dict(im) for im in images]
    big[1]["depth"] = np.ones((1, 32769), np.float32)
    big[1]["normal"] = np.zeros((3, 1, 32769), np.float32)
    refused(big, overlap)
    for value in (np.nan, np.inf):
        broken = [dict(im) for im in images]
        broken[2]["depth"] = images[2]["depth"].copy()
        broken[2]["depth"][3, 5] = value
        refused(broken, overlap)
        broken = [dict(im) for im in images]
        broken[2]["normal"] = images[2]["normal"].copy()
        broken[2]["normal"][1, 3, 5] = value
        refused(broken, overlap)
    # NULL where data is needed, at the C-ABI itself
    arr, offs, idx, keep = capi._fusion_call_arguments(images, overlap)
    n = capi.ctypes.c_uint64(77)
    L, h = dsm._L, dsm._h
    assert L.dsm_fuse_stereo(h, None, len(images), None, offs.ctypes.data, idx.ctypes.data, capi.ctypes.byref(n)) == 1
    assert L.dsm_fuse_stereo(h, None, len(images), capi.ctypes.addressof(arr), None, idx.ctypes.data, capi.ctypes.byref(n)) == 1
    assert L.dsm_fuse_stereo(h, None, len(images), capi.ctypes.addressof(arr), offs.ctypes.data, None, capi.ctypes.byref(n)) == 1
    assert L.dsm_fuse_stereo(h, None, len(images), capi.ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, None) == 1
    arr[1].depth_map = None
    assert L.dsm_fuse_stereo(h, None, len(images), capi.ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, capi.ctypes.byref(n)) == 1
    assert n.value == 77
    # the last good call's points are still the context's
    want = cases.expected("slanted")
    rec = np.zeros(len(want["points"]), dtype=capi.FUSED_POINT_DTYPE)
    assert L.dsm_get_fused_points(h, rec.ctypes.data, len(rec), None, None, 0) == 0
    assert rec["xyz"].tobytes() == want["points"][:, :3].tobytes()
    assert L.dsm_get_fused_points(h, rec.ctypes.data, len(rec) - 1, None, None, 0) == 4  # a capacity below the points


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_empty_calls(dsm, monkeypatch, schedule):
    _schedule(monkeypatch, schedule)
    for images, lists in (([], []), ([{"used": False}], [[]]), ([{"used": False}, {"used": False}], [[1], [0]])):
        points, colours, normals, vis = dsm.stereo_fusion(images, lists)
        assert points.shape == (0, 3) and vis == []
        assert dsm.stereo_fusion_time()["rounds"] == 0
