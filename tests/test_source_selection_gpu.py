"""dsm_select_source_images on the device against tests/source_selection_ref.py, bit for bit, in the product's
schedule and in the check build's one lane (DSM_SOURCE_SELECTION_SERIAL), on the fixture models of
tests/source_selection_fixtures.py: track lengths around the wave and past 2^16 items, every residue of the percentile index,
images without depths and at the depth indices' sizes, the degenerate geometry, the NaN ruling, the gate at equality, ties, the
list limit and the mask, and one moderate synthetic scene."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import patch_match_cases as pm_cases
from tests import source_selection_fixtures as fx
from tests import source_selection_ref as ref

pytestmark = pytest.mark.gpu

SCHEDULES = ["product", "serial"]


def _schedule(monkeypatch, schedule):
    if schedule == "serial":
        monkeypatch.setenv("DSM_SOURCE_SELECTION_SERIAL", "1")  # the check build's one lane: the reference's loops


def _run(dsm, case_name):
    _, model_name, kw = fx.case(case_name)
    m = fx.model(model_name)
    return dsm.select_source_images(m["R"], m["T"], m["xyz"], m["tracks"], **dict(kw))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("case_name", fx.case_names())
def test_case_equals_the_restatement(dsm, monkeypatch, case_name, schedule):
    _schedule(monkeypatch, schedule)
    want = fx.reference(case_name)
    assert (want["nan_items"] > 0) == (fx.case(case_name)[1] in fx.NAN_MODELS)
    got = _run(dsm, case_name)
    assert fx.same(got, want) is None, fx.same(got, want)
    assert got["stats"] == {"items": want["items"], "pairs": want["n_pairs"], "nan_items": want["nan_items"]}
    times = dsm.source_selection_time()
    assert tuple(times) == capi.SOURCE_SELECTION_STAGES
    assert (times["items_count"], times["pairs"], times["nan_items"]) == (want["items"], want["n_pairs"], want["nan_items"])
    assert all(times[k] >= 0 for k in capi.SOURCE_SELECTION_STAGES)


def test_fixtures_show_what_they_are_for():
    """The conditions under which the cases above show anything (the restatement's side; no device call)."""
    tracks = fx.model("tracks")["tracks"]
    assert sorted(set(len(t) for t in tracks)) == [0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 363]
    assert len(tracks[0]) == 0 and len(tracks[2]) == 0 and len(tracks[-2]) == 0 and len(tracks[-1]) == 2  # points between and after empty tracks
    assert [4, 11, 4, 20, 4] in tracks and [6, 6, 6, 6] in tracks
    assert sorted(fx.reference("pairs_p75")["pairs"][2].tolist()) == sorted(fx.PAIR_COUNTS)
    images = fx.model("images")
    kept = [sum(1 for p, t in enumerate(images["tracks"]) if t == [a] and ref.depth(images["R"][a], images["T"][a], images["xyz"][p]) > 0)
            for a in range(2, 2 + len(fx.DEPTH_COUNTS))]
    assert tuple(kept) == fx.DEPTH_COUNTS
    ranges = fx.reference("images")["depth_ranges"]
    assert ranges[0].tolist() == [-1, -1] and ranges[1].tolist() == [-1, -1] and (ranges[2:] > 0).all()
    geometry = fx.model("geometry")
    centers = [ref.projection_center(geometry["R"][a], geometry["T"][a]) for a in range(4)]
    assert ref.item_quotient(centers[1], centers[0], [float(v) for v in geometry["xyz"][0]]) < 0  # obtuse: the pi - a branch
    assert ref.item_quotient(centers[1], centers[0], [float(v) for v in geometry["xyz"][1]]) is None  # a point at a centre
    assert centers[1] == centers[2]
    assert fx.reference("gate")["sources"][0] == [4, 1, 2, 3] and fx.reference("gate_mask")["sources"][0] == [1, 2, 3]
    assert 4 in fx.reference("gate_equal")["sources"][0] and 4 not in fx.reference("gate_above")["sources"][0]
    assert [len(fx.reference("gate_max%d" % m)["sources"][0]) for m in (0, 1, 4, 7)] == [0, 1, 4, 4]
    scene = fx.reference("scene")
    assert len(scene["sources"]) == 240 and 5e4 <= scene["items"] <= 2e5 and scene["nan_items"] == 0


def test_two_calls_return_the_same_bytes(dsm):
    first, second = _run(dsm, "scene"), _run(dsm, "scene")
    assert first["sources"] == second["sources"]
    assert first["depth_ranges"].tobytes() == second["depth_ranges"].tobytes()
    for a, b in zip(first["pairs"], second["pairs"]):
        assert a.tobytes() == b.tobytes()
    times = dsm.source_selection_time()
    want = fx.reference("scene")
    assert times["items_count"] == want["items"] and times["pairs"] == want["n_pairs"]
    assert all(times[k] > 0 for k in ("upload", "depths", "items", "sort", "pairs_select", "download"))


def test_memory_budget_too_small_is_refused_whole(dsm):
    m = fx.model("scene")
    want = fx.reference("scene")
    dsm.set_memory_budget(1 << 16)  # the items alone are 2 x 8 bytes x ~1e5
    try:
        with pytest.raises(capi.DsmError, match=r"need \d+ bytes, the memory budget is 65536 bytes") as e:
            dsm.select_source_images(m["R"], m["T"], m["xyz"], m["tracks"])
        assert e.value.rc == 4  # DSM_ERR_OUT_OF_RANGE
    finally:
        dsm.set_memory_budget(0)
    dsm.set_memory_budget(1 << 30)
    try:
        got = dsm.select_source_images(m["R"], m["T"], m["xyz"], m["tracks"])
    finally:
        dsm.set_memory_budget(0)
    assert fx.same(got, want) is None


def test_invalid_arguments_and_empty_models(dsm):
    m = fx.model("gate")
    for kw in ({"max_num_src_images": -1}, {"triangulation_angle_percentile": 100.5}, {"min_triangulation_angle": float("nan")}):
        with pytest.raises(capi.DsmError):
            dsm.select_source_images(m["R"], m["T"], m["xyz"], m["tracks"], **kw)
    with pytest.raises(capi.DsmError, match="out of range"):
        dsm.select_source_images(m["R"], m["T"], m["xyz"], [[0, 6]] + m["tracks"][1:])
    empty = dsm.select_source_images(np.zeros((0, 9)), np.zeros((0, 3)), np.zeros((0, 3)), [])
    assert empty["sources"] == [] and len(empty["pairs"][0]) == 0
    no_points = dsm.select_source_images(m["R"], m["T"], np.zeros((0, 3)), [])
    assert no_points["sources"] == [[]] * 6 and (no_points["depth_ranges"] == -1).all()
    only_empty_tracks = dsm.select_source_images(m["R"], m["T"], np.ones((3, 3)), [[], [], []])
    assert only_empty_tracks["sources"] == [[]] * 6 and (only_empty_tracks["depth_ranges"] == -1).all()
    single = dsm.select_source_images(m["R"], m["T"], np.ones((2, 3)), [[3], [3]])  # track elements, no item
    assert single["sources"] == [[]] * 6 and dsm.source_selection_time()["items_count"] == 0


def test_problems_to_patch_match_end_to_end(dsm):
    """patch_match_problems -> patch_match_stereo on 3 images of 32 x 24 with `__auto__, 2` equals the same PatchMatch call with
    the restatement's lists and ranges passed by hand."""
    sizes = ((32, 24),) * 3
    images, truth = pm_cases.scene("slanted", sizes)
    # a sparse model on the plane: every fourth pixel of view 0 back-projected at its true depth (view 0: R = I, C = 0)
    K = np.asarray(images[0]["K"], dtype=np.float64).reshape(3, 3)
    xyz = []
    for y in range(2, 24, 4):
        for x in range(2, 32, 4):
            d = truth[0]["depth"][y, x]
            xyz.append([(x - K[0, 2]) / K[0, 0] * d, (y - K[1, 2]) / K[1, 1] * d, d])
    tracks = [[0, 1, 2] if k % 3 else [2, 0] for k in range(len(xyz))]
    model = {"R": [im["R"] for im in images], "T": [im["T"] for im in images], "xyz": xyz, "tracks": tracks}
    config = ["# written by hand", "0", "__auto__, 2", "", "1", "__auto__, 2", "2", "__auto__, 2"]
    problems = dsm.patch_match_problems(model, config, {"min_triangulation_angle": 1.0})
    want = ref.select(np.asarray(model["R"]), np.asarray(model["T"]), np.asarray(xyz), tracks, max_num_src_images=2, candidate_mask=[1, 1, 1])
    assert want["nan_items"] == 0 and all(len(s) == 2 for s in want["sources"])
    by_hand = [(a, want["sources"][a], float(want["depth_ranges"][a][0]), float(want["depth_ranges"][a][1])) for a in range(3)]
    assert problems == by_hand
    o = pm_cases.capi_options(pm_cases.options())
    got = dsm.patch_match_stereo(images, problems, o)
    expect = dsm.patch_match_stereo(images, by_hand, o)
    assert len(got) == 3
    for k in range(3):
        pm_cases.assert_same_bits(got[k], expect[k], "problem %d" % k)
        assert np.isfinite(got[k]["depth"]).all() and (got[k]["depth"] > 0).any()
