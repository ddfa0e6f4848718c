"""dsm_complete_images on the device against the restatement (tests/complete_image_ref.py) and the hand-computed
answers of tests/complete_image_scenes.py: tracks, ids, image_num_tris, modified ids, complete_trials and ransac_trials exactly,
existing points' xyz bit for bit, new points' xyz within 1e-9 relative (DESIGN.md 13's tolerance: numpy's SVD and eigh round
differently from the device's Jacobi sweeps).  Every random scene keeps its decision margins at 1e-9 or above under the
restatement (tests/test_complete_image_cpu.py holds that without a GPU)."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import complete_image_ref as ref
from tests import complete_image_scenes as scenes
from tests import oracle_lib
from tests import track_update_scenes as tus

pytestmark = pytest.mark.gpu
MERGE, COMPLETE = ref.MERGE, ref.COMPLETE
CASES = scenes.CASES


@pytest.fixture(scope="module", params=["product", "check"])
def ctx(request):
    return capi.Context(0, check=request.param == "check")


@pytest.fixture(scope="module")
def to_world():
    orc = oracle_lib.load()
    return lambda cam, xy: orc.image_to_world(cam, np.asarray(xy, np.float64))


def counts_agree(got, exp):
    r = got["report"]
    assert (int(r.num_new_points), int(r.num_new_observations), int(r.num_completed_observations)) == (
        exp["num_new_points"], exp["num_new_observations"], exp["num_completed_observations"])
    assert int(sum(got["image_num_tris"])) == exp["num_new_observations"] + exp["num_completed_observations"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_known_answer(ctx, name):
    c = CASES[name]
    got = ctx.complete_images(c["scene"], c["images"], c["steps"], c["selected"], **c["options"])
    scenes.check_case(c, got)
    exp = ref.complete_images(c["scene"], c["images"], c["steps"], c["selected"], **c["options"])
    scenes.same_result(got, exp)
    counts_agree(got, exp)
    assert got["report"].num_serial_items == 0 and got["report"].num_rounds == (1 if got["report"].num_items else 0)


def test_carried_min_num_trials_ran_ahead_with_the_right_value(ctx):
    """The list of 16 behind the list of 3 is estimated ahead with the 3 its predecessor leaves, and with 0 in an image of its
    own: neither falls back to the commit lane."""
    for name, trials in (("carried_min_trials", 8), ("carried_resets_per_image", 6)):
        c = CASES[name]
        r = ctx.complete_images(c["scene"], c["images"])["report"]
        assert (int(r.ransac_trials), int(r.num_estimated_ahead), int(r.num_serial_items)) == (trials, 2, 0)


def test_mispredicted_carried_value_is_estimated_again(ctx):
    """Image 0: point2D 0 has point 10 = [a0, p1]; its Complete walks p1 -> ca0 -> ra -> ca1 and takes all three.  ra (point2D
    1, a list of 3) was a candidate before the image ran, so the list of 16 behind it (point2D 2) was estimated ahead with the
    3 it would have left; at its turn ra has a point and runs Complete, the carried value is still 0, and the list of 16 is
    estimated again on the commit lane: 3 trials, not 5."""
    t = scenes.Tiny(17)
    Xa, Xb = scenes.O, scenes.X(3)
    a0, ra, rb = t.feat(0, Xa), t.feat(0, Xa), t.feat(0, Xb)
    ca = [t.feat(1, Xa), t.feat(2, Xa)]
    cb = [t.feat(i, Xb) for i in range(1, 16)]
    p1 = t.feat(3, Xa)
    for x in ca:
        t.link(ra, x)
    for x in cb:
        t.link(rb, x)
    t.link(a0, p1)
    t.link(p1, ca[0])
    t.point(10, Xa, [a0, p1])
    s = t.scene()
    got = ctx.complete_images(s, [t.image_id(0)])
    exp = ref.complete_images(s, [t.image_id(0)])
    scenes.same_result(got, exp)
    assert [(n, m, tr) for _, _, n, m, tr in exp["items"]] == [(16, 0, 3)] and [int(x) for x in exp["image_num_tris"]] == [3 + 16]
    r = got["report"]
    assert (int(r.ransac_trials), int(r.complete_trials), int(r.num_estimated_ahead), int(r.num_serial_items)) == (3, 3, 2, 1)


@pytest.mark.parametrize("name", sorted(scenes.RANDOM))
def test_random_scenes(ctx, name):
    """forty: the 40-image synthetic scene, three of its images; small_steps: [MERGE, COMPLETE] first"""
    scene, ids, steps, exp, _ = scenes.named_random_scene(name)
    got = ctx.complete_images(scene, ids, steps)
    scenes.same_result(got, exp)
    counts_agree(got, exp)
    assert scenes.old_xyz_same_bytes(scene, got) > 0
    r = got["report"]
    assert r.num_new_points > 0 and r.num_estimated_ahead >= r.num_new_points and r.num_items > r.num_estimated_ahead
    for key in ("min_residual_margin", "min_support_margin", "min_angle_margin", "min_depth_margin", "min_complete_error_margin",
                "min_bogus_margin"):
        assert getattr(r, key) >= scenes.MIN_MARGIN, key


@pytest.mark.parametrize("model", range(11))
def test_every_camera_model(ctx, to_world, model):
    scene, ids, exp, _ = scenes.model_scene(model, to_world)
    got = ctx.complete_images(scene, ids)
    scenes.same_result(got, exp)
    counts_agree(got, exp)
    assert got["report"].num_new_points > 0


def test_both_list_orders(ctx):
    scene, ids, _, exp, _ = scenes.named_random_scene("small")
    back = ids[::-1]
    exp_back = ref.complete_images(scene, back)
    assert ref.min_margin(exp_back) >= scenes.MIN_MARGIN
    got = ctx.complete_images(scene, back)
    scenes.same_result(got, exp_back)
    assert not np.array_equal(exp_back["track_obs"], exp["track_obs"])  # the order of the list changes the result


def test_same_bytes_across_repeats_and_input_orders(ctx):
    scene, ids, _, _, _ = scenes.named_random_scene("forty")
    steps = [MERGE, COMPLETE]
    base = scenes.result_bytes(ctx.complete_images(scene, ids, steps))
    assert scenes.result_bytes(ctx.complete_images(scene, ids, steps)) == base
    assert scenes.result_bytes(ctx.complete_images(tus.shuffled_points(scene, 3), ids, steps)) == base
    assert scenes.result_bytes(ctx.complete_images(tus.shuffled_matches(scene, 4), ids, steps)) == base


def test_serial_form_and_exhausted_pool_give_the_same_bytes(monkeypatch):
    """The check build's DSM_COMPLETE_IMAGE_SERIAL=1 (every estimate on the commit lane) and an estimate pool of 40 list
    entries (the estimates behind it fall back) against the product, in fresh contexts."""
    scene, ids, _, exp, _ = scenes.named_random_scene("forty")
    steps = [MERGE, COMPLETE]
    product = capi.Context(0, check=False)
    base = product.complete_images(scene, ids, steps)
    assert base["report"].num_serial_items == 0
    for value in ("1", "pool:40"):
        monkeypatch.setenv("DSM_COMPLETE_IMAGE_SERIAL", value)
        check = capi.Context(0)
        assert check.check
        got = check.complete_images(scene, ids, steps)
        assert scenes.result_bytes(got) == scenes.result_bytes(base)
        assert scenes.trial_counts(got) == scenes.trial_counts(base)
        r = got["report"]
        assert r.num_serial_items > 0 and (r.num_estimated_ahead == 0) == (value == "1")
        if value != "1":
            assert 0 < r.num_estimated_ahead < base["report"].num_estimated_ahead
    monkeypatch.delenv("DSM_COMPLETE_IMAGE_SERIAL")


def test_steps_and_images_in_one_call_equal_two_calls(ctx):
    """[MERGE, COMPLETE] + the images equals update_tracks, apply_track_update, then complete_images without steps, the id
    counter continuing behind the merge events."""
    scene, ids, steps, exp, _ = scenes.named_random_scene("small_steps")
    one = ctx.complete_images(scene, ids, steps)
    first = ctx.update_tracks(scene, steps)
    next_id = int(np.asarray(scene["point3D_ids"]).max()) + 1 + int(first["report"].num_merge_events)
    assert first["report"].num_merge_events > 0
    second = ctx.complete_images(capi.apply_track_update(scene, first), ids, next_point3D_id=next_id)
    for key in ("point_ids", "xyz", "track_offsets", "track_obs", "image_num_tris"):
        assert np.ascontiguousarray(one[key]).tobytes() == np.ascontiguousarray(second[key]).tobytes(), key
    assert np.array_equal(one["step_counts"], first["step_counts"])
    assert int(one["report"].ransac_trials) == int(second["report"].ransac_trials)
    assert int(one["report"].steps.complete_trials) == int(first["report"].complete_trials)
    assert int(one["report"].complete_trials) == int(first["report"].complete_trials) + int(second["report"].complete_trials)
    capi.apply_track_update(scene, one)


def test_adjust_local_bundle_tracks(ctx):
    scene, _, _, _, _ = scenes.named_random_scene("small")
    image_id = int(scene["image_ids"][4])
    variable = np.sort(np.asarray(scene["point3D_ids"]))[::2]
    exp = ref.complete_images(scene, [image_id], [MERGE, COMPLETE], variable)
    assert ref.min_margin(exp) >= scenes.MIN_MARGIN
    got = ctx.adjust_local_bundle_tracks(scene, image_id, variable)
    scenes.same_result(got, exp)
    assert got["num_merged_observations"] == int(exp["step_counts"][0])
    assert got["num_completed_observations"] == int(exp["step_counts"][1]) + int(exp["image_num_tris"][0]) > 0
    out = capi.apply_track_update(scene, got)
    assert len(out["point3D_ids"]) == len(got["point_ids"]) and (out["points2D_point3D"] >= 0).sum() == len(got["track_obs"])


@pytest.mark.parametrize("case", scenes.invalid_cases() + [(c[0], c[1], [1], c[5]) for c in tus.invalid_cases()
                                                           if c[0] in ("feature_in_two_tracks", "repeated_pair", "self_pair")],
                         ids=lambda c: c[0])
def test_invalid_arguments(ctx, case):
    _, s, ids, kw = case
    with pytest.raises(capi.DsmError):
        ctx.complete_images(s, ids, **kw)


def test_invalid_arguments_leave_the_outputs_untouched(ctx):
    """The C entry with sentinel-filled outputs: DSM_ERR_INVALID_ARGUMENT and not a byte written."""
    import ctypes
    c = CASES["order_A_C"]
    s = c["scene"]
    a = lambda key, dt, shape=-1: np.ascontiguousarray(s[key], dt).reshape(shape)
    cam_ids, cams = a("camera_ids", np.uint32), (capi.Camera * 2)(*s["cameras"])
    img_ids, img_cam, reg = a("image_ids", np.uint32), a("image_camera_ids", np.uint32), a("registered", np.uint8)
    N = len(img_ids)
    qvec, tvec, poff, xy = a("qvec", np.float64, (N, 4)), a("tvec", np.float64, (N, 3)), a("points2D_offsets", np.uint32), a("points2D_xy", np.float64)
    pairs, moff, m = a("pairs", np.uint32), a("match_offsets", np.uint64), a("matches", np.uint32)
    pids, pxyz, toff, tobs = np.zeros(1, np.uint64), np.zeros(3), a("track_offsets", np.uint64), np.zeros(2, np.uint32)
    outs = [np.full(64, 0xAB, np.uint8) for _ in range(9)]
    before = [o.copy() for o in outs]
    rep = capi.CompleteImagesReport()
    ctypes.memset(ctypes.addressof(rep), 0xAB, ctypes.sizeof(rep))
    rep_before = bytes(rep)
    ptr = lambda x: x.ctypes.data
    for bad_ids, opts in (([1, 999], {}), ([1, 1], {}), ([1], dict(max_transitivity=2)), ([1], dict(ransac_max_num_trials=0)),
                          ([1], dict(ransac_confidence=1.5)), ([1], dict(min_angle=float("inf")))):
        ci = np.array(bad_ids, np.uint32)
        o = capi.default_track_update_options(**opts)
        rc = ctx._L.dsm_complete_images(ctx._h, len(cam_ids), ptr(cam_ids), ctypes.addressof(cams), N, ptr(img_ids), ptr(img_cam), ptr(reg),
                                        ptr(qvec), ptr(tvec), ptr(poff), ptr(xy), len(pairs) // 2, ptr(pairs), ptr(moff), ptr(m), 0, ptr(pids),
                                        ptr(pxyz), ptr(toff), ptr(tobs), 0, None, 0, None, 0, len(ci), ptr(ci), ctypes.byref(o),
                                        *[ptr(x) for x in outs], ctypes.addressof(rep))
        assert rc == capi.DSM_ERR_INVALID_ARGUMENT, (bad_ids, opts, rc)
        assert all((x == y).all() for x, y in zip(outs, before)) and bytes(rep) == rep_before


def test_existing_entries_keep_their_bytes(ctx):
    """dsm_update_tracks through the shared driver and dsm_retriangulate through rt_loransac.h return the bytes they returned
    before either moved: the digests in tests/golden/complete_image_parent_digests.json were recorded on the device from the
    library built from the commit before (tools/fuzz_complete_image.py --record-digests)."""
    import json
    import os
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "complete_image_parent_digests.json")))
    got = scenes.existing_entry_digests(ctx)
    assert sorted(got) == sorted(k for k in want if not k.startswith("_")) and len(got) >= 3
    for key, digest in got.items():
        assert digest == want[key], key
