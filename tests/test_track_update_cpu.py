"""CompleteTracks / MergeTracks without a GPU: the restatement (tests/track_update_ref.py) against hand-computed
answers, one per branch of the reference, and the host build of csrc/track_update.h (libdsm_track_update_host.so: the text the
kernels are built from) against the restatement -- ids, track order, modified ids, step counts and trial counts exactly, xyz bit
for bit.  Every scene has all decision margins clear of 1e-9 under the restatement."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import track_update_ref as ref
from tests import track_update_scenes as scenes

MERGE, COMPLETE = ref.MERGE, ref.COMPLETE
CASES, random_scene, invalid_cases = scenes.CASES, scenes.named_random_scene, scenes.invalid_cases


def test_binding_and_switch_exist():
    assert hasattr(capi.Context, "update_tracks") and hasattr(capi.Context, "complete_and_merge_tracks")
    assert hasattr(capi.Context, "merge_and_complete_tracks") and "DSM_TRACK_UPDATE_SERIAL" in capi.CHECK_OPTION_KEYS
    o = capi.TrackUpdateOptions()
    capi.track_update_host_lib().dsm_tu_host_default_options(ctypes.byref(o))
    # incremental_triangulator.h: complete_max_reproj_error, merge_max_reproj_error, complete_max_transitivity and the bogus limits
    assert (o.complete_max_reproj_error, o.merge_max_reproj_error, o.complete_max_transitivity) == (4.0, 4.0, 5)
    assert (o.tri.min_focal_length_ratio, o.tri.max_focal_length_ratio, o.tri.max_extra_param) == (0.1, 10.0, 1.0)
    d = ref.default_options()
    assert (d["complete_max_reproj_error"], d["merge_max_reproj_error"], d["complete_max_transitivity"]) == (4.0, 4.0, 5)


@pytest.mark.parametrize("name", sorted(CASES))
def test_known_answer(name):
    """The restatement and the host build both give the hand-computed tracks, counts, modified ids, xyz and trial counts."""
    c = CASES[name]
    exp = ref.update_tracks(c["scene"], c["steps"], c["selected"], **c["options"])
    assert ref.min_margin(exp) >= scenes.MIN_MARGIN
    got = capi.update_tracks_host(c["scene"], c["steps"], c["selected"], **c["options"])
    for r in (exp, got):
        scenes.check_case(c, r)
        ct, mt = scenes.trial_counts(r)
        assert c["complete_trials"] in (None, ct) and c["merge_trials"] in (None, mt), (ct, mt)
    scenes.same_result(got, exp)


def test_step_orders_differ():
    a, b = CASES["complete_then_merge"], CASES["merge_then_complete"]
    ra = capi.update_tracks_host(a["scene"], a["steps"])
    rb = capi.update_tracks_host(b["scene"], b["steps"])
    assert [int(i) for i in ra["point_ids"]] == [3, 8] and [int(i) for i in rb["point_ids"]] == [9]


@pytest.mark.parametrize("name", ["small", "medium", "unregistered", "forty"])
@pytest.mark.parametrize("steps", scenes.STEP_ORDERS, ids=["complete_merge", "merge_complete"])
def test_host_build_equals_restatement(name, steps):
    s = random_scene(name)
    exp = ref.update_tracks(s, steps)
    assert ref.min_margin(exp) >= scenes.MIN_MARGIN
    assert exp["step_counts"].min() > 0, "the scene must exercise both steps"
    got = capi.update_tracks_host(s, steps)
    scenes.same_result(got, exp)
    assert int(got["report"].num_merge_events) == len(s["point3D_ids"]) - len(exp["point_ids"])
    assert min(got["report"].min_complete_error_margin, got["report"].min_merge_error_margin, got["report"].min_depth_margin) >= scenes.MIN_MARGIN


def test_selection_and_repeated_steps():
    """The AdjustLocalBundle order over every third id (ids merged away are skipped, merged ids are not in the set), and a call
    of four steps: MERGE's memo is cleared per step."""
    s = random_scene("medium")
    ids = np.sort(np.asarray(s["point3D_ids"]))[::3]
    scenes.same_result(capi.update_tracks_host(s, [MERGE, COMPLETE], ids), ref.update_tracks(s, [MERGE, COMPLETE], ids))
    steps = [COMPLETE, MERGE, MERGE, COMPLETE]
    scenes.same_result(capi.update_tracks_host(s, steps), ref.update_tracks(s, steps))


def test_input_order_does_not_matter():
    s = random_scene("medium")
    for steps in scenes.STEP_ORDERS:
        base = capi.update_tracks_host(s, steps)
        scenes.same_result(capi.update_tracks_host(scenes.shuffled_points(s, 3), steps), base)
        scenes.same_result(capi.update_tracks_host(scenes.shuffled_matches(s, 4), steps), base)


@pytest.mark.parametrize("builder,arg", [(scenes.long_track, 16), (scenes.long_track, 17), (scenes.long_track, 30), (scenes.long_track, 31), (scenes.long_track, 62), (scenes.long_track, 63), (scenes.long_track, 64), (scenes.long_track, 65), (scenes.long_track, 257),
                                         (scenes.wide_level, 64), (scenes.wide_level, 65), (scenes.claim_chain, 1), (scenes.claim_chain, 2),
                                         (scenes.claim_chain, 9), (scenes.merge_chain, 1), (scenes.merge_chain, 2), (scenes.merge_chain, 64),
                                         (scenes.merge_chain, 65)])
def test_edge_scenes(builder, arg):
    s = builder(arg)
    for steps in scenes.STEP_ORDERS:
        exp = ref.update_tracks(s, steps)
        assert ref.min_margin(exp) >= scenes.MIN_MARGIN
        scenes.same_result(capi.update_tracks_host(s, steps), exp)
    if builder is scenes.merge_chain:  # one point is left, with the last of the n - 1 ids handed out
        exp = ref.update_tracks(s, [MERGE])
        assert len(exp["point_ids"]) == 1 and int(exp["step_counts"][0]) == (2 * arg if arg > 1 else 0)
        assert int(exp["point_ids"][0]) == (50 + 2 * (arg - 1) + (arg - 1) if arg > 1 else 50)
    if builder is scenes.claim_chain:  # p_j takes c_j; the last point takes nothing
        exp = ref.update_tracks(s, [COMPLETE])
        assert int(exp["step_counts"][0]) == arg - 1
        assert list(np.diff(exp["track_offsets"].astype(np.int64))) == [3] * (arg - 1) + [2]
    if builder is scenes.wide_level:
        assert int(ref.update_tracks(s, [COMPLETE])["step_counts"][0]) == 2 * arg


@pytest.mark.parametrize("case", invalid_cases(), ids=lambda c: c[0])
def test_invalid_arguments(case):
    _, s, steps, selected, next_id, kw = case
    with pytest.raises(capi.DsmError):
        capi.update_tracks_host(s, steps, selected, next_id, **kw)
    if "threshold" not in case[0] and case[0] not in ("unknown_step", "track_unknown_image", "track_index_out_of_range",
                                                      "track_unregistered_image", "non_finite_xyz", "self_pair", "repeated_pair",
                                                      "match_out_of_range", "track_offsets_descend"):
        with pytest.raises((ValueError, KeyError)):  # the rulings the restatement states itself
            ref.update_tracks(s, steps, selected, next_id, **kw)


def test_apply_track_update_round_trip():
    """The result written back is a scene the next call takes: MERGE alone, then COMPLETE on the scene written back, is the
    two-step call; points2D_point3D names the owner of every track element."""
    s = random_scene("small")
    r = capi.update_tracks_host(s, [MERGE])
    s2 = capi.apply_track_update(s, r)
    r2 = capi.update_tracks_host(s2, [COMPLETE])
    both = capi.update_tracks_host(s, [MERGE, COMPLETE])
    for key in ("point_ids", "track_offsets", "track_obs"):
        assert np.array_equal(r2[key], both[key]), key
    assert r2["xyz"].tobytes() == both["xyz"].tobytes()
    r = both
    s2 = capi.apply_track_update(s, r)
    p3 = s2["points2D_point3D"]
    assert (p3 >= 0).sum() == len(r["track_obs"])
    arrays = capi.bundle_arrays(s2)
    assert arrays["obs_xy"].shape == (len(r["track_obs"]), 2) and arrays["track_offsets"][-1] == len(r["track_obs"])
