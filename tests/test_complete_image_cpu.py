"""CompleteImage without a GPU: the restatement (tests/complete_image_ref.py) against the hand-computed answers of
tests/complete_image_scenes.py, the margins of the random scenes the GPU suite uses, the restatement against CompleteTracks where
the two must agree, and the entry point's declaration, binding and export."""
import os
import re
import subprocess

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import complete_image_ref as ref
from tests import complete_image_scenes as scenes
from tests import track_update_ref as tu
from tests import track_update_scenes as tus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "dagsfm_mi355x.h")).read()
    assert re.search(r"\bint dsm_complete_images\(dsm_ctx\* ctx,", header) and "} dsm_complete_images_report;" in header
    assert hasattr(capi.Context, "complete_images") and hasattr(capi.Context, "adjust_local_bundle_tracks")
    assert "DSM_COMPLETE_IMAGE_SERIAL" in capi.CHECK_OPTION_KEYS and "DSM_COMPLETE_IMAGE_SERIAL" not in capi.PRODUCT_OPTION_KEYS
    ctx_h = open(os.path.join(ROOT, "dagsfm_amd", "csrc", "ctx.h")).read()
    assert '"DSM_COMPLETE_IMAGE_SERIAL"' in ctx_h.split("dsm_check_debug_keys")[1]
    assert '"DSM_COMPLETE_IMAGE_SERIAL"' not in ctx_h.split("dsm_check_debug_keys")[0]
    syms = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT dsm_complete_images\b", syms)
    assert capi.lib().dsm_complete_images.argtypes is not None


@pytest.mark.parametrize("name", sorted(scenes.CASES))
def test_restatement_gives_the_hand_computed_answers(name):
    c = scenes.CASES[name]
    got = ref.complete_images(c["scene"], c["images"], c["steps"], c["selected"], **c["options"])
    scenes.check_case(c, got)


def test_carried_min_num_trials_is_what_changes_the_count():
    """The two items of carried_min_trials one by one: the list of 16 runs with the 3 the list of 3 left (5 trials), and with 0
    where it is alone in its image (3 trials)."""
    one = ref.complete_images(scenes.CASES["carried_min_trials"]["scene"], scenes.CASES["carried_min_trials"]["images"])
    two = ref.complete_images(scenes.CASES["carried_resets_per_image"]["scene"], scenes.CASES["carried_resets_per_image"]["images"])
    assert [(n, m, t) for _, _, n, m, t in one["items"]] == [(3, 3, 3), (16, 3, 5)]
    assert [(n, m, t) for _, _, n, m, t in two["items"]] == [(3, 3, 3), (16, 0, 3)]


@pytest.mark.parametrize("name", sorted(scenes.RANDOM))
def test_random_scenes_are_clear_of_rounding(name):
    """Every random scene the GPU suite uses has all margins at MIN_MARGIN or above under the restatement; a seed that has not
    is replaced by the next one, and at most 1 of any 10 consecutive seeds may be skipped."""
    scene, ids, steps, exp, skipped = scenes.named_random_scene(name)
    assert ref.min_margin(exp) >= scenes.MIN_MARGIN
    assert skipped <= scenes.MAX_SEED_SKIPS
    assert exp["num_new_points"] > 0 and exp["num_completed_observations"] + int(sum(exp["step_counts"])) > 0


def test_camera_model_scenes_are_clear_of_rounding():
    """The seeds of the GPU suite's scenes per camera model (ImageToWorld is the oracle's): the same condition on the seeds."""
    from tests import oracle_lib
    orc = oracle_lib.load()
    to_world = lambda cam, xy: orc.image_to_world(cam, np.asarray(xy, np.float64))
    for model in range(11):
        _, _, exp, skipped = scenes.model_scene(model, to_world)
        assert ref.min_margin(exp) >= scenes.MIN_MARGIN and skipped <= scenes.MAX_SEED_SKIPS, model
        assert exp["num_new_points"] > 0, model


def test_all_points2D_with_points_is_complete_tracks():
    """An image whose point2Ds all have points, with ids ascending in point2D order: CompleteImage is Complete of those ids in
    that order, which is CompleteTracks over them."""
    s = tus.named_random_scene("small")
    sc = tu.rt.Scene(s)
    i = 3
    off, n = int(sc.off[i]), sc.nfeat(i)
    toff = np.asarray(s["track_offsets"], np.int64)
    tobs = np.asarray(s["track_obs"], np.int64).reshape(-1, 2)
    iid = int(s["image_ids"][i])
    owner = {}
    for p in range(len(toff) - 1):
        for im, k in tobs[toff[p]:toff[p + 1]]:
            if im == iid:
                owner[int(k)] = p
    with_point = sorted(owner)
    assert len(with_point) >= 5 and len(set(owner.values())) == len(owner)
    # the image reduced to its point2Ds with a point, and their points renumbered ascending in point2D order
    keep = np.array(with_point)
    new_index = {int(k): j for j, k in enumerate(keep)}
    s2 = dict(s)
    nf = np.diff(np.asarray(s["points2D_offsets"], np.int64))
    nf[i] = len(keep)
    s2["points2D_offsets"] = np.concatenate([[0], np.cumsum(nf)]).astype(np.uint32)
    xy = np.asarray(s["points2D_xy"], np.float64).reshape(-1, 2)
    s2["points2D_xy"] = np.concatenate([xy[:off], xy[off + keep], xy[off + n:]])
    tobs2 = tobs.copy()
    for e in range(len(tobs2)):
        if tobs2[e, 0] == iid:
            tobs2[e, 1] = new_index[int(tobs2[e, 1])]
    s2["track_obs"] = tobs2.astype(np.uint32)
    pairs = np.asarray(s["pairs"], np.int64).reshape(-1, 2)
    moff = np.asarray(s["match_offsets"], np.int64)
    m = np.asarray(s["matches"], np.int64).reshape(-1, 2)
    out_m, out_off = [], [0]
    for k, (a, b) in enumerate(pairs):
        for i1, i2 in m[moff[k]:moff[k + 1]]:
            if a == iid:
                if int(i1) not in new_index:
                    continue
                i1 = new_index[int(i1)]
            if b == iid:
                if int(i2) not in new_index:
                    continue
                i2 = new_index[int(i2)]
            out_m.append((i1, i2))
        out_off.append(len(out_m))
    s2["matches"], s2["match_offsets"] = np.array(out_m, np.uint32).reshape(-1, 2), np.array(out_off, np.uint64)
    ids = np.asarray(s["point3D_ids"], np.uint64).copy()
    base = int(ids.max()) + 1
    sel = []
    for j, k in enumerate(with_point):
        ids[owner[k]] = base + j
        sel.append(base + j)
    s2["point3D_ids"] = ids
    a = ref.complete_images(s2, [iid])
    b = tu.update_tracks(s2, [tu.COMPLETE], selected=sel)
    for key in ("point_ids", "track_offsets", "track_obs", "modified"):
        assert np.array_equal(np.asarray(a[key], np.int64), np.asarray(b[key], np.int64)), key
    assert a["xyz"].tobytes() == b["xyz"].tobytes()
    assert int(a["image_num_tris"][0]) == int(b["step_counts"][0]) > 0
    assert a["complete_trials"] == b["complete_trials"] and a["ransac_trials"] == 0


def test_steps_then_images_is_two_calls_of_the_restatement():
    """[MERGE, COMPLETE] and the images in one run equal update_tracks, the result applied, then the images alone with the id
    counter where the merge events left it."""
    scene, ids, steps, exp, _ = scenes.named_random_scene("small_steps")
    st = tu.State(scene)
    counts = [st.step(int(k), None) for k in steps]
    first = tu.update_tracks(scene, steps)
    assert [int(c) for c in first["step_counts"]] == counts
    second = ref.complete_images(capi.apply_track_update(scene, first), ids, next_point3D_id=st.next_id)
    for key in ("point_ids", "track_offsets", "track_obs", "image_num_tris"):
        assert np.array_equal(np.asarray(second[key], np.int64), np.asarray(exp[key], np.int64)), key
    assert second["xyz"].tobytes() == exp["xyz"].tobytes()
    assert second["ransac_trials"] == exp["ransac_trials"] and st.next_id > int(np.asarray(scene["point3D_ids"]).max()) + 1


@pytest.mark.parametrize("case", scenes.invalid_cases(), ids=lambda c: c[0])
def test_restatement_refuses_what_the_entry_refuses(case):
    _, s, ids, kw = case
    with pytest.raises(ValueError):
        ref.complete_images(s, ids, **kw)
