"""Re-triangulation of the under-reconstructed pairs on the device (dsm_retriangulate_pairs) against the
sequential numpy restatement (tests/pair_retriangulation_ref.py): decisions identical and xyz within 1e-9 relative wherever
every margin of the scene is >= 1e-9; num_tris within 2 % otherwise.  Also the option gates, the trial counters, byte-identical
repeats, shuffles and pair orders, the argument errors, and the chain dsm_retriangulate -> dsm_retriangulate_pairs ->
dsm_bundle_adjust."""
import math
import os
import re

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import oracle_lib
from tests import pair_retriangulation_ref as ref
from tests.test_retriangulation_gpu import CAMS, shuffled

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
RTOL = 1e-9
_SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dagsfm_amd", "csrc", "retriangulation.hip")).read()
GATE_BLOCK = int(re.search(r"constexpr int RT_BLOCK = (\d+);", _SRC).group(1))  # k_rp_gate's workgroup
assert re.search(r"hipLaunchKernelGGL\(k_rp_gate, dim3\([^)]*\), dim3\(RT_BLOCK\)", _SRC)


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def to_world():
    orc = oracle_lib.load()
    return lambda cam, xy: orc.image_to_world(cam, np.asarray(xy, np.float64))


def triples(obs, ids):
    return [(int(a), int(b), int(c)) for (a, b), c in zip(obs, ids)]


def compare(dev, exp, clear_required=False):
    """True when compared decision for decision, False when the scene is unclear (totals checked)."""
    assert [int(x) for x in dev["pair_num_total_corrs"]] == exp["pair_num_total_corrs"]  # the duplicate rule: no rounding in it
    clear = ref.min_margin(exp) >= MARGIN
    if clear_required:
        assert clear, ref.min_margin(exp)
    if not clear:
        assert abs(int(dev["num_tris"]) - exp["num_tris"]) <= max(2, 0.02 * exp["num_tris"])
        return False
    rep = dev["report"]
    assert [int(x) for x in dev["pair_status"]] == exp["pair_status"]
    assert [int(x) for x in dev["pair_num_tri_corrs"]] == exp["pair_num_tri_corrs"]
    assert [int(x) for x in dev["re_num_trials"]] == exp["re_num_trials"]
    assert int(dev["num_tris"]) == exp["num_tris"] == rep.num_tris
    assert [int(x) for x in dev["new_point_ids"]] == exp["new_point_ids"]
    assert [[tuple(int(v) for v in o) for o in t] for t in dev["new_track_obs"]] == exp["new_tracks"]
    if exp["new_xyz"]:
        e = np.array(exp["new_xyz"])
        assert (np.abs(dev["new_xyz"] - e) <= RTOL * np.maximum(np.abs(e), 1.0)).all()
    assert triples(dev["continued_obs"], dev["continued_point_ids"]) == exp["continued"]
    assert triples(dev["touched_obs"], dev["touched_point_ids"]) == exp["touched"]
    c = exp["counts"]
    assert (rep.num_both, rep.num_continue_tried, rep.num_continue_taken, rep.num_two_view_skipped, rep.num_create_tried,
            rep.num_create_taken) == (c["both"], c["continue_tried"], c["continue_taken"], c["two_view_skipped"],
                                      c["create_tried"], c["create_taken"])
    assert list(rep.num_pairs_by_status) == [exp["pair_status"].count(v) for v in range(6)]
    assert rep.num_correspondences == sum(exp["pair_num_total_corrs"])
    return True


def run(ctx, scene, to_world=None, re_num_trials=None, **kw):
    dev = ctx.retriangulate_pairs(scene, capi.default_pair_retriangulation_options(**kw), re_num_trials=re_num_trials)
    exp = ref.retriangulate_pairs(scene, options=kw, re_num_trials=re_num_trials, to_world=to_world)
    return dev, exp


def fold_dev(scene, dev):
    return ref.fold(scene, triples(dev["touched_obs"], dev["touched_point_ids"]), dev["new_point_ids"], dev["new_xyz"])


CLEAR_SETS = [dict(n_images=8, n_points=80, track=(3, 6), existing=0.3), dict(n_images=6, n_points=120, track=(4, 6), existing=0.15)]


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("params", range(2))
def test_clear_scenes_decision_for_decision(ctx, params, seed):
    """Smallest margin of these eight scenes under the restatement: 5.2e-2.  7 to 10 of their 15 to 25 pairs are
    open when the call starts and closed by their turn."""
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=seed, **CLEAR_SETS[params])
    dev, exp = run(ctx, s)
    assert compare(dev, exp, clear_required=True)
    assert ref.CLOSED_BY_ITS_TURN in exp["pair_status"] and dev["report"].num_rounds > 1
    assert exp["counts"]["continue_taken"] >= 12 and exp["counts"]["create_taken"] >= 12
    for key in ("min_residual_margin", "min_angle_margin", "min_depth_margin", "min_continue_margin", "min_bogus_margin"):
        assert getattr(dev["report"], key) >= MARGIN


@pytest.mark.parametrize("model", range(11))
def test_every_camera_model(ctx, to_world, model):
    mid, params = CAMS[model]
    cams = [capi.camera(mid, params, 640, 480), capi.simple_pinhole(480.0, 320.0, 240.0, 640, 480)]
    clear = 0
    for seed in range(3):
        s, _ = ref.make_scene(n_images=9, n_points=90, track=(3, 7), noise=0.3, wrong=0.1, existing=0.2, cameras=cams,
                              seed=100 * model + seed)
        dev, exp = run(ctx, s, to_world=to_world)
        assert exp["counts"]["continue_taken"] > 0 and exp["counts"]["create_taken"] > 0
        clear += compare(dev, exp)
    assert clear >= 2


def test_two_view_rule(ctx):
    s, _ = ref.make_scene(n_images=2, n_points=10, track=(2, 2), noise=0.05, wrong=0.0, seed=4)
    dev, exp = run(ctx, s)
    assert compare(dev, exp, clear_required=True)
    assert dev["num_tris"] == 0 and dev["report"].num_two_view_skipped == 10 == dev["report"].num_correspondences
    assert list(dev["pair_status"]) == [capi.PAIR_PROCESSED] and list(dev["re_num_trials"]) == [1]
    dev, exp = run(ctx, s, ignore_two_view_tracks=0)
    assert compare(dev, exp, clear_required=True)
    assert dev["report"].num_create_taken > 0 and dev["report"].num_two_view_skipped == 0


def test_ratio_gate(ctx):
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=1, unregistered=(7,), **CLEAR_SETS[0])
    dev, exp = run(ctx, s, re_min_ratio=0.0)
    assert compare(dev, exp, clear_required=True)
    assert set(dev["pair_status"]) == {capi.PAIR_NOT_UNDER_RECONSTRUCTED} and dev["num_tris"] == 0 and not dev["re_num_trials"].any()
    assert dev["report"].num_rounds == 0
    dev, exp = run(ctx, s, re_min_ratio=1.5)
    assert compare(dev, exp, clear_required=True)
    last = int(s["image_ids"][7])
    assert [int(v) for v in dev["pair_status"]] == [capi.PAIR_UNREGISTERED if last in (int(a), int(b)) else capi.PAIR_PROCESSED
                                                    for a, b in s["pairs"]]


def test_trials_persist_across_calls(ctx):
    """re_min_ratio 0.95: with a tenth of the matches wrong most pairs stay open after their trial"""
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=0, **CLEAR_SETS[0])
    first, exp = run(ctx, s, re_min_ratio=0.95)
    assert compare(first, exp, clear_required=True) and first["num_tris"] > 0
    folded = fold_dev(s, first)
    again, exp = run(ctx, folded, re_num_trials=first["re_num_trials"], re_min_ratio=0.95)
    assert compare(again, exp, clear_required=True)
    assert again["num_tris"] == 0 and (again["re_num_trials"] == first["re_num_trials"]).all()
    assert capi.PAIR_PROCESSED not in again["pair_status"] and capi.PAIR_TRIALS_EXHAUSTED in again["pair_status"]
    assert (again["pair_num_tri_corrs"] == first["pair_num_tri_corrs"]).all()
    twice, exp = run(ctx, folded, re_num_trials=first["re_num_trials"], re_min_ratio=0.95, re_max_trials=2)
    assert compare(twice, exp, clear_required=True)
    second = twice["pair_status"] == capi.PAIR_PROCESSED
    assert second.any() and (twice["re_num_trials"][second] == 2).all()
    assert (again["pair_status"][second] == capi.PAIR_TRIALS_EXHAUSTED).all()


def test_unregistered_image_counts_no_trial(ctx):
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=2, unregistered=(3,), **CLEAR_SETS[0])
    dev, exp = run(ctx, s)
    assert compare(dev, exp, clear_required=True)
    unreg = dev["pair_status"] == capi.PAIR_UNREGISTERED
    img = int(s["image_ids"][3])
    assert unreg.any() and not dev["re_num_trials"][unreg].any()
    assert all(img in (int(a), int(b)) for a, b in s["pairs"][unreg]) and img not in dev["touched_obs"][:, 0]
    # such a pair can still close: its features carry points already, and other pairs continue their partners onto them
    on_img = np.array([img in (int(a), int(b)) for a, b in s["pairs"]])
    assert capi.PAIR_CLOSED_BY_ITS_TURN in dev["pair_status"][on_img]


def test_bogus_camera_counts_the_trial_and_adds_nothing(ctx):
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=2, **CLEAR_SETS[0])
    s["cameras"] = [capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)]
    dev, exp = run(ctx, s)
    assert compare(dev, exp, clear_required=True)
    bogus = dev["pair_status"] == capi.PAIR_BOGUS_CAMERA
    assert bogus.any() and set(dev["pair_status"]) <= {capi.PAIR_BOGUS_CAMERA, capi.PAIR_NOT_UNDER_RECONSTRUCTED}
    assert (dev["re_num_trials"] == bogus).all() and dev["num_tris"] == 0 and len(dev["touched_obs"]) == 0
    s["cameras"] = [capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480), capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)]
    s["camera_ids"] = np.array([7, 8], np.uint32)
    s["image_camera_ids"] = np.where(np.arange(8) == 2, 8, 7).astype(np.uint32)  # one image on the bogus camera
    dev, exp = run(ctx, s)
    assert compare(dev, exp, clear_required=True)
    assert capi.PAIR_BOGUS_CAMERA in dev["pair_status"] and capi.PAIR_PROCESSED in dev["pair_status"] and dev["num_tris"] > 0


def gate_only_scene(seed):
    """Ten images, two of them unregistered and one on a bogus camera, 60 % of the points existing and then 35 % of the
    feature -> point links dropped anywhere in a track: pairs that are only gated share features with later candidates."""
    rng = np.random.default_rng(seed)
    unregistered = tuple(int(x) for x in rng.choice(10, 2, replace=False))
    s, _ = ref.make_scene(n_images=10, n_points=120, track=(3, 6), noise=0.3, wrong=0.1, existing=0.6, seed=seed,
                          unregistered=unregistered)
    s["cameras"] = [capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480), capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)]
    s["camera_ids"] = np.array([7, 8], np.uint32)
    s["image_camera_ids"] = np.where(np.arange(10) == int(rng.integers(0, 10)), 8, 7).astype(np.uint32)
    p3 = s["points2D_point3D"]
    s["points2D_point3D"] = np.where(rng.random(len(p3)) < 0.35, -1, p3).astype(np.int32)
    return s


@pytest.mark.parametrize("seed,pair,status", [(7, 25, ref.UNREGISTERED), (298, 17, ref.BOGUS_CAMERA), (361, 20, ref.BOGUS_CAMERA)])
def test_gate_only_pair_is_gated_before_later_candidates_write(ctx, seed, pair, status):
    """A pair that is only gated (unregistered image, bogus camera) whose round is set by one feature shares another with
    a sequentially later candidate.  If that candidate may run in an earlier round, it writes before the gate counts, and the
    pair reports "closed by its turn" (and, on a bogus camera, loses its counted trial) where the sequential loop finds it
    open.  The three scenes are those of seeds 0..599 on which a schedule without that order differs from the restatement;
    their smallest margins are 7.8e-2, 1.8e-1 and 6.9e-2."""
    s = gate_only_scene(seed)
    dev, exp = run(ctx, s)
    assert exp["pair_status"][pair] == status and exp["re_num_trials"][pair] == (status == ref.BOGUS_CAMERA)
    assert {status, ref.PROCESSED, ref.CLOSED_BY_ITS_TURN} <= set(exp["pair_status"])
    assert compare(dev, exp, clear_required=True)
    assert int(dev["pair_status"][pair]) == status


def test_one_correspondence_more_than_the_gate_block(ctx):
    n = GATE_BLOCK + 1
    s, _ = ref.make_scene(n_images=3, n_points=n, track=(3, 3), noise=0.3, wrong=0.0, existing=0.1, seed=9)
    dev, exp = run(ctx, s)
    assert list(dev["pair_num_total_corrs"]) == [n] * 3
    assert compare(dev, exp) and dev["report"].num_rounds == 3
    assert list(dev["pair_status"]) == [capi.PAIR_PROCESSED, capi.PAIR_PROCESSED, capi.PAIR_CLOSED_BY_ITS_TURN]


def test_duplicate_rule(ctx):
    """a match list that is not one-to-one: the later match of a repeated feature is dropped, on either side"""
    s, _ = ref.make_scene(noise=0.3, wrong=0.1, seed=3, **CLEAR_SETS[1])
    off = [int(x) for x in s["match_offsets"]]
    m = [s["matches"][off[k]:off[k + 1]] for k in range(len(off) - 1)]
    n2 = int(s["points2D_offsets"][2] - s["points2D_offsets"][1])
    extra = np.array([[m[0][0][0], (m[0][0][1] + 1) % n2], [m[0][3][0], m[0][5][1]], [m[0][2][0], m[0][2][1]]], np.uint32)
    m[0] = np.concatenate([m[0][:6], extra, m[0][6:]])
    s["matches"] = np.concatenate(m)
    s["match_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in m])]).astype(np.uint64)
    dev, exp = run(ctx, s)
    assert compare(dev, exp)
    assert dev["pair_num_total_corrs"][0] == len(m[0]) - 3


def same(a, b):
    for k in ("new_point_ids", "new_xyz", "new_track_obs", "continued_obs", "continued_point_ids", "touched_obs",
              "touched_point_ids", "pair_num_total_corrs", "pair_num_tri_corrs", "pair_status", "re_num_trials"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_byte_identical_repeats_shuffles_and_pair_order(ctx):
    rng = np.random.default_rng(13)
    s, _ = ref.make_scene(n_images=10, n_points=150, track=(3, 8), noise=0.3, wrong=0.1, existing=0.3, seed=13)
    base = ctx.retriangulate_pairs(s)
    assert base["report"].num_create_taken > 0 and base["report"].num_continue_taken > 0 and base["report"].num_rounds > 1
    same(base, ctx.retriangulate_pairs(s))
    same(base, ctx.retriangulate_pairs(shuffled(s, rng, matches=False)))
    same(base, ctx.retriangulate_pairs(shuffled(s, rng, points=False)))
    same(base, ctx.retriangulate_pairs(shuffled(s, rng)))
    t = dict(s, pairs=s["pairs"].copy(), matches=s["matches"].copy())
    off = s["match_offsets"]
    for k in range(0, len(s["pairs"]), 2):  # every other pair as (image2, image1) with its matches swapped
        t["pairs"][k] = s["pairs"][k][::-1]
        t["matches"][int(off[k]):int(off[k + 1])] = s["matches"][int(off[k]):int(off[k + 1]), ::-1]
    same(base, ctx.retriangulate_pairs(t))


def test_invalid_arguments(ctx):
    s, _ = ref.make_scene(n_images=4, n_points=30, track=(2, 4), noise=0.3, wrong=0.0, existing=0.3, seed=14)
    ctx.retriangulate_pairs(s)

    def bad(scene=s, trials=None, **opts):
        with pytest.raises(capi.DsmError):
            ctx.retriangulate_pairs(scene, capi.default_pair_retriangulation_options(**opts), re_num_trials=trials)

    for opts in ({"re_max_angle_error": 0.0}, {"re_max_angle_error": -1.0}, {"re_max_angle_error": np.nan},
                 {"re_max_angle_error": np.inf}, {"re_min_ratio": -0.1}, {"re_min_ratio": np.nan}, {"re_min_ratio": np.inf},
                 {"re_max_trials": -1}):
        bad(**opts)
    bad(max_transitivity=2)                                           # inherited: an option of the triangulation member
    p = s["pairs"].copy()
    p[1] = [p[1][0], p[1][0]]
    bad(dict(s, pairs=p))                                             # inherited: a self-pair
    m = s["matches"].copy()
    m[0, 0] = 10 ** 6
    bad(dict(s, matches=m))                                           # inherited: a match index out of range
    bad(trials=[0])                                                   # the binding: one counter per pair
    dev = ctx.retriangulate_pairs(s, capi.default_pair_retriangulation_options(re_max_trials=0))
    assert dev["num_tris"] == 0 and capi.PAIR_PROCESSED not in dev["pair_status"]  # 0 trials allowed: valid, nothing runs
    ctx.retriangulate_pairs(s)                                        # the context is still usable


def test_chain_retriangulate_pairs_bundle_adjust(ctx):
    """dsm_retriangulate over two images -> fold -> dsm_retriangulate_pairs -> fold -> dsm_bundle_adjust on one small scene.
    Twelve images with tracks of 3 to 5: the two separators reach only some of the pairs, so others are still open afterwards
    (with 8 images and tracks of 3 to 6 the first step closes every pair and the second has nothing to do)."""
    s, truth = ref.make_scene(n_images=12, n_points=160, track=(3, 5), noise=0.3, wrong=0.0, existing=0.4, seed=21)
    ids = [int(x) for x in s["image_ids"]]
    tri = ctx.retriangulate(s, ids[3:5])
    assert tri["report"].num_tris > 0
    s1 = ref.fold(s, triples(tri["touched_obs"], tri["touched_point_ids"]), tri["new_point_ids"], tri["new_xyz"])
    out = ctx.retriangulate_pairs(s1)
    assert out["report"].num_create_taken > 0 and out["report"].num_continue_taken > 0
    compare(out, ref.retriangulate_pairs(s1))
    assert int(out["new_point_ids"].min()) > int(s1["point3D_ids"].max())
    errs = [np.linalg.norm(x - truth[tuple(int(v) for v in t[0])]) for x, t in zip(out["new_xyz"], out["new_track_obs"])]
    assert np.median(errs) < 0.05
    s2 = fold_dev(s1, out)
    off, p3 = s2["points2D_offsets"], s2["points2D_point3D"]
    tracks = {}
    for i in range(len(ids)):
        for k in range(int(off[i + 1] - off[i])):
            if p3[off[i] + k] >= 0:
                tracks.setdefault(int(p3[off[i] + k]), []).append((i, k))
    pts = sorted(p for p in tracks if len(tracks[p]) >= 2)
    cam = s2["cameras"][0]
    ba_scene = dict(camera_model_ids=[cam.model_id], camera_params=list(cam.params)[:3], image_camera=np.zeros(len(ids)),
                    qvec=s2["qvec"], tvec=s2["tvec"], image_constant_pose=np.array([1, 1] + [0] * (len(ids) - 2)),
                    point_ids=s2["point3D_ids"][pts], xyz=s2["point3D_xyz"][pts],
                    track_offsets=np.concatenate([[0], np.cumsum([len(tracks[p]) for p in pts])]),
                    obs_image=[i for p in pts for i, _ in tracks[p]],
                    obs_xy=[s2["points2D_xy"][off[i] + k] for p in pts for i, k in tracks[p]])
    ba = ctx.bundle_adjust(ba_scene)
    assert ba["report"].termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE)
    assert math.isfinite(ba["report"].final_cost) and ba["report"].final_cost <= ba["report"].initial_cost
