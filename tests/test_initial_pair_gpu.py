"""dsm_find_initial_pairs on the device against the sequential restatement (tests/initial_pair_ref.py), on the
product and on the check build.

Parity: the pair found, the tried list, config, the inlier matches, the trial counts and E / F / H equal the restatement
exactly (they are the oracle's own output); qvec, tvec and tri_angle within the tolerance the project uses for poses against the
oracle (rtol 1e-6); the triangulation is compared on its own with the restatement fed the device's qvec / tvec: the same points
kept in the same order, xyz within RTOL = 1e-9 relative.  Every scene's acceptance margins are at least 1e-3 and its point
margins at least 1e-9 under the restatement: tests/test_initial_pair_cpu.py holds that without a GPU, so no case is skipped."""
import numpy as np
import pytest

from dagsfm_amd import capi, synthetic
from tests import initial_pair_ref as ref
from tests import initial_pair_scenes as scenes

pytestmark = pytest.mark.gpu
RTOL = 1e-9        # xyz, as the re-triangulation tests
POSE_RTOL = 1e-6   # qvec, tvec, tri_angle against the oracle (README)

_expected = {}


def expected(name, oracle):
    """The restatement's results of a named scene, computed once and left unchanged."""
    if name not in _expected:
        s, problems, kw = scenes.get(name)
        _expected[name] = ref.find_initial_pairs(s, problems, oracle, **kw)
    return _expected[name]


@pytest.fixture(scope="module", params=["product", "check"])
def ctx(request):
    return capi.Context(0, check=request.param == "check")


@pytest.fixture(scope="module")
def check_ctx():
    """A context of the check build for the serial cross-check (the binding forwards DSM_INITIAL_PAIR_SERIAL from the
    environment before every call, so the test sets it with monkeypatch after its last call on `ctx`)."""
    return capi.Context(0, check=True)


def compare(dev, exp, oracle):
    """One problem's device result against the restatement's."""
    assert dev["found"] == exp["found"]
    assert (dev["image_id1"], dev["image_id2"]) == (exp["image_id1"], exp["image_id2"])
    assert [tuple(int(x) for x in t) for t in dev["tried_pairs"]] == [tuple(t) for t in exp["tried"]]
    assert dev["num_tried"] == len(exp["tried"])
    g = dev["two_view_geometry"]
    if not exp["found"]:
        assert bytes(g) == bytes(capi.TwoViewGeometry()) and len(dev["new_xyz"]) == 0 and len(dev["inlier_matches"]) == 0
        return
    e = exp["estimate"]
    t = e["tvg"]
    assert g.config == e["config"] and g.num_inliers == len(e["inliers"]) and g.num_matches == len(e["matches"])
    assert (dev["inlier_matches"] == e["inliers"]).all()
    assert list(g.E) == list(t.E) and list(g.F) == list(t.F) and list(g.H) == list(t.H)
    assert list(g.num_trials) == list(t.num_trials)
    assert np.allclose(list(g.qvec), e["qvec"], rtol=POSE_RTOL, atol=1e-12) and np.allclose(list(g.tvec), e["tvec"], rtol=POSE_RTOL, atol=1e-12)
    assert np.isclose(g.tri_angle, e["tri_angle"], rtol=POSE_RTOL, atol=1e-12)
    # the triangulation on its own: the restatement on the device's pose
    pts = ref.triangulate(exp["view"], exp["options"], exp["image_id1"], exp["image_id2"], list(g.qvec), list(g.tvec), oracle, ref.Margins())
    obs = dev["new_track_obs"]
    assert [(int(o[0, 1]), int(o[1, 1])) for o in obs] == [(a, b) for _, a, b in pts]
    assert all(int(o[0, 0]) == exp["image_id1"] and int(o[1, 0]) == exp["image_id2"] for o in obs)
    if pts:
        want = np.array([x for x, _, _ in pts])
        assert (np.abs(dev["new_xyz"] - want) <= RTOL * np.maximum(np.abs(want), 1.0)).all()


def run(ctx, name, oracle, **kw):
    s, problems, okw = scenes.get(name)
    out = ctx.find_initial_pairs(s, problems, **dict(okw, **kw))
    exp = expected(name, oracle)
    assert len(out["results"]) == len(exp)
    for d, e in zip(out["results"], exp):
        compare(d, e, oracle)
    return out


def test_first_candidate_success_on_a_ring(ctx, oracle):
    out = run(ctx, "ring", oracle)
    r, rep = out["results"][0], out["report"]
    assert r["found"] and r["num_tried"] == 1 and rep.num_rounds == 1
    assert rep.num_verified - rep.num_speculated == 1
    m = expected("ring", oracle)[0]["margins"]
    assert np.isclose(rep.min_tri_angle_margin, m.tri_angle, rtol=1e-3) and np.isclose(rep.min_forward_motion_margin, m.forward, rtol=1e-3)
    assert np.isclose(rep.min_point_angle_margin, m.point_angle, rtol=1e-3) and np.isclose(rep.min_point_depth_margin, m.point_depth, rtol=1e-3)
    assert rep.device_ms > 0 and rep.verify_ms > 0


def test_rejection_by_forward_motion(ctx, oracle):
    out = run(ctx, "forward_motion", oracle)
    assert out["results"][0]["num_tried"] == 2 and out["report"].min_forward_motion_margin < 0.06


def test_rejection_by_tri_angle_success_at_the_sixth(ctx, oracle):
    out = run(ctx, "small_baseline", oracle)
    assert out["results"][0]["found"] and out["results"][0]["num_tried"] == 6


def test_planar_scene_pose_from_H(ctx, oracle):
    out = run(ctx, "planar", oracle)
    assert out["results"][0]["two_view_geometry"].config == 4


def test_pure_rotation_is_rejected(ctx, oracle):
    out = run(ctx, "pure_rotation", oracle)
    assert not out["results"][0]["found"] and out["results"][0]["image_id1"] == capi.NO_IMAGE


def test_watermark_pair_is_rejected_by_configuration(ctx, oracle):
    out = run(ctx, "watermark", oracle)
    assert out["results"][0]["num_tried"] == 2


def test_no_pair_found_tries_the_whole_list(ctx, oracle):
    out = run(ctx, "nothing_found", oracle)
    s, problems, kw = scenes.get("nothing_found")
    r = out["results"][0]
    assert not r["found"] and [tuple(int(x) for x in t) for t in r["tried_pairs"]] == [tuple(t) for t in ref.candidate_order(s, problems[0], **kw)]
    assert out["report"].num_candidates == 6 and out["report"].num_speculated == 0


def result_bytes(out):
    return [(r["found"], r["image_id1"], r["image_id2"], bytes(r["two_view_geometry"]), r["inlier_matches"].tobytes(), r["num_tried"],
             r["tried_pairs"].tobytes(), r["new_xyz"].tobytes(), r["new_track_obs"].tobytes()) for r in out["results"]]


def test_windowing_changes_no_byte(ctx, check_ctx, oracle, monkeypatch):
    """Success at the sixth candidate with windows of 1, 2, 4 and 64 and with the serial cross-check: identical bytes."""
    outs = {w: run(ctx, "small_baseline", oracle, speculation_window=w) for w in (1, 2, 4, 64)}
    first = result_bytes(outs[1])
    for w, out in outs.items():
        assert result_bytes(out) == first, w
        assert out["results"][0]["num_tried"] == 6
        rep = out["report"]
        assert rep.num_rounds == -(-6 // w) and rep.num_verified == min(rep.num_rounds * w, 6) and rep.num_speculated == rep.num_verified - 6
        assert rep.min_tri_angle_margin == outs[1]["report"].min_tri_angle_margin
    others = {name: result_bytes(run(ctx, name, oracle)) for name in ("batching", "triangulation_257", "duplicates", "camera_models")}
    monkeypatch.setenv("DSM_INITIAL_PAIR_SERIAL", "1")  # from here on only the check build's context is called
    ser = run(check_ctx, "small_baseline", oracle, speculation_window=64)
    assert result_bytes(ser) == first and ser["report"].num_rounds == 6 and ser["report"].num_speculated == 0
    for name, want in others.items():
        assert result_bytes(run(check_ctx, name, oracle)) == want, name


def test_batching_equals_single_problem_calls(ctx, oracle):
    out = run(ctx, "batching", oracle)
    s, problems, kw = scenes.get("batching")
    singles = [ctx.find_initial_pairs(s, [p], **kw) for p in problems]
    assert result_bytes(out) == [result_bytes(x)[0] for x in singles]
    ctx.set_memory_budget(20000)  # every problem its own batch: the same bytes
    try:
        cut = ctx.find_initial_pairs(s, problems, **kw)
    finally:
        ctx.set_memory_budget(0)
    assert result_bytes(cut) == result_bytes(out) and cut["report"].num_batches == 3 and out["report"].num_batches == 1
    assert result_bytes(ctx.find_initial_pairs(s, problems[::-1], **kw)) == result_bytes(out)[::-1]


def test_duplicates_across_the_count_threshold(ctx, oracle):
    out = run(ctx, "duplicates", oracle)
    s, problems, kw = scenes.get("duplicates")
    lists, kept = capi.initial_pair_host_candidates(s, problems, capi.default_initial_pair_options(**kw))
    assert list(kept) == [29, 60, 50] and list(np.diff(np.asarray(s["match_offsets"], np.int64))) == [69, 63, 50]
    assert out["report"].num_candidates == len(lists[0]) == 2


def test_opencv_and_fisheye_cameras(ctx, oracle):
    run(ctx, "camera_models", oracle)


@pytest.mark.parametrize("n", [63, 64, 65, 257])
def test_triangulation_wave_and_block_edges(ctx, oracle, n):
    out = run(ctx, "triangulation_%d" % n, oracle)
    r = out["results"][0]
    assert r["found"] and r["two_view_geometry"].num_matches == n and 0 < len(r["new_xyz"]) < n
    assert (r["image_id1"], r["image_id2"]) == tuple(int(x) for x in scenes.get("triangulation_%d" % n)[0]["image_ids"][::-1])


def test_invalid_arguments_leave_the_context_usable(ctx, oracle):
    s, problems, kw = scenes.get("ring")
    ids = [int(x) for x in s["image_ids"]]
    bad_problems = [dict(image_ids=ids + [999]), dict(image_ids=ids + ids[:1]), dict(image_ids=ids[:3], seed_image1=ids[4]),
                    dict(image_ids=ids, seed_image1=ids[0], seed_image2=ids[0]), dict(image_ids=ids, num_registrations=[0])]
    for p in bad_problems:
        with pytest.raises(capi.DsmError):
            ctx.find_initial_pairs(s, [p], **kw)
    for okw in (dict(init_min_num_inliers=-1), dict(init_max_reg_trials=0), dict(init_max_error=-1.0), dict(init_max_forward_motion=2.0),
                dict(init_min_tri_angle=float("nan")), dict(speculation_window=0)):
        with pytest.raises(capi.DsmError, match="dsm error -?%d" % abs(capi_invalid())):
            ctx.find_initial_pairs(s, problems, **dict(kw, **okw))
    for key, value in (("pairs", np.array([[ids[0], ids[0]]] * len(s["pairs"]), np.uint32)), ("image_camera_ids", np.full(len(ids), 77, np.uint32)),
                       ("matches", np.full_like(s["matches"], 100000))):
        with pytest.raises(capi.DsmError):
            ctx.find_initial_pairs(dict(s, **{key: value}), problems, **kw)
    run(ctx, "ring", oracle)


def capi_invalid():
    return 1  # DSM_ERR_INVALID_ARGUMENT (include/dagsfm_mi355x.h)


def test_verify_pairs_results_are_undisturbed(ctx, oracle):
    scene = synthetic.Scene(3, 256, seed=5)
    ims = [scene.image(i) for i in range(3)]
    cams = [capi.simple_pinhole(800.0, 500.0, 375.0, 1000, 750, True) for _ in range(3)]
    ctx.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
    ctx.match_pairs(synthetic.exhaustive_pairs(3))
    ctx.verify_pairs(capi.default_two_view_options(), user_seed=7, stage_filter=False)
    before = [bytes(g) for g in ctx.two_view_geometries()]
    ioffs, inl = ctx.inlier_matches()
    run(ctx, "ring", oracle)
    assert [bytes(g) for g in ctx.two_view_geometries()] == before
    ioffs2, inl2 = ctx.inlier_matches()
    assert (ioffs2 == ioffs).all() and (inl2 == inl).all()
