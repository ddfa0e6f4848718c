"""dsm_bundle_adjust on the device against the numpy restatement (tests/bundle_adjustment_ref.py), DESIGN.md 12."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import bundle_adjustment_ref as ref

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def run(ctx, scene, **kw):
    o = capi.default_bundle_adjustment_options(**kw)
    return ctx.bundle_adjust(scene, o)


def clear(rep):
    return min(rep["min_rho_margin"], rep["min_cg_margin"], rep["min_gradient_margin"]) >= MARGIN


def compare(dev, rr, scene):
    """Identity of every decision and agreement of the values, where the restatement's margins are clear."""
    d, r = dev["report"], rr["report"]
    tr_d, tr_r = dev["trace"], rr["trace"]
    assert d.termination == r["termination"]
    assert d.num_iterations == r["num_iterations"] and d.num_successful_steps == r["num_successful_steps"]
    assert list(tr_d[1:, 4].astype(int)) == rr["accepted"]
    assert list(tr_d[1:, 3].astype(int)) == rr["cg_iterations"]
    assert d.total_cg_iterations == r["total_cg_iterations"]
    assert d.num_effective_parameters == r["num_effective_parameters"] and d.num_residuals == r["num_residuals"]
    np.testing.assert_allclose(tr_d[:, 0], tr_r[:, 0], rtol=1e-9)
    np.testing.assert_allclose(d.initial_cost, r["initial_cost"], rtol=1e-12)
    scale = max(1.0, float(np.abs(scene["xyz"]).max()))
    np.testing.assert_allclose(dev["xyz"], rr["xyz"], rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(dev["tvec"], rr["tvec"], rtol=0, atol=1e-7 * scale)
    np.testing.assert_allclose(dev["qvec"], rr["qvec"], rtol=0, atol=1e-7)
    # focal lengths and principal points relative, the dimensionless distortion coefficients against 1
    np.testing.assert_allclose(dev["camera_params"], rr["camera_params"], rtol=1e-7, atol=1e-7)


def check_against_ref(ctx, scene, **kw):
    dev = run(ctx, scene, **kw)
    rr = ref.bundle_adjust(scene, kw)
    if clear(rr["report"]) and ref.stable_under_rounding(scene, kw, rr):
        compare(dev, rr, scene)
        return True
    # where rounding decides the trajectory, the run still ends the same way and near the same cost
    assert dev["report"].termination == rr["report"]["termination"]
    np.testing.assert_allclose(dev["report"].final_cost, rr["report"]["final_cost"], rtol=1e-4)
    return False


def scenes():
    out = []
    for m in range(11):  # every camera model, shared and per-image cameras
        out.append(("model%d_shared" % m, ref.make_scene(100 + m, models=(m,), n_points=300), {}))
        out.append(("model%d_per_image" % m, ref.make_scene(200 + m, models=(m, (m + 3) % 11), shared=False, n_points=300, arc=1.5),
                    dict(max_num_iterations=5, refine_extra_params=0)))  # per-image distortion is ill-posed here
    out.append(("mixed_constant_points", ref.make_scene(301, n_points=80, const_point_frac=0.3), {}))
    out.append(("no_gauge", ref.make_scene(302, gauge=False), {}))
    for f in (0, 1):
        for pp in (0, 1):
            for ex in (0, 1):
                out.append(("refine_%d%d%d" % (f, pp, ex), ref.make_scene(310 + 4 * f + 2 * pp + ex, models=(4,), n_points=150),
                            dict(refine_focal_length=f, refine_principal_point=pp, refine_extra_params=ex)))
    return out


SCENES = scenes()


def test_device_matches_restatement_per_iteration(ctx):
    clear_runs = 0
    for name, scene, kw in SCENES:
        kw = dict(dict(max_num_iterations=10), **kw)
        if check_against_ref(ctx, scene, **kw):
            clear_runs += 1
    assert clear_runs >= 0.9 * len(SCENES), "%d of %d runs clear of the margin" % (clear_runs, len(SCENES))


def test_no_f_blocks_back_substitution_only(ctx):
    scene = ref.make_scene(400, n_points=40)
    scene["image_constant_pose"][:] = 1
    kw = dict(refine_focal_length=0, refine_principal_point=0, refine_extra_params=0)
    dev = run(ctx, scene, **kw)
    rr = ref.bundle_adjust(scene, kw)
    assert dev["report"].total_cg_iterations == 0
    assert clear(rr["report"])
    compare(dev, rr, scene)


def test_long_tracks_and_a_camera_shared_by_many_observations(ctx):
    # 300 images, every point seen by 260..300 of them: tracks past 256, one camera with > 65 536 observations
    scene = ref.make_scene(401, n_images=300, n_points=240, min_track=260, max_track=300, noise=0.3)
    assert len(scene["obs_image"]) > 65536
    kw = dict(max_num_iterations=6)
    dev = run(ctx, scene, **kw)
    rr = ref.bundle_adjust(scene, kw)
    assert clear(rr["report"])
    compare(dev, rr, scene)


def test_noise_free_recovery(ctx):
    scene = ref.make_scene(402, n_points=100, noise=0.0)
    dev = run(ctx, scene, gradient_tolerance=1e-12, max_num_iterations=200, max_linear_solver_iterations=500)
    rep = dev["report"]
    r = ref.Problem(scene, dict(refine_focal_length=1, refine_principal_point=0, refine_extra_params=1)).residuals(
        {"qvec": dev["qvec"], "tvec": dev["tvec"], "xyz": dev["xyz"], "camera_params": dev["camera_params"]})
    assert np.sqrt((r * r).sum(1).mean()) < 1e-6, rep.as_dict()


def test_noisy_run_reaches_the_restatement_optimum(ctx):
    scene = ref.make_scene(403, n_points=80, noise=0.5)
    kw = dict(gradient_tolerance=1e-10, max_num_iterations=200, max_linear_solver_iterations=500)
    dev = run(ctx, scene, **kw)
    np.testing.assert_allclose(dev["report"].final_cost, ref.scipy_optimum(scene, {}), rtol=1e-6)


def test_constants_stay_bit_identical(ctx):
    scene = ref.make_scene(404, n_points=80, const_point_frac=0.3)
    scene["image_constant_tvec"][2] = 5
    dev = run(ctx, scene, gradient_tolerance=1e-6)
    assert dev["report"].num_successful_steps > 0
    assert (dev["qvec"][0].tobytes() == (scene["qvec"][0] / np.linalg.norm(scene["qvec"][0])).tobytes())
    assert dev["tvec"][0].tobytes() == scene["tvec"][0].tobytes()
    assert dev["tvec"][1, 0] == scene["tvec"][1, 0] and dev["tvec"][2, 0] == scene["tvec"][2, 0] and dev["tvec"][2, 2] == scene["tvec"][2, 2]
    assert dev["tvec"][1, 1] != scene["tvec"][1, 1]
    pc = scene["point_constant"].astype(bool)
    assert pc.any() and dev["xyz"][pc].tobytes() == scene["xyz"][pc].tobytes()
    assert (dev["xyz"][~pc] != scene["xyz"][~pc]).all()
    assert dev["camera_params"][1:3].tobytes() == scene["camera_params"][1:3].tobytes()  # principal point
    assert dev["camera_params"][0] != scene["camera_params"][0]


def test_unobserved_images_and_cameras_come_back_unchanged(ctx):
    scene = ref.make_scene(405, n_points=50)
    scene["camera_model_ids"] = np.concatenate([scene["camera_model_ids"], [0]]).astype(np.int32)
    scene["camera_params"] = np.concatenate([scene["camera_params"], [300.0, 1.0, 2.0]])
    scene["image_camera"] = np.concatenate([scene["image_camera"], [1]]).astype(np.uint32)
    scene["qvec"] = np.vstack([scene["qvec"], [[2.0, 0.0, 0.0, 0.0]]])
    scene["tvec"] = np.vstack([scene["tvec"], [[1.0, 2.0, 3.0]]])
    scene["image_constant_pose"] = np.concatenate([scene["image_constant_pose"], [0]]).astype(np.uint8)
    scene["image_constant_tvec"] = np.concatenate([scene["image_constant_tvec"], [0]]).astype(np.uint8)
    dev = run(ctx, scene)
    assert list(dev["qvec"][-1]) == [2.0, 0.0, 0.0, 0.0] and list(dev["tvec"][-1]) == [1.0, 2.0, 3.0]
    assert list(dev["camera_params"][-3:]) == [300.0, 1.0, 2.0]


def shuffled(scene, seed):
    rng = np.random.default_rng(seed)
    toff = scene["track_offsets"]
    P = len(toff) - 1
    perm = rng.permutation(P)
    offs, oi, ox = [0], [], []
    for p in perm:
        a, b = toff[p], toff[p + 1]
        k = rng.permutation(b - a) + a
        oi.extend(scene["obs_image"][k])
        ox.extend(scene["obs_xy"][k])
        offs.append(len(oi))
    out = dict(scene)
    out.update(point_ids=scene["point_ids"][perm], xyz=scene["xyz"][perm], point_constant=scene["point_constant"][perm],
               track_offsets=np.array(offs, np.uint32), obs_image=np.array(oi, np.uint32), obs_xy=np.array(ox))
    return out, perm


def test_deterministic_across_repeats_and_shuffles(ctx):
    scene = ref.make_scene(406, n_points=120, models=(3,), const_point_frac=0.1)
    a = run(ctx, scene, gradient_tolerance=1e-6)
    b = run(ctx, scene, gradient_tolerance=1e-6)
    for k in ("xyz", "qvec", "tvec", "camera_params", "trace"):
        assert a[k].tobytes() == b[k].tobytes()
    for seed in (1, 2):
        sc, perm = shuffled(scene, seed)
        c = run(ctx, sc, gradient_tolerance=1e-6)
        assert c["xyz"].tobytes() == a["xyz"][perm].tobytes()
        for k in ("qvec", "tvec", "camera_params", "trace"):
            assert c[k].tobytes() == a[k].tobytes()


def test_iteration_cap_and_convergence_at_iteration_zero(ctx):
    scene = ref.make_scene(407)
    dev = run(ctx, scene, max_num_iterations=3, gradient_tolerance=0.0)
    assert dev["report"].termination == capi.BA_NO_CONVERGENCE and dev["report"].num_iterations == 3
    assert dev["trace"].shape == (4, capi.BA_TRACE_COLUMNS)
    dev0 = run(ctx, scene, gradient_tolerance=1e30)
    rep = dev0["report"]
    assert rep.termination == capi.BA_CONVERGENCE and rep.num_iterations == 0
    qn = scene["qvec"] / np.linalg.norm(scene["qvec"], axis=1, keepdims=True)
    assert dev0["qvec"].tobytes() == qn.tobytes()
    assert dev0["xyz"].tobytes() == np.asarray(scene["xyz"], np.float64).tobytes()
    assert dev0["camera_params"].tobytes() == scene["camera_params"].tobytes()


def test_argument_errors(ctx):
    base = ref.make_scene(408, n_points=20)

    def bad(**chg):
        sc = {k: np.array(v, copy=True) for k, v in base.items()}
        sc.update(chg)
        return sc

    cases = [
        bad(camera_model_ids=np.array([11], np.int32)),
        bad(image_camera=np.array([0, 0, 0, 0, 0, 5], np.uint32)),
        bad(obs_image=np.where(np.arange(len(base["obs_image"])) == 0, 99, base["obs_image"]).astype(np.uint32)),
        bad(point_ids=np.where(np.arange(20) == 1, base["point_ids"][0], base["point_ids"]).astype(np.uint64)),
        bad(xyz=np.where(np.arange(60).reshape(20, 3) == 4, np.nan, base["xyz"])),
        bad(qvec=np.where(np.arange(24).reshape(6, 4) // 4 == 2, 0.0, base["qvec"])),
        bad(image_constant_tvec=np.array([0, 8, 0, 0, 0, 0], np.uint8)),
    ]
    toff = base["track_offsets"].copy()
    short = bad(track_offsets=np.concatenate([[0, 1], toff[2:]]).astype(np.uint32))
    short["track_offsets"][1] = 1  # a track of one element and one of the rest
    cases.append(short)
    dup = bad()
    a = int(toff[0])
    dup["obs_image"][a + 1] = dup["obs_image"][a]
    cases.append(dup)
    empty = bad(point_ids=np.zeros(0, np.uint64), xyz=np.zeros((0, 3)), point_constant=np.zeros(0, np.uint8),
                track_offsets=np.zeros(1, np.uint32), obs_image=np.zeros(0, np.uint32), obs_xy=np.zeros((0, 2)))
    cases.append(empty)
    # track_offsets not starting at 0 (a slice of a larger CSR), and offsets whose "+ 2" wraps in 32 bits
    shifted = bad(track_offsets=(toff + 1).astype(np.uint32), obs_image=np.concatenate([[0], base["obs_image"]]).astype(np.uint32),
                  obs_xy=np.vstack([[[0.0, 0.0]], base["obs_xy"]]))
    cases.append(shifted)
    wrap = bad(point_ids=base["point_ids"][:2], xyz=base["xyz"][:2], point_constant=base["point_constant"][:2],
               track_offsets=np.array([0, 0xFFFFFFFF, 5], np.uint32), obs_image=base["obs_image"][:5], obs_xy=base["obs_xy"][:5])
    cases.append(wrap)
    for sc in cases:
        with pytest.raises(capi.DsmError, match="dsm error 1"):
            run(ctx, sc)
    for kw in (dict(max_num_iterations=-1), dict(max_linear_solver_iterations=0), dict(gradient_tolerance=-1.0),
               dict(function_tolerance=float("nan")), dict(parameter_tolerance=float("inf")), dict(max_num_consecutive_invalid_steps=-1)):
        with pytest.raises(capi.DsmError, match="dsm error 1"):
            run(ctx, base, **kw)
