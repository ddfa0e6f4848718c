"""GPU: dsm_refine_absolute_poses against the sequential restatement (tests/pose_refinement_ref.py), DESIGN.md 15.

Comparison rule: a problem that is clear (every margin of the restatement >= 1e-9 and its conditioning probe stable)
agrees in termination, iteration count, the accepted / rejected sequence, success, and in the costs, qvec, tvec and camera
parameters within REFINE_TOLERANCE; the others agree on success and on the final cost within HAND_COST_TOLERANCE of the initial
cost.  Clear is decided by the restatement alone.  Both tolerances are measured on the restatement (tests/pose_refinement_scenes.py, re-measured by the CPU test)."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import pose_refinement_ref as ref
from tests import pose_refinement_scenes as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def run(ctx, problems, options=None):
    return ctx.refine_absolute_poses(options=options, **sc.batch(problems))


def close(a, b, what, tol=sc.REFINE_TOLERANCE):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    scale = max(float(np.max(np.abs(b))), 1e-300)
    err = float(np.max(np.abs(a - b))) / scale
    print("   ", what, "%.2e" % err)
    assert err <= tol, (what, err)


def compare(res, steps, margins, p, want, index, options=None, exact_data=False):
    """One problem against the restatement; returns whether it is clear.  Clear is the restatement's verdict alone (margins and
    the conditioning probe); on a clear problem the device's own margins must be clear too.  exact_data: a hand problem, whose
    final cost is compared against the initial cost (HAND_COST_TOLERANCE) because it is orders below it."""
    clear = ref.is_clear(want["margins"]) and ref.stable_under_rounding(sc.args(p), options, want)
    print(index, "device", res.termination, res.num_iterations, list(steps), "%.6g -> %.6g" % (res.initial_cost, res.final_cost),
          "ref", want["termination"], want["num_iterations"], want["steps"], "%.6g -> %.6g" % (want["initial_cost"], want["final_cost"]),
          "margins %.1e %.1e" % (min(margins), min(want["margins"])), "clear", clear)
    assert bool(res.success) == want["success"], index
    assert res.num_residual_blocks == want["num_residual_blocks"], index
    hand_err = abs(res.final_cost - want["final_cost"]) / max(want["initial_cost"], 1e-300)
    if clear:
        assert ref.is_clear(list(margins)), (index, list(margins))
        assert res.termination == want["termination"] and res.num_iterations == want["num_iterations"], index
        assert list(steps) == want["steps"], index
        assert res.num_successful_steps == want["num_successful_steps"] and res.num_invalid_steps == want["num_invalid_steps"], index
        close([res.initial_cost], [want["initial_cost"]], "initial cost %s" % index)
        close(list(res.qvec), want["qvec"], "qvec %s" % index)
        close(list(res.tvec), want["tvec"], "tvec %s" % index)
        close(list(res.camera_params), want["camera_params"], "camera %s" % index)
        if not exact_data:
            close([res.final_cost], [want["final_cost"]], "final cost %s" % index)
    if exact_data or not clear:
        print("    final cost over initial cost", "%.2e" % hand_err)
        assert hand_err <= sc.HAND_COST_TOLERANCE, (index, hand_err)
    return clear


def test_grid_against_the_restatement(ctx):
    grid = sc.grid()
    out = run(ctx, grid)
    clear = 0
    for b, p in enumerate(grid):
        want = ref.refine(*sc.args(p))
        clear += compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, b)
        assert out["results"][b].success and out["results"][b].final_cost < out["results"][b].initial_cost
    rep = out["report"]
    print("clear on both sides %d of %d; iterations %d; solve %.3f ms, device %.3f ms" %
          (clear, len(grid), rep.num_iterations, rep.solve_ms, rep.device_ms))
    assert clear >= 0.9 * len(grid)
    assert rep.num_problems == len(grid) and rep.num_iterations == sum(r.num_iterations for r in out["results"])
    assert list(rep.min_margin) == list(out["margins"].min(axis=0))


def test_tight_gradient_tolerance_runs_to_the_function_tolerance(ctx):
    grid = sc.grid()[::4]
    o = capi.default_pose_refinement_options(gradient_tolerance=1e-10)
    out = run(ctx, grid, o)
    for b, p in enumerate(grid):
        want = ref.refine(*sc.args(p), opts=dict(gradient_tolerance=1e-10))
        compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, b, dict(gradient_tolerance=1e-10))
        assert out["steps"][b][-1] == capi.POSE_STEP_TOLERANCE


def result_bytes(out, b):
    return bytes(out["results"][b]) + out["margins"][b].tobytes() + out["steps"][b].tobytes()


def test_batch_composition_does_not_change_a_result(ctx):
    grid = sc.grid()
    grid = grid[:8] + grid[20:30]
    base = run(ctx, grid)
    again = run(ctx, grid)
    for b in range(len(grid)):
        assert result_bytes(base, b) == result_bytes(again, b), b
    order = [9, 3, 17, 0, 3, 12, 5, 11, 0]
    shuffled = run(ctx, [grid[i] for i in order])
    for k, i in enumerate(order):
        assert result_bytes(shuffled, k) == result_bytes(base, i), (k, i)
    for i in (2, 14):
        alone = run(ctx, [grid[i]])
        assert result_bytes(alone, 0) == result_bytes(base, i), i


def test_small_rank_deficient_and_empty_problems_terminate(ctx):
    hand = sc.hand_problems()
    names = sorted(hand)
    out = run(ctx, [hand[k] for k in names])
    for b, k in enumerate(names):
        res = out["results"][b]
        want = ref.refine(*sc.args(hand[k]))
        compare(res, out["steps"][b], out["margins"][b], hand[k], want, k, exact_data=True)
        assert res.num_iterations <= 100 and res.termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE, capi.BA_FAILURE)
        assert np.isfinite(res.final_cost) and res.final_cost <= res.initial_cost
    # zero inliers: the input bits, qvec not normalised
    p = dict(hand["n0"], qvec=np.array(hand["n0"]["qvec"]) * 1.7, flags=3)
    res = run(ctx, [p])["results"][0]
    assert res.success and res.termination == capi.BA_CONVERGENCE and res.num_iterations == 0 and res.num_residual_blocks == 0
    assert np.array(list(res.qvec)).tobytes() == p["qvec"].tobytes() and np.array(list(res.tvec)).tobytes() == np.asarray(p["tvec"]).tobytes()
    assert list(res.camera_params) == list(p["cam"].params) and res.initial_cost == 0.0 and res.final_cost == 0.0
    # the iteration cap: 0 and 2 iterations end NO_CONVERGENCE and usable
    g = sc.grid()[2]
    for cap in (0, 2):
        r = run(ctx, [g], capi.default_pose_refinement_options(max_num_iterations=cap))["results"][0]
        assert r.success and r.termination == capi.BA_NO_CONVERGENCE and r.num_iterations == cap
        assert abs(np.linalg.norm(list(r.qvec)) - 1.0) < 1e-15


def test_argument_errors(ctx):
    good = sc.grid()[0]

    def fails(problems=None, options=None, text="", **replace):
        kw = sc.batch(problems or [good])
        kw.update(replace)
        with pytest.raises(capi.DsmError) as e:
            ctx.refine_absolute_poses(options=options, **kw)
        assert "dsm error 1" in str(e.value) and "dsm_refine_absolute_poses" in str(e.value) and text in str(e.value), str(e.value)
    for key, text in (("xy", "non-finite points2D"), ("X", "non-finite points3D"), ("qvec", "non-finite qvec"), ("tvec", "non-finite tvec")):
        bad = dict(good, **{key: np.array(good[key], np.float64)})
        bad[key].reshape(-1)[1] = np.nan
        fails([bad], text=text)
    cam = capi.Camera.from_buffer_copy(bytes(good["cam"]))
    cam.model_id = 11
    fails([dict(good, cam=cam)], text="unknown camera model")
    cam = capi.Camera.from_buffer_copy(bytes(sc.grid()[2]["cam"]))
    cam.params[3] = np.inf
    fails([dict(sc.grid()[2], cam=cam)], text="non-finite camera")
    n = len(good["xy"])
    fails([good], text="start at 0", offsets=np.array([1, n], np.uint64))
    fails([good, good], text="ascend", offsets=np.array([0, n + 5, n], np.uint64))
    fails([dict(good, flags=4)], text="refine_flags")
    d = capi.default_pose_refinement_options
    for kw in (dict(gradient_tolerance=-1.0), dict(gradient_tolerance=np.nan), dict(max_num_iterations=-1), dict(loss_function_scale=-1.0),
               dict(loss_function_scale=np.inf)):
        fails(options=d(**kw), text="option out of range")
    fails(options=d(loss_function_scale=0.0), text="loss_function_scale = 0")
    fails(options=d(max_num_iterations=capi.POSE_REFINEMENT_MAX_ITERATIONS + 1), text="max_num_iterations above 1000")
    o = d()
    assert (o.gradient_tolerance, o.loss_function_scale, o.max_num_iterations) == (1.0, 1.0, 100)  # pose.h:82-88
    L = capi.lib()
    res = capi.PoseRefinementResult()
    offs = np.array([0, n], np.uint64)
    rc = L.dsm_refine_absolute_poses(ctx._h, 1, None, offs.ctypes.data, None, None, None, None, None, None, None, ctypes.addressof(res),
                                     None, None, None)
    assert rc == 1 and b"NULL" in L.dsm_last_error(ctx._h)
    out = run(ctx, [])  # an empty batch is not an error
    assert out["results"] == [] and out["report"].num_problems == 0


def test_chain_estimate_refine_retriangulate_bundle_adjust(ctx):
    """The chain of section 14 with the refinement in its place: dsm_estimate_absolute_poses -> dsm_refine_absolute_poses ->
    dsm_retriangulate -> dsm_bundle_adjust.  The refined poses have a Cauchy cost no higher than the estimates'; on the noise-free
    scene they sit closer to the planted poses."""
    from tests import absolute_pose_scenes as scenes
    from tests import retriangulation_ref as rt
    for noise in (0.3, 0.0):
        s, truth = rt.make_scene(n_images=8, n_points=500, track=(3, 6), noise=noise, wrong=0.0, existing=0.6, seed=31)
        ids = [int(x) for x in s["image_ids"]]
        off, p3 = s["points2D_offsets"], s["points2D_point3D"]
        rows = [np.nonzero(p3[off[i]:off[i + 1]] >= 0)[0] for i in range(len(ids))]
        cams = [s["cameras"][0]] * len(ids)
        offs = np.concatenate([[0], np.cumsum([len(k) for k in rows])]).astype(np.uint64)
        xy = np.concatenate([s["points2D_xy"][off[i] + k] for i, k in enumerate(rows)])
        X = np.concatenate([s["point3D_xyz"][p3[off[i] + k]] for i, k in enumerate(rows)])
        if noise == 0.0:
            # make_scene moves the existing points by 1e-3 whatever `noise` is, so its noise = 0 scene is not exact: take the points
            # as they are and observe them through the planted poses, then (xy, X) and the planted poses agree to rounding
            cam0 = s["cameras"][0]
            for i in range(len(ids)):
                P = np.array(rt.pose_matrix(s["qvec"][i], s["tvec"][i])[0]).reshape(3, 4)
                sl = slice(int(offs[i]), int(offs[i + 1]))
                pc = X[sl] @ P[:, :3].T + P[:, 3]
                xy[sl] = np.stack([cam0.params[0] * pc[:, 0] / pc[:, 2] + cam0.params[1], cam0.params[0] * pc[:, 1] / pc[:, 2] + cam0.params[2]], axis=1)
        reg = ctx.register_images(cams, offs, xy, X, estimate_focal_length=[0] * len(ids), refine_flags=[0] * len(ids))
        enough = [len(k) >= 30 for k in rows]
        assert sum(enough) >= 6 and all(enough[3:5]) and list(reg["registered"]) == enough
        qvec, tvec = np.array(s["qvec"], np.float64), np.array(s["tvec"], np.float64)
        for i in range(len(ids)):
            if not enough[i]:
                assert reg["refined_index"][i] == -1
                continue
            e = reg["estimate"]["results"][i]
            sl = slice(int(offs[i]), int(offs[i + 1]))
            mask = reg["inlier_mask"][sl]
            before = ref.cauchy_cost(cams[i], xy[sl], X[sl], mask, list(e.qvec), list(e.tvec))
            after = ref.cauchy_cost(cams[i], xy[sl], X[sl], mask, reg["qvec"][i], reg["tvec"][i])
            r = reg["refinement"]["results"][reg["refined_index"][i]]
            planted = np.array(rt.pose_matrix(s["qvec"][i], s["tvec"][i])[0]).reshape(3, 4)
            Pe = np.array(list(e.proj_matrix)).reshape(3, 4)
            Pr = np.concatenate([scenes.quat_to_rot(reg["qvec"][i]), reg["tvec"][i][:, None]], axis=1)
            print(noise, i, "cost %.6g -> %.6g" % (before, after), "to planted %.3e -> %.3e" % (np.linalg.norm(Pe - planted), np.linalg.norm(Pr - planted)))
            # slack: rounding only.  On exact data the estimate is already at the minimum to ~1e-12, the refinement ends at the
            # gradient test without a step and returns the pose with qvec normalised: equal up to a few ulps of the O(1) entries
            assert after <= before * (1 + 1e-9) + 1e-15 and abs(r.final_cost - after) <= 1e-9 * after + 1e-15
            if noise == 0.0:
                assert np.linalg.norm(Pr - planted) <= np.linalg.norm(Pe - planted) + 1e-12
            assert np.linalg.norm(Pr - planted) < 5e-2
            qvec[i], tvec[i] = reg["qvec"][i], reg["tvec"][i]
        if noise == 0.0:
            continue
        scene = dict(s)
        scene.update(qvec=qvec, tvec=tvec, registered=np.array(enough, np.uint8))
        tri = ctx.retriangulate(scene, ids[3:5])
        assert tri["report"].num_new_points > 0 and tri["num_tris"] > 0
        toffs = tri["new_track_offsets"]
        tracks = {}
        for i in range(len(ids)):
            for k, m in zip(rows[i], reg["inlier_mask"][int(offs[i]):int(offs[i + 1])]):
                if m and enough[i]:
                    tracks.setdefault(int(s["point3D_ids"][p3[off[i] + k]]), []).append((i, int(k)))
        for (img, k), pid in zip(tri["continued_obs"], tri["continued_point_ids"]):
            tracks.setdefault(int(pid), []).append((ids.index(int(img)), int(k)))
        xyz = {int(p): x for p, x in zip(s["point3D_ids"], s["point3D_xyz"])}
        for kk in range(len(toffs) - 1):
            pid = int(tri["new_point_ids"][kk])
            xyz[pid] = tri["new_xyz"][kk]
            tracks[pid] = [(ids.index(int(a)), int(b)) for a, b in tri["new_track_obs"][toffs[kk]:toffs[kk + 1]]]
        pids = sorted(p for p in tracks if len(tracks[p]) >= 2)
        cam = s["cameras"][0]
        ba = ctx.bundle_adjust(dict(
            camera_model_ids=[cam.model_id], camera_params=list(cam.params)[:3], image_camera=np.zeros(len(ids)), qvec=qvec, tvec=tvec,
            image_constant_pose=np.array([1 if (i < 2 or not enough[i]) else 0 for i in range(len(ids))]),
            point_ids=np.array(pids, np.uint64), xyz=np.array([xyz[p] for p in pids]),
            track_offsets=np.concatenate([[0], np.cumsum([len(tracks[p]) for p in pids])]),
            obs_image=[i for p in pids for i, _ in tracks[p]], obs_xy=[s["points2D_xy"][off[i] + k] for p in pids for i, k in tracks[p]]))
        assert ba["report"].termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE)
        assert np.isfinite(ba["report"].final_cost) and ba["report"].final_cost <= ba["report"].initial_cost
