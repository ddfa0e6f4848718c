"""GPU: dsm_estimate_absolute_poses against the sequential restatement (tests/absolute_pose_ref.py), DESIGN.md 14.

Comparison rule (section 13's): where every margin of a problem is >= 1e-9, decision for decision -- success, the winning factor
index, num_trials, model_is_local, the inlier mask bit for bit, num_inliers -- and the model, qvec, tvec within POSE_TOLERANCE; the
other problems must agree on success and on num_inliers within 2 %.  At least 90 % of the random problems must be clear, in the
restatement (asserted without a device in test_absolute_pose_cpu.py) and in the device's own margins."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import absolute_pose_ref as ref
from tests import absolute_pose_scenes as scenes
from tests.absolute_pose_compare import compare, result_bytes, run_batch

pytestmark = pytest.mark.gpu

POSE_TOLERANCE = scenes.POSE_TOLERANCE  # measured on the restatement and re-measured by the CPU test (absolute_pose_scenes.py)


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def test_hand_scenes(ctx):
    hand = scenes.hand_scenes()
    names = sorted(hand)
    problems = [dict(cam=hand[k][0], xy=hand[k][1], X=hand[k][2], sweep=False) for k in names]
    out, offs = run_batch(ctx, problems)
    for b, k in enumerate(names):
        want = ref.estimate_absolute_pose(problems[b]["cam"], problems[b]["xy"], problems[b]["X"], False, problem=b)
        res = out["results"][b]
        print(k, res.success, res.num_inliers, res.num_trials, want["success"], want["num_inliers"], want["num_trials"])
        compare(res, out["inlier_mask"][int(offs[b]):int(offs[b + 1])], out["margins"][b], want, b)
        if k in ("n0", "n2"):
            assert not res.success and res.num_trials == 0 and res.factor_index == -1
        if k in ("planar", "collinear"):  # EPnP's rank test fires on every local optimisation: no local model can win
            assert res.success and not res.model_is_local and not want["model_is_local"]
            assert res.num_inliers == len(problems[b]["xy"]) and want["runs"][0]["num_lo"] > 0
            assert out["margins"][b][ref.M_BETA] == np.inf and want["margins"][ref.M_BETA] == np.inf  # EPnP never got past it
        if k in ("collinear", "planar", "n0", "n2", "n5"):  # clear in the restatement: compared decision for decision
            assert ref.is_clear(want["margins"]) and ref.is_clear(list(out["margins"][b])), k
        if k in ("n3", "n4", "duplicated"):  # exact ties (equal counts with equal zero sums, a root at exactly 0): never clear
            assert not ref.is_clear(want["margins"]), k


def test_random_grid_against_the_restatement(ctx):
    grid = scenes.RANDOM_GRID + scenes.SWEEP_GRID
    problems = [scenes.grid_problem(e) for e in grid]
    out, offs = run_batch(ctx, problems)
    clear = device_clear = 0
    for b, p in enumerate(problems):
        want = ref.estimate_absolute_pose(p["cam"], p["xy"], p["X"], p["sweep"], problem=b)
        res = out["results"][b]
        print(grid[b][:6], "device", res.success, res.factor_index, res.num_inliers, res.num_trials, res.model_is_local,
              "ref", want["success"], want["factor_index"], want["num_inliers"], want["num_trials"], want["model_is_local"],
              "margins", "%.1e" % min(out["margins"][b]), "%.1e" % min(want["margins"]))
        clear += compare(res, out["inlier_mask"][int(offs[b]):int(offs[b + 1])], out["margins"][b], want, b)
        device_clear += ref.is_clear(list(out["margins"][b]))
        assert res.success
    rep = out["report"]
    print("clear on both sides %d, on the device %d of %d; runs %d trials %d models %d local optimisations %d; device %.2f ms" %
          (clear, device_clear, len(grid), rep.num_runs, rep.num_trials, rep.num_models, rep.num_local_optimizations, rep.device_ms))
    assert device_clear >= 0.9 * len(grid) and clear >= 0.9 * len(grid)
    assert rep.num_runs == len(scenes.RANDOM_GRID) + 31 * len(scenes.SWEEP_GRID)
    wrong = out["results"][len(grid) - 1]  # the wrong prior: only the sweep recovers it
    assert wrong.factor_index > 0 and 0.7 * 800 < wrong.focal_params[0] < 1.3 * 800


def test_all_camera_models(ctx):
    problems = []
    for m in range(11):
        cam, xy, X, _ = scenes.registration(500 + m, 150, 0.3, 0.5, m)
        problems.append(dict(cam=cam, xy=xy, X=X, sweep=False))
    out, offs = run_batch(ctx, problems)
    for b, p in enumerate(problems):
        want = ref.estimate_absolute_pose(p["cam"], p["xy"], p["X"], False, problem=b)
        assert out["results"][b].success and out["results"][b].num_inliers >= 90
        compare(out["results"][b], out["inlier_mask"][int(offs[b]):int(offs[b + 1])], out["margins"][b], want, b)


def test_batch_composition_does_not_change_a_result(ctx):
    """The same problem alone, repeated, and shuffled inside a larger batch returns the same bytes (given the same seeds); two calls
    return the same bytes; explicit seeds equal the default ones when set to dsm_absolute_pose_seed."""
    grid = [scenes.grid_problem(e) for e in scenes.RANDOM_GRID[:6]] + [scenes.grid_problem(scenes.SWEEP_GRID[0])]
    S = len(capi.absolute_pose_factors())
    base, offs = run_batch(ctx, grid)
    again, _ = run_batch(ctx, grid)
    assert result_bytes(base) == result_bytes(again)
    default_seeds = np.array([[capi.absolute_pose_seed(b, s, 0) for s in range(S)] for b in range(len(grid))], np.uint32)
    explicit, _ = run_batch(ctx, grid, seeds=default_seeds)
    assert result_bytes(base) == result_bytes(explicit)
    order = [4, 6, 0, 2, 2, 5, 1, 3, 6]  # shuffled, with repeats; every problem keeps the seeds it had
    shuffled, soffs = run_batch(ctx, [grid[i] for i in order], seeds=default_seeds[order])
    for k, i in enumerate(order):
        assert bytes(shuffled["results"][k]) == bytes(base["results"][i]), (k, i)
        assert (shuffled["inlier_mask"][int(soffs[k]):int(soffs[k + 1])] == base["inlier_mask"][int(offs[i]):int(offs[i + 1])]).all()
    alone, _ = run_batch(ctx, [grid[6]], seeds=default_seeds[[6]])
    assert bytes(alone["results"][0]) == bytes(base["results"][6])
    other, _ = run_batch(ctx, grid, options=capi.default_absolute_pose_options(random_seed=5))
    assert result_bytes(other) != result_bytes(base)  # the user seed reaches the streams


def test_argument_errors(ctx):
    p = scenes.grid_problem(scenes.RANDOM_GRID[0])
    good = dict(cam=p["cam"], xy=p["xy"], X=p["X"], sweep=False)

    def fails(problems=None, options=None, offsets=None, text=""):
        problems = problems or [good]
        with pytest.raises(capi.DsmError) as e:
            if offsets is None:
                run_batch(ctx, problems, options)
            else:
                ctx.estimate_absolute_poses([q["cam"] for q in problems], [0] * len(problems), offsets,
                                            np.concatenate([q["xy"] for q in problems]), np.concatenate([q["X"] for q in problems]), options)
        assert "dsm error 1" in str(e.value) and "dsm_estimate_absolute_poses" in str(e.value) and text in str(e.value)
    bad = dict(good, xy=good["xy"].copy())
    bad["xy"][3, 1] = np.nan
    fails([bad], text="non-finite points2D")
    bad = dict(good, X=good["X"].copy())
    bad["X"][0, 0] = np.inf
    fails([bad], text="non-finite points3D")
    cam = scenes.camera(0)
    cam.model_id = 11
    fails([dict(good, cam=cam)], text="unknown camera model")
    cam = scenes.camera(2)
    cam.params[3] = np.nan
    fails([dict(good, cam=cam)], text="non-finite camera")
    n = len(good["xy"])
    fails([good, good], offsets=[0, n + 5, n], text="ascend")
    fails([good], offsets=[1, n], text="start at 0")
    d = capi.default_absolute_pose_options
    for kw in (dict(num_focal_length_samples=0), dict(min_focal_length_ratio=0.0), dict(max_focal_length_ratio=-1.0),
               dict(min_focal_length_ratio=10.0, max_focal_length_ratio=10.0), dict(max_error=0.0), dict(max_error=np.nan),
               dict(min_inlier_ratio=-0.1), dict(min_inlier_ratio=1.5), dict(confidence=-0.1), dict(confidence=1.5),
               dict(min_num_trials=50, max_num_trials=40), dict(confidence=np.nan)):
        fails(options=d(**kw), text="option out of range")
    fails(options=d(num_focal_length_samples=5000), problems=[dict(good, sweep=True)], text="focal-length factors")
    for kw in (dict(confidence=1.0), dict(min_inlier_ratio=0.0)):  # Check() accepts them, but the trial count is unbounded
        fails(options=d(**kw), text="trial count")
        bounded, _ = run_batch(ctx, [good], options=d(max_num_trials=50, **kw))
        assert bounded["results"][0].num_trials <= 50
    L = capi.lib()
    res, mask = capi.AbsolutePoseResult(), np.zeros(n, np.uint8)
    offs = np.array([0, n], np.uint64)
    rc = L.dsm_estimate_absolute_poses(ctx._h, 1, None, None, offs.ctypes.data, None, None, None, None, ctypes.addressof(res),
                                       mask.ctypes.data, None, None)
    assert rc == 1 and b"NULL" in L.dsm_last_error(ctx._h)
    offs = np.array([0, 2 ** 20 + 1], np.uint64)
    cams = (capi.Camera * 1)(good["cam"])
    flag = np.zeros(1, np.uint8)
    rc = L.dsm_estimate_absolute_poses(ctx._h, 1, ctypes.addressof(cams), flag.ctypes.data, offs.ctypes.data, None, None, None, None,
                                       ctypes.addressof(res), mask.ctypes.data, None, None)
    assert rc == 1 and b"1048576" in L.dsm_last_error(ctx._h)
    out, _ = run_batch(ctx, [])  # an empty batch is not an error
    assert out["results"] == [] and out["report"].num_runs == 0


def test_chain_register_retriangulate_bundle_adjust(ctx):
    """The chain, as section 13's: the images of a planted scene are registered by this call from their observations of the existing
    points -> the registered poses replace the scene's -> dsm_retriangulate over two of the images -> dsm_bundle_adjust."""
    from tests import retriangulation_ref as rt
    s, truth = rt.make_scene(n_images=8, n_points=500, track=(3, 6), noise=0.3, wrong=0.0, existing=0.6, seed=31)
    ids = [int(x) for x in s["image_ids"]]
    off, p3 = s["points2D_offsets"], s["points2D_point3D"]
    problems, rows = [], []
    for i in range(len(ids)):
        k = np.nonzero(p3[off[i]:off[i + 1]] >= 0)[0]
        rows.append(k)
        problems.append(dict(cam=s["cameras"][0], xy=s["points2D_xy"][off[i] + k], X=s["point3D_xyz"][p3[off[i] + k]], sweep=False))
    # the scene leaves the last image of every track unobserved, so the last image sees no existing point: it stays unregistered
    # (the mapper's abs_pose_min_num_inliers is 30), out of the re-triangulation and constant in the adjustment
    enough = [len(k) >= 30 for k in rows]
    assert sum(enough) >= 6 and all(enough[3:5])
    out, offs = run_batch(ctx, problems)
    qvec, tvec = np.array(s["qvec"], np.float64), np.array(s["tvec"], np.float64)
    for i, r in enumerate(out["results"]):
        if not enough[i]:
            continue
        assert r.success and r.num_inliers >= 0.95 * len(rows[i])
        planted = np.array(rt.pose_matrix(s["qvec"][i], s["tvec"][i])[0]).reshape(3, 4)
        assert np.linalg.norm(np.array(list(r.proj_matrix)).reshape(3, 4) - planted) < 5e-2
        qvec[i], tvec[i] = list(r.qvec), list(r.tvec)
    reg = dict(s)
    reg.update(qvec=qvec, tvec=tvec, registered=np.array(enough, np.uint8))
    seps = ids[3:5]
    tri = ctx.retriangulate(reg, seps)
    assert tri["report"].num_new_points > 0 and tri["num_tris"] > 0
    toffs = tri["new_track_offsets"]
    errs = [np.linalg.norm(tri["new_xyz"][k] - truth[tuple(int(v) for v in tri["new_track_obs"][toffs[k]])]) for k in range(len(toffs) - 1)]
    assert np.median(errs) < 0.05 and np.mean(np.array(errs) < 0.2) > 0.9
    # the reconstruction for BA: the inlier observations of the registrations + the continued observations + the new points
    tracks = {}
    for i in range(len(ids)):
        mask = out["inlier_mask"][int(offs[i]):int(offs[i + 1])]
        for k, m in zip(rows[i], mask):
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
    obs_image = [i for p in pids for i, _ in tracks[p]]
    obs_xy = [s["points2D_xy"][off[i] + k] for p in pids for i, k in tracks[p]]
    toff = np.concatenate([[0], np.cumsum([len(tracks[p]) for p in pids])])
    cam = s["cameras"][0]
    ba_scene = dict(camera_model_ids=[cam.model_id], camera_params=list(cam.params)[:3], image_camera=np.zeros(len(ids)),
                    qvec=qvec, tvec=tvec, image_constant_pose=np.array([1 if (i < 2 or not enough[i]) else 0 for i in range(len(ids))]),
                    point_ids=np.array(pids, np.uint64), xyz=np.array([xyz[p] for p in pids]), track_offsets=toff,
                    obs_image=obs_image, obs_xy=obs_xy)
    ba = ctx.bundle_adjust(ba_scene)
    assert ba["report"].termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE)
    assert np.isfinite(ba["report"].final_cost) and ba["report"].final_cost <= ba["report"].initial_cost
    for i in range(len(ids)):
        planted = np.array(rt.pose_matrix(s["qvec"][i], s["tvec"][i])[0]).reshape(3, 4)
        P = np.concatenate([scenes.quat_to_rot(ba["qvec"][i]), ba["tvec"][i][:, None]], axis=1)
        assert np.linalg.norm(P - planted) < 5e-2
