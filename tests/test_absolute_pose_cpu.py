"""CPU-only: the restatement of EstimateAbsolutePose (tests/absolute_pose_ref.py) against the reference's known answers, the pinned
counts of DESIGN.md 14, the C symbols of the stage, and the clear-scene share of the random grid the GPU test compares on."""
import ctypes
import math

import numpy as np

from dagsfm_amd import capi
from tests import absolute_pose_ref as ref
from tests import absolute_pose_scenes as scenes
from tests import oracle_lib


def test_focal_length_factor_counts():
    """pose.cc:92-98 as written: 30 samples give 31 factors (the last from f = 0.9999999999999999), 50 give 50 (the end point is
    lost), 100 give 100 -- in the restatement and in the library."""
    for n, want in ((30, 31), (50, 50), (100, 100)):
        f = ref.focal_length_factors(n, 0.1, 10.0)
        assert len(f) == want
        got = capi.absolute_pose_factors(capi.default_absolute_pose_options(num_focal_length_samples=n))
        assert list(got) == f
    f = ref.focal_length_factors(30, 0.1, 10.0)
    assert f[0] == 0.1 and f[-1] < 10.0 and f[-1] > 9.99


def test_constructor_cap_is_585():
    orc = oracle_lib.load()
    assert orc.compute_num_trials(25000, 100000, 0.9999, 3) == 585
    assert ref.max_num_trials(ref.DEFAULTS) == 585
    assert capi.absolute_pose_max_trials() == 585
    assert capi.absolute_pose_max_trials(capi.default_absolute_pose_options(max_num_trials=100)) == 100
    for k, n in ((1, 10), (5, 10), (10, 10), (300, 1000)):  # the restatement's table against the oracle's ComputeNumTrials
        assert ref.compute_num_trials(k, n, 0.9999) == orc.compute_num_trials(k, n, 0.9999, 3)


def test_option_defaults_match_the_mapper():
    # src/sfm/incremental_mapper.cc:438-449, incremental_mapper.h:84,90,106,107; RANSACOptions' max_num_trials (ransac.h:62)
    o = capi.default_absolute_pose_options()
    assert (o.num_focal_length_samples, o.min_focal_length_ratio, o.max_focal_length_ratio) == (30, 0.1, 10.0)
    assert (o.max_error, o.min_inlier_ratio, o.confidence, o.min_num_trials, o.max_num_trials) == (12.0, 0.25, 0.9999, 30, 2 ** 64 - 1)
    for k, v in ref.DEFAULTS.items():
        assert getattr(o, k) == v


def test_seed_function_against_the_c_symbol():
    def py_seed(b, s, user):
        m = (1 << 64) - 1
        h = (((b << 32) | s) + 0x9e3779b97f4a7c15) & m
        h ^= h >> 33
        h = (h * 0xff51afd7ed558ccd) & m
        h ^= h >> 33
        h = (h * 0xc4ceb9fe1a85ec53) & m
        h ^= h >> 33
        return (h & 0xffffffff) ^ user
    seen = set()
    for b in (0, 1, 2, 63, 2 ** 32 - 1):
        for s in (0, 1, 30):
            for user in (0, 7):
                assert capi.absolute_pose_seed(b, s, user) == py_seed(b, s, user)
                seen.add(capi.absolute_pose_seed(b, s, user))
    assert len(seen) == 30


def test_known_answer_scenes():
    """src/estimators/absolute_pose_test.cc: the eight points under qx in {0 .. 0.8}, tx in {0 .. 0.9}; the model within 1e-2 (P3P,
    here the LO-RANSAC of P3P + EPnP) and 1e-3 (EPnP over the sampler's 4-point sets, as RANSAC<EPNPEstimator> draws them) of the
    planted transform, exact points' residuals < 1e-3, faulty ones > 0.1."""
    orc = oracle_lib.load()
    X = scenes.KNOWN_POINTS3D
    faulty = X.copy()
    faulty[:, 0] = 20
    for qx in scenes.KNOWN_QX:
        for tx in scenes.KNOWN_TX:
            P, x = scenes.known_scene(qx, tx)
            rep = ref.loransac(x, X, 1e-5 * 1e-5, 0, dict(ref.DEFAULTS))
            assert rep["success"]
            assert np.linalg.norm(rep["model"] - P) < 1e-2
            assert (ref.residuals(rep["model"], x, X) < 1e-3).all()
            assert (ref.residuals(rep["model"], x, faulty) > 0.1).all()
            best, best_n = None, -1
            for s in orc.sample_sequence(0, 4, 8, 100):
                m = ref.epnp(x[s], X[s])
                if m is None:
                    continue
                n = int((ref.residuals(m, x, X) <= 1e-10).sum())
                if n > best_n:
                    best, best_n = m, n
            assert best is not None and np.linalg.norm(best - P) < 1e-3
            assert (ref.residuals(best, x, X) < 1e-3).all()
            assert (ref.residuals(best, x, faulty) > 0.1).all()


def test_p3p_returns_the_planted_pose_among_its_models():
    """P3P alone, on all 50 known-answer scenes: one of its models is the planted transform within the reference's 1e-2."""
    for qx in scenes.KNOWN_QX:
        for tx in scenes.KNOWN_TX:
            P, x = scenes.known_scene(qx, tx)
            models = ref.p3p(x[[0, 1, 7]], scenes.KNOWN_POINTS3D[[0, 1, 7]])
            assert 1 <= len(models) <= 4
            best = min(models, key=lambda m: np.linalg.norm(m - P))
            assert np.linalg.norm(best - P) < 1e-2
            assert (ref.residuals(best, x, scenes.KNOWN_POINTS3D) < 1e-3).all()
    assert ref.p3p(x[[0, 0, 7]], scenes.KNOWN_POINTS3D[[0, 0, 7]]) == []  # a repeated world point: no model


def test_solve_for_sign_negates_whenever_the_depth_is_non_zero():
    """absolute_pose.cc:538-547 as the reference has it: the control points are negated whenever pcs_[0][2] is non-zero, whatever its
    sign.  Every candidate of every scene is negated, so a candidate that started in front of the camera ends behind it; EPnP is
    right only where the null vector's arbitrary sign put the points behind the camera first."""
    right = wrong = 0
    for qx in scenes.KNOWN_QX:
        for tx in scenes.KNOWN_TX[::3]:
            P, x = scenes.known_scene(qx, tx)
            trace = []
            m = ref.epnp(x, scenes.KNOWN_POINTS3D, trace=trace)
            assert len(trace) == 3 and all(t["negated"] for t in trace)
            behind_first = [t["first_depth_before"] < 0 for t in trace]
            good = np.linalg.norm(m - P) < 1e-3
            if good:
                assert any(behind_first)  # a right answer needs a candidate that started behind the camera
            if not any(behind_first):
                assert not good           # all three started in front and were negated: no candidate is left to be right
            right += good
            wrong += not good
    assert right >= 1 and wrong >= 1 and right + wrong == 20  # the rule gives both outcomes on exact data


def test_tree_sum_is_the_fixed_order_it_says():
    rng = np.random.default_rng(3)
    for n in (1, 63, 64, 65, 200):
        t = rng.normal(size=n) * 10.0 ** rng.integers(-8, 8, n)
        lanes = [0.0] * 64
        for i in range(n):
            lanes[i % 64] = lanes[i % 64] + float(t[i])
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ o] for l in range(64)]
        assert ref.tree_sum(t) == lanes[0]
    mask = rng.random(200) < 0.5
    assert ref.tree_sum(t, mask) == ref.tree_sum(np.where(mask, t, 0.0))


def test_small_linear_algebra_against_numpy():
    rng = np.random.default_rng(5)
    for k in (3, 4, 5):
        A, b = rng.normal(size=(6, k)), rng.normal(size=6)
        want = np.linalg.lstsq(A, b, rcond=None)[0]
        assert np.allclose(ref.svd_solve_tall(A, b), want, rtol=1e-10, atol=1e-12)
        assert np.allclose(ref.qr_solve(A, b), want, rtol=1e-10, atol=1e-12)
    M = rng.normal(size=(3, 3))
    assert np.allclose(ref.inverse3(M), np.linalg.inv(M)) and math.isclose(ref.det3(M), np.linalg.det(M), rel_tol=1e-12)


def test_too_few_points_is_not_an_error():
    cam = scenes.camera(0)
    for n in (0, 2):
        out = ref.estimate_absolute_pose(cam, np.zeros((n, 2)), np.zeros((n, 3)), False)
        assert not out["success"] and out["num_trials"] == 0 and out["num_inliers"] == 0


def test_unbounded_trial_counts_are_refused():
    """Options Check() accepts but that leave the trial count unbounded (DSM_ABSOLUTE_POSE_MAX_TRIALS)."""
    import pytest
    cam, xy, X, _ = scenes.registration(1, 30)
    xn = (xy - [500.0, 375.0]) / 800.0
    for kw in (dict(confidence=1.0), dict(min_inlier_ratio=0.0)):
        o = dict(ref.DEFAULTS, **kw)
        assert ref.max_num_trials(o) > ref.MAX_TRIALS
        assert capi.absolute_pose_max_trials(capi.default_absolute_pose_options(**kw)) > ref.MAX_TRIALS
        with pytest.raises(ValueError):
            ref.loransac(xn, X, 1e-4, 1, o)
        assert ref.loransac(xn, X, 1e-4, 1, dict(o, max_num_trials=40))["num_trials"] <= 40


def test_one_ulp_sensitivity_stays_within_the_measured_constant():
    """Re-measures what POSE_TOLERANCE rests on: every input of every clear grid problem moved by one ulp flips no decision and
    changes model / qvec / tvec by at most MEASURED_ULP_SENSITIVITY of the largest entry."""
    rng = np.random.default_rng(2024)
    worst = 0.0
    for b, entry in enumerate(scenes.RANDOM_GRID + scenes.SWEEP_GRID):
        pr = scenes.grid_problem(entry)
        a = ref.estimate_absolute_pose(pr["cam"], pr["xy"], pr["X"], pr["sweep"], problem=b)
        if not ref.is_clear(a["margins"]):
            continue
        c = ref.estimate_absolute_pose(pr["cam"], scenes.ulp_perturbed(rng, pr["xy"]), scenes.ulp_perturbed(rng, pr["X"]), pr["sweep"],
                                       problem=b)
        assert (a["mask"] == c["mask"]).all() and a["num_trials"] == c["num_trials"] and a["factor_index"] == c["factor_index"]
        assert a["model_is_local"] == c["model_is_local"]
        for k in ("proj_matrix", "qvec", "tvec"):
            worst = max(worst, float(np.max(np.abs(np.asarray(a[k]) - np.asarray(c[k]))) / np.max(np.abs(np.asarray(a[k])))))
    print("largest relative change under one ulp: %.3e" % worst)
    assert worst <= scenes.MEASURED_ULP_SENSITIVITY


def test_clear_share_of_the_random_grid():
    """The cap of the GPU comparison: at least 90 % of the random problems must be clear -- every margin >= 1e-9 -- in
    and, because near-identical EPnP candidates may swap, the residual and tie margins >= SWAP_BAR -- in the restatement alone.  A
    condition on the committed seeds and parameters, not a measurement of the device."""
    grid = scenes.RANDOM_GRID + scenes.SWEEP_GRID
    clear = 0
    for b, entry in enumerate(grid):  # problem b of the batch the GPU test runs: the same seeds
        pr = scenes.grid_problem(entry)
        out = ref.estimate_absolute_pose(pr["cam"], pr["xy"], pr["X"], pr["sweep"], problem=b)
        assert out["success"]
        clear += ref.is_clear(out["margins"])
    print("clear problems: %d of %d" % (clear, len(grid)))
    assert clear >= 0.9 * len(grid)


def test_sweep_recovers_a_wrong_prior():
    pr = scenes.grid_problem(scenes.SWEEP_GRID[1])  # the camera claims 2400, the scene was made with 800
    fixed = ref.estimate_absolute_pose(pr["cam"], pr["xy"], pr["X"], False)
    swept = ref.estimate_absolute_pose(pr["cam"], pr["xy"], pr["X"], True)
    assert swept["success"] and swept["num_inliers"] >= 0.6 * len(pr["xy"])
    assert swept["num_inliers"] > fixed["num_inliers"]  # with the wrong focal length fewer points fit any pose
    assert 0.7 * 800 < swept["focal_params"][0] < 1.3 * 800
    assert swept["focal_params"][0] == pr["cam"].params[0] * swept["focal_length_factor"]
