"""CPU: the numpy restatement of dsm_refine_absolute_poses (tests/pose_refinement_ref.py) against an independent
scipy minimum, planted poses and Ceres' rules; the non-vacuity and clear-share conditions of the grid the GPU test compares on;
the measured tolerances of that comparison."""
import functools

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import absolute_pose_scenes as scenes
from tests import pose_refinement_ref as ref
from tests import pose_refinement_scenes as sc
from tests.bundle_adjustment_ref import NUM_PARAMS, TWO_FOCAL

TIGHT = dict(gradient_tolerance=1e-10)


@functools.lru_cache(maxsize=None)
def grid_runs():
    """(problem, default run, probe stable, tight run) of every grid problem."""
    out = []
    for p in sc.grid():
        a = sc.args(p)
        r = ref.refine(*a)
        out.append((p, r, ref.stable_under_rounding(a, None, r), ref.refine(*a, opts=TIGHT)))
    return out


def clear(r, stable):
    return ref.is_clear(r["margins"]) and stable


def test_grid_is_not_vacuous():
    runs = grid_runs()
    noisy = [(p, r, t) for p, r, _, t in runs if p["noise"] > 0]
    assert len(noisy) >= 40
    for p, r, t in noisy:
        assert r["success"] and r["num_successful_steps"] >= 1, r["steps"]
        assert r["final_cost"] < r["initial_cost"]
        # gradient_tolerance 1e-10 is out of reach: the run goes on to the function or the parameter tolerance
        assert t["termination"] == ref.CONVERGENCE and t["steps"][-1] == ref.TOLERANCE, t["steps"]
        assert t["num_iterations"] >= r["num_iterations"]
    assert sum(r["num_iterations"] >= 2 for _, r, _ in noisy) >= 0.5 * len(noisy)
    assert any(r["steps"][-1] == ref.ACCEPTED for _, r, _ in noisy)  # the default tolerance of 1.0 ends runs at the gradient test too


def test_clear_share():
    runs = grid_runs()
    n = sum(clear(r, s) for _, r, s, _ in runs)
    print("clear %d of %d" % (n, len(runs)))
    assert n >= 0.9 * len(runs)


def test_optimum_equals_scipy_least_squares():
    """Every grid problem with pixel noise (the one noise-free problem ends at a cost of 1e-10, rounding of its exact data, where
    a bound relative to the cost says nothing: it must end below 1e-9 of its initial cost, and test_exact_scenes_return_the_planted_pose
    checks such scenes against their planted pose).  With gradient_tolerance 1e-10 a run ends at Ceres' function tolerance: its last cost change was below
    1e-6 of the cost.  The bound allows as much again for what is left to the minimum (the steps of a converging
    Levenberg-Marquardt run on these small-residual problems shrink, so the tail is below the last change): the restatement's cost
    may be at most 2e-6 (relative) above a minimum scipy finds.  scipy is asked twice, to tolerances of 1e-13: from the same start,
    and from the restatement's own result (a descent direction the restatement missed would show there).  A scipy run that ends
    ABOVE the restatement is scipy stopping early on an ill-conditioned camera block; a minimiser's result does not bound the
    minimum from below, so that side is not asserted."""
    for i, (p, _, _, t) in enumerate(grid_runs()):
        if p["noise"] == 0:
            assert t["final_cost"] <= 1e-9 * t["initial_cost"], i
            continue
        got = ref.cauchy_cost((p["cam"].model_id, list(t["camera_params"])), p["xy"], p["X"], p["mask"], t["qvec"], t["tvec"])
        assert abs(got - t["final_cost"]) <= 1e-12 * got  # the cost of the result, summed independently
        from_start = ref.scipy_optimum(*sc.args(p))
        cam = capi.Camera.from_buffer_copy(bytes(p["cam"]))
        for j in range(12):
            cam.params[j] = t["camera_params"][j]
        from_result = ref.scipy_optimum(cam, p["xy"], p["X"], p["mask"], t["qvec"], t["tvec"], p["flags"])
        print(i, got, from_start, from_result, (got - min(from_start, from_result)) / got)
        assert got <= from_start * (1 + 2e-6) and got <= from_result * (1 + 2e-6), i


def test_exact_scenes_return_the_planted_pose():
    for m in range(11):
        for flags in (0, 3):
            p = sc.problem(900 + m, 80, 0.0, 0.0, m, flags, focal_error=0.01 if flags else 0.0)
            r = ref.refine(*sc.args(p), opts=TIGHT)
            assert r["success"] and r["final_cost"] < 1e-9 * r["initial_cost"], (m, flags, r["final_cost"])
            q = sc.planted_quat(p["P"])
            assert min(np.abs(r["qvec"] - q).max(), np.abs(r["qvec"] + q).max()) < 1e-6, (m, flags)
            assert np.abs(r["tvec"] - p["P"][:, 3]).max() < 1e-5 * np.abs(p["P"][:, 3]).max(), (m, flags)
            if flags:
                true = scenes.camera(m)
                nfoc = 2 if m in TWO_FOCAL else 1
                assert np.allclose(r["camera_params"][:nfoc], list(true.params)[:nfoc], rtol=1e-5), (m, r["camera_params"])
                assert list(r["camera_params"][nfoc:nfoc + 2]) == list(true.params)[nfoc:nfoc + 2]  # the principal point: the input bits


def test_zero_inliers_return_the_input_bits():
    p = sc.hand_problems()["n0"]
    q = np.array(p["qvec"]) * 1.7  # not normalised: Ceres never touches it
    r = ref.refine(p["cam"], p["xy"], p["X"], p["mask"], q, p["tvec"], 3)
    assert r["success"] and r["termination"] == ref.CONVERGENCE and r["num_iterations"] == 0 and r["num_residual_blocks"] == 0
    assert r["qvec"].tobytes() == q.tobytes() and r["tvec"].tobytes() == np.asarray(p["tvec"]).tobytes()
    assert list(r["camera_params"]) == list(p["cam"].params) and r["initial_cost"] == 0.0 and r["final_cost"] == 0.0


def test_flags_free_exactly_the_expected_indices():
    """Every flag combination on every model: the refined run changes the free indices only (pose.cc:252-288)."""
    for m in range(11):
        nfoc, npar = (2 if m in TWO_FOCAL else 1), NUM_PARAMS[m]
        focal, pp, extra = list(range(nfoc)), [nfoc, nfoc + 1], list(range(nfoc + 2, npar))
        for flags in range(4):
            want = (focal if flags & 1 else []) + (extra if flags & 2 else [])
            assert ref.free_indices(m, flags) == want and not set(want) & set(pp)
            p = sc.problem(950 + m, 120, 0.1, 0.5, m, flags, focal_error=0.01)
            r = ref.refine(*sc.args(p))
            before = np.array(list(p["cam"].params))
            moved = [j for j in range(12) if r["camera_params"][j] != before[j]]
            assert r["success"] and moved == want, (m, flags, moved, want)


def test_corrector_always_takes_its_first_branch():
    """rho'' of the Cauchy loss is negative for every s and every scale, so Corrector's first branch (residual and Jacobian rows
    scaled by sqrt(rho')) is the only one RefineAbsolutePose can reach; the second branch's formula is pinned for contrast."""
    s = np.concatenate([[0.0], np.logspace(-300, 300, 601)])
    for scale in (1e-3, 0.5, 1.0, 7.0, 1e3):
        rho, rho1, rho2 = ref.cauchy(s, scale * scale)
        assert (rho2 <= 0.0).all() and (rho1 > 0.0).all() and ref.corrector_branch(s, rho1, rho2).all()
        big = (s / scale ** 2 > 1e-3) & (s / scale ** 2 < 1e200)
        assert np.allclose(rho[big], scale * scale * np.log1p(s[big] / scale ** 2), rtol=1e-12)
    assert not ref.corrector_branch(np.array([1.0]), np.array([1.0]), np.array([0.1]))[0]  # a loss with rho'' > 0 would leave it
    # evaluate() asserts the branch on every residual it corrects; its rows are the plain rows times sqrt(rho')
    p = sc.grid()[0]
    free = ref.free_indices(p["cam"].model_id, 0)
    prm = np.array(list(p["cam"].params))
    _, J, r = ref.evaluate(p["cam"].model_id, prm, free, p["qvec"], p["tvec"], p["xy"], p["X"], p["mask"], 1.0)
    _, J0, r0 = ref.evaluate(p["cam"].model_id, prm, free, p["qvec"], p["tvec"], p["xy"], p["X"], p["mask"], 1e300)  # rho' = 1
    sq = np.sqrt(1.0 / (1.0 + (r0 * r0).sum(1)))
    assert np.allclose(J, J0 * sq[:, None, None], rtol=1e-14) and np.allclose(r, r0 * sq[:, None], rtol=1e-14)


def test_option_errors():
    p = sc.grid()[0]
    for kw, text in ((dict(gradient_tolerance=-1.0), "out of range"), (dict(gradient_tolerance=np.nan), "out of range"),
                     (dict(max_num_iterations=-1), "out of range"), (dict(loss_function_scale=-1.0), "out of range"),
                     (dict(loss_function_scale=np.inf), "out of range"), (dict(loss_function_scale=0.0), "loss_function_scale = 0"),
                     (dict(max_num_iterations=ref.MAX_ITERATIONS + 1), "above 1000")):
        with pytest.raises(ValueError) as e:
            ref.refine(*sc.args(p), opts=kw)
        assert text in str(e.value)
    r = ref.refine(*sc.args(p), opts=dict(max_num_iterations=0))  # Check() accepts it: no step, NO_CONVERGENCE, still usable
    assert r["success"] and r["termination"] == ref.NO_CONVERGENCE and r["num_iterations"] == 0
    assert abs(np.linalg.norm(r["qvec"]) - 1.0) < 1e-15
    r = ref.refine(*sc.args(p), opts=dict(max_num_iterations=2))
    assert r["termination"] == ref.NO_CONVERGENCE and r["num_iterations"] == 2
    assert ref.DEFAULTS == dict(gradient_tolerance=1.0, loss_function_scale=1.0, max_num_iterations=100)  # pose.h:82-88
    assert capi.POSE_REFINEMENT_MAX_ITERATIONS == ref.MAX_ITERATIONS and capi.POSE_REFINEMENT_MARGINS == ref.MARGINS


def one_ulp(p, seed):
    rng = np.random.default_rng([seed, 77])
    cam = capi.Camera.from_buffer_copy(bytes(p["cam"]))
    prm = scenes.ulp_perturbed(rng, np.array(list(cam.params)))
    for j in range(12):
        cam.params[j] = prm[j]
    return (cam, scenes.ulp_perturbed(rng, p["xy"]), scenes.ulp_perturbed(rng, p["X"]), p["mask"], scenes.ulp_perturbed(rng, p["qvec"]),
            scenes.ulp_perturbed(rng, p["tvec"]), p["flags"])


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / max(float(np.max(np.abs(b))), 1e-300))


def test_one_ulp_sensitivity_stays_within_the_measured_constants():
    """The GPU comparison's tolerances are 16 times these: every input of a problem moved by one ulp.  Clear grid problems: the
    costs, qvec, tvec and the camera parameters, no decision flipped.  The hand problems: the final cost against the initial
    cost (what exact data leaves as a final cost is orders below it), clear or not."""
    worst = 0.0
    for i, (p, r, stable, _) in enumerate(grid_runs()):
        if not clear(r, stable):
            continue
        o = ref.refine(*one_ulp(p, i))
        assert o["steps"] == r["steps"] and o["termination"] == r["termination"], i
        worst = max(worst, rel(o["qvec"], r["qvec"]), rel(o["tvec"], r["tvec"]), rel(o["camera_params"], r["camera_params"]),
                    rel([o["final_cost"]], [r["final_cost"]]), rel([o["initial_cost"]], [r["initial_cost"]]))
    print("clear grid problems: %.3e" % worst)
    assert worst <= sc.MEASURED_ULP_SENSITIVITY
    # the hand problems (exact data): the final cost against the initial cost, 16 directions; the clear ones also in the rest
    worst_h = 0.0
    for k, p in sc.hand_problems().items():
        r = ref.refine(*sc.args(p))
        is_clear = clear(r, ref.stable_under_rounding(sc.args(p), None, r))
        for seed in range(16):
            o = ref.refine(*one_ulp(p, seed))
            assert o["success"] == r["success"], k
            worst_h = max(worst_h, abs(o["final_cost"] - r["final_cost"]) / max(r["initial_cost"], 1e-300))
            if is_clear and r["num_residual_blocks"]:
                assert o["steps"] == r["steps"] and o["termination"] == r["termination"], k
                assert max(rel(o["qvec"], r["qvec"]), rel(o["tvec"], r["tvec"]), rel(o["camera_params"], r["camera_params"]),
                           rel([o["initial_cost"]], [r["initial_cost"]])) <= sc.MEASURED_ULP_SENSITIVITY, k
        print(k, "clear", is_clear, "final cost %.3e of initial %.3e" % (r["final_cost"], r["initial_cost"]))
    print("hand problems, final cost over initial cost: %.3e" % worst_h)
    assert worst_h <= sc.MEASURED_ULP_SENSITIVITY_HAND


def test_hand_problems_terminate():
    for k, p in sc.hand_problems().items():
        r = ref.refine(*sc.args(p))
        assert r["num_iterations"] <= 100 and r["termination"] in (ref.CONVERGENCE, ref.NO_CONVERGENCE, ref.FAILURE), k
        assert np.isfinite(r["final_cost"]) and r["final_cost"] <= r["initial_cost"], k
