"""The numpy restatement of the global bundle adjustment (tests/bundle_adjustment_ref.py) on its own: Jacobians
against central differences, the optimum against scipy, and the LM / CG rules on hand-built cases."""
import os

import numpy as np
import pytest

from dagsfm_amd import capi
from dagsfm_amd.synthetic import world_to_image
from tests import bundle_adjustment_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("model", range(11))
def test_projection_jacobian_matches_central_differences(model):
    rng = np.random.default_rng(model)
    params = np.array(ref.DEFAULT_PARAMS[model], np.float64)
    u, v = rng.uniform(-0.6, 0.6, 40), rng.uniform(-0.5, 0.5, 40)
    u[0] = v[0] = 0.003  # FOV's small-radius branch, the fisheye models near the centre
    x, y, dx, dy = ref.project_with_jacobian(model, params, u, v)
    xs, ys = world_to_image(model, params, u, v)
    np.testing.assert_allclose(x, xs, rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(y, ys, rtol=1e-12, atol=1e-9)
    for k in range(2 + len(params)):
        h = 1e-6 * (1.0 if k < 2 else max(1.0, abs(params[k - 2])))
        if k < 2:
            du, dv = (h, 0.0) if k == 0 else (0.0, h)
            xp, yp = world_to_image(model, params, u + du, v + dv)
            xm, ym = world_to_image(model, params, u - du, v - dv)
        else:
            pp, pm = params.copy(), params.copy()
            pp[k - 2] += h
            pm[k - 2] -= h
            xp, yp = world_to_image(model, pp, u, v)
            xm, ym = world_to_image(model, pm, u, v)
        np.testing.assert_allclose(dx[:, k], (xp - xm) / (2 * h), rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(dy[:, k], (yp - ym) / (2 * h), rtol=1e-5, atol=1e-4)


def test_fov_small_omega_branch_jacobian():
    params = np.array([500.0, 510.0, 320.0, 240.0, 0.005])
    u, v = np.array([0.2, -0.1]), np.array([0.1, 0.3])
    _, _, dx, _ = ref.project_with_jacobian(7, params, u, v)
    h = 1e-7
    pp, pm = params.copy(), params.copy()
    pp[4] += h
    pm[4] -= h
    np.testing.assert_allclose(dx[:, 6], (world_to_image(7, pp, u, v)[0] - world_to_image(7, pm, u, v)[0]) / (2 * h), rtol=1e-5)


def test_residual_jacobian_matches_central_differences_through_quaternion_plus():
    scene = ref.make_scene(5, n_images=4, n_points=12, models=(4,), gauge=False)
    scene["image_constant_tvec"][2] = 2
    opt = dict(refine_focal_length=1, refine_principal_point=1, refine_extra_params=1)
    pb = ref.Problem(scene, opt)
    st = {"qvec": scene["qvec"] / np.linalg.norm(scene["qvec"], axis=1, keepdims=True), "tvec": scene["tvec"].copy(),
          "xyz": scene["xyz"].copy(), "camera_params": scene["camera_params"].copy()}
    r, J = pb.residuals(st, True)
    J = J.toarray()
    n = pb.ne + pb.nf
    h = 1e-6
    num = np.zeros((2 * pb.n, n))
    for c in range(n):
        d = np.zeros(n)
        d[c] = h
        rp = pb.residuals(pb.plus(st, d)).reshape(-1)
        rm = pb.residuals(pb.plus(st, -d)).reshape(-1)
        num[:, c] = (rp - rm) / (2 * h)
    np.testing.assert_allclose(J, num, rtol=1e-5, atol=1e-4 * np.abs(num).max())


def test_quaternion_plus_is_ceres():
    x = np.array([0.9, 0.1, -0.3, 0.2])
    x /= np.linalg.norm(x)
    d = np.array([0.01, -0.02, 0.03])
    out = ref.quat_plus(x, d)[0]
    n = np.linalg.norm(d)
    a = np.concatenate([[np.cos(n)], np.sin(n) / n * d])
    prod = np.array([a[0] * x[0] - a[1:] @ x[1:], *(a[0] * x[1:] + x[0] * a[1:] + np.cross(a[1:], x[1:]))])
    np.testing.assert_allclose(out, prod, rtol=1e-15)
    assert np.isclose(np.linalg.norm(out), 1.0)
    assert (ref.quat_plus(x, np.zeros(3))[0] == x).all()


@pytest.mark.parametrize("model,shared", [(2, True), (4, False), (7, True)])
def test_restatement_reaches_the_scipy_optimum(model, shared):
    scene = ref.make_scene(20 + model, n_images=5, n_points=40, models=(model,), shared=shared, const_point_frac=0.1)
    opt = dict(gradient_tolerance=1e-12, max_num_iterations=200, max_linear_solver_iterations=500)
    out = ref.bundle_adjust(scene, opt)
    best = ref.scipy_optimum(scene, {})
    assert abs(out["report"]["final_cost"] - best) <= 1e-8 * best


class RecordingOperator:
    """S as an operator that records every vector it is applied to."""

    def __init__(self, S):
        self.S, self.args = S, []

    def __matmul__(self, v):
        self.args.append(np.array(v, copy=True))
        return self.S @ v


def test_cg_resets_the_residual_every_ten_iterations():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(30, 30))
    S = A @ A.T + 1e-3 * np.eye(30)  # ill-conditioned: the recurrence residual drifts from b - S x
    b = rng.normal(size=30)
    op = RecordingOperator(S)
    x, k, fail = ref.cg(op, b, np.eye(30), 25, {"cg": np.inf})
    assert fail == 0 and 10 < k < 20
    # one S p per iteration, plus S x after iteration 10: the 11th product is applied to the iterate of iteration 10
    assert len(op.args) == k + 1
    x10, _, _ = ref.cg(S, b, np.eye(30), 10, {"cg": np.inf})
    assert (op.args[10] == x10).all()
    # and the iterate after the reset follows r = b - S x: a plain recurrence gives a different iterate 11
    def plain_cg(n):
        x, r, rho, p = np.zeros(30), b.copy(), 1.0, None
        for i in range(1, n + 1):
            z = np.eye(30) @ r
            last, rho = rho, r @ z
            p = z if i == 1 else z + (rho / last) * p
            q = S @ p
            alpha = rho / (p @ q)
            x, r = x + alpha * p, r - alpha * q
        return x
    x11, _, _ = ref.cg(S, b, np.eye(30), 11, {"cg": np.inf})
    assert (plain_cg(10) == x10).all() and not (plain_cg(11) == x11).all()


def test_cg_invalid_and_zero_right_hand_side():
    S = np.diag([1.0, -1.0])
    _, k, fail = ref.cg(S, np.array([0.0, 1.0]), np.eye(2), 10, {"cg": np.inf})
    assert fail == 2 and k == 1  # p'Sp <= 0
    x, k, fail = ref.cg(np.eye(2), np.zeros(2), np.eye(2), 10, {"cg": np.inf})
    assert k == 0 and fail == 0 and (x == 0).all()


def test_rejected_steps_shrink_the_radius_and_the_cap_counts_every_iteration():
    scene = ref.make_scene(100, models=(0,))  # converges to the rounding floor by iteration 10, then rejects
    out = ref.bundle_adjust(scene, dict(gradient_tolerance=0.0, max_num_iterations=16))
    tr = out["trace"]
    assert out["report"]["termination"] == ref.NO_CONVERGENCE and out["report"]["num_iterations"] == 16
    acc = np.array(out["accepted"])
    assert (acc == 0).any() and (acc == 1).any()
    k = int(np.nonzero(acc == 0)[0][0]) + 1
    assert tr[k, 1] == tr[k - 1, 1] / 2.0  # the first rejection after an acceptance: decrease factor 2
    assert out["report"]["num_iterations"] == len(acc)


def test_invalid_steps_end_in_failure(monkeypatch):
    scene = ref.make_scene(31)
    monkeypatch.setattr(ref, "cg", lambda S, b, M, k, m: (np.zeros_like(b), 1, 2))  # every solve ends at p'Sp <= 0
    out = ref.bundle_adjust(scene, dict(max_num_consecutive_invalid_steps=3))
    rep, tr = out["report"], out["trace"]
    assert rep["termination"] == ref.FAILURE and rep["num_iterations"] == 3 and rep["num_invalid_steps"] == 3
    assert list(tr[:, 1]) == [1e4, 1e4 / 2, 1e4 / 8, 1e4 / 8]  # radius / 2, / 4, then the failure leaves it


def test_failed_initial_evaluation_is_a_failure():
    scene = ref.make_scene(32)
    scene["obs_xy"][:] = np.nan
    out = ref.bundle_adjust(scene)
    assert out["report"]["termination"] == ref.FAILURE and out["report"]["num_iterations"] == 0


def test_entry_point_is_exported_by_both_libraries():
    for check in (False, True):
        L = capi.lib(check)
        assert hasattr(L, "dsm_bundle_adjust") and hasattr(L, "dsm_default_bundle_adjustment_options")
    o = capi.default_bundle_adjustment_options()
    assert (o.max_num_iterations, o.max_linear_solver_iterations, o.gradient_tolerance, o.function_tolerance,
            o.parameter_tolerance, o.max_num_consecutive_invalid_steps) == (50, 100, 1.0, 0.0, 0.0, 10)
    assert (o.refine_focal_length, o.refine_principal_point, o.refine_extra_params) == (1, 0, 1)
    assert os.path.getsize(capi.LIB_PATH) <= 3.5 * 2 ** 20
