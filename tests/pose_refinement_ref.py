"""A sequential numpy restatement of dsm_refine_absolute_poses for test sizes: RefineAbsolutePose
(src/estimators/pose.cc:198-311) -- BundleAdjustmentCostFunction with the 3D point constant under ceres::CauchyLoss, the
trust-region rules of DESIGN.md 12, the damped normal equations solved by an unpivoted Cholesky -- in the device's summation
order (tests/absolute_pose_ref.tree_sum).  Every decision margin is recorded.  TEST INFRASTRUCTURE ONLY.

The loss and its corrector, in full (ceres/loss_function.cc, ceres/internal/corrector.cc).  CauchyLoss(a): b = a^2, c = 1 / b;
for s = |r|^2: sum = 1 + s c, inv = 1 / sum, rho = b log(sum), rho' = max(DBL_MIN, inv), rho'' = -c inv^2.
Corrector(s, rho): sqrt_rho1 = sqrt(rho').  If s == 0 or rho'' <= 0: residual_scaling = sqrt_rho1, alpha_sq_norm = 0 (the FIRST
branch).  Otherwise D = 1 + 2 s rho'' / rho', alpha = 1 - sqrt(D), residual_scaling = sqrt_rho1 / (1 - alpha),
alpha_sq_norm = alpha / s.  CorrectJacobian: alpha_sq_norm == 0 -> J *= sqrt_rho1, else
J = sqrt_rho1 (J - alpha_sq_norm r (r' J)).  CorrectResiduals: r *= residual_scaling.  rho'' of the Cauchy loss is negative
for every s (c > 0, inv > 0), so the first branch is always taken: rows and residual scaled by sqrt(rho')."""
import numpy as np

from tests.absolute_pose_ref import tree_sum
from tests.bundle_adjustment_ref import (CONVERGENCE, FAILURE, NO_CONVERGENCE, NUM_PARAMS, TWO_FOCAL, margin, project_with_jacobian,
                                         quat_plus, quat_rotate)

DBL_MIN = float(np.finfo(np.float64).tiny)
MIN_REL_DECREASE, MIN_DIAG, MAX_DIAG, MAX_RADIUS, MIN_RADIUS = 1e-3, 1e-6, 1e32, 1e16, 1e-32
FUNCTION_TOLERANCE, PARAMETER_TOLERANCE, MAX_INVALID = 1e-6, 1e-8, 5  # ceres::Solver::Options' defaults
MAX_ITERATIONS = 1000  # DSM_POSE_REFINEMENT_MAX_ITERATIONS
ACCEPTED, REJECTED, INVALID, TOLERANCE = 1, 2, 3, 4
MARGINS = ("acceptance", "gradient", "function_tolerance", "parameter_tolerance", "pivot")
CLEAR_MARGIN = 1e-9
DEFAULTS = dict(gradient_tolerance=1.0, loss_function_scale=1.0, max_num_iterations=100)


def check_options(opts):
    """AbsolutePoseRefinementOptions::Check plus what the device refuses; returns the error text or None."""
    g, s, m = opts["gradient_tolerance"], opts["loss_function_scale"], opts["max_num_iterations"]
    if not (g >= 0.0 and np.isfinite(g) and m >= 0 and s >= 0.0 and np.isfinite(s)):
        return "option out of range"
    if s == 0.0:
        return "loss_function_scale = 0"
    if m > MAX_ITERATIONS:
        return "max_num_iterations above 1000"
    return None


def free_indices(model, flags):
    """The camera parameter indices RefineAbsolutePose leaves free (pose.cc:252-288): never the principal point."""
    nfoc = 2 if model in TWO_FOCAL else 1
    return [j for j in range(NUM_PARAMS[model]) if (j < nfoc and flags & 1) or (j >= nfoc + 2 and flags & 2)]


def cauchy(s, b):
    """(rho, rho', rho'') of ceres::CauchyLoss with b = scale^2."""
    c = 1.0 / b
    sum_ = 1.0 + s * c
    inv = 1.0 / sum_
    return b * np.log(sum_), np.maximum(DBL_MIN, inv), -c * (inv * inv)


def corrector_branch(s, rho1, rho2):
    """True where Corrector takes its first branch."""
    return (s == 0.0) | (rho2 <= 0.0)


def evaluate(model, prm, free, q, t, xy, X, mask, b, jac=True):
    """cost, and with jac the corrected Jacobian rows J [N, 2, P] and residuals r [N, 2] (rows of masked points are unused)."""
    w = quat_rotate(np.tile(q, (len(X), 1)), X)
    P0, P1, P2 = w[:, 0] + t[0], w[:, 1] + t[1], w[:, 2] + t[2]
    with np.errstate(all="ignore"):
        u, v = P0 / P2, P1 / P2
        x, y, dx, dy = project_with_jacobian(model, list(prm[:NUM_PARAMS[model]]), u, v)
        r0, r1 = x - xy[:, 0], y - xy[:, 1]
        s = r0 * r0 + r1 * r1
        rho, rho1, rho2 = cauchy(s, b)
        cost = tree_sum(0.5 * rho, mask)
        if not jac:
            return cost
        assert corrector_branch(s, rho1, rho2)[np.asarray(mask, bool)].all()
        sq = np.sqrt(rho1)
        iz = 1.0 / P2
        Z = np.zeros_like(iz)
        duP = [iz, Z, -P0 * iz * iz]
        dvP = [Z, iz, -P1 * iz * iz]
        Dq = [[Z, 2.0 * w[:, 2], -2.0 * w[:, 1]], [-2.0 * w[:, 2], Z, 2.0 * w[:, 0]], [2.0 * w[:, 1], -2.0 * w[:, 0], Z]]
        J = np.zeros((len(X), 2, 6 + len(free)))
        for r, dd in enumerate((dx, dy)):
            JP = [dd[:, 0] * duP[a] + dd[:, 1] * dvP[a] for a in range(3)]
            for a in range(3):
                J[:, r, a] = sq * (JP[0] * Dq[0][a] + JP[1] * Dq[1][a] + JP[2] * Dq[2][a])
                J[:, r, 3 + a] = sq * JP[a]
            for j, pj in enumerate(free):
                J[:, r, 6 + j] = sq * dd[:, 2 + pj]
        rr = np.stack([sq * r0, sq * r1], axis=1)
    return cost, J, rr


def normal_equations(J, r, mask):
    """J'J and J'r as the device sums them: per entry the fixed-order tree sum of J0a J0b + J1a J1b over the points."""
    P = J.shape[2]
    terms, where = [], []
    for a in range(P):
        for b in range(a, P):
            terms.append(J[:, 0, a] * J[:, 0, b] + J[:, 1, a] * J[:, 1, b])
            where.append((a, b))
        terms.append(J[:, 0, a] * r[:, 0] + J[:, 1, a] * r[:, 1])
        where.append((a, -1))
    with np.errstate(all="ignore"):
        sums = tree_sum(np.stack(terms, axis=1), mask)
    A, g = np.zeros((P, P)), np.zeros(P)
    for (a, b), v in zip(where, sums):
        if b < 0:
            g[a] = v
        else:
            A[a, b] = A[b, a] = v
    return A, g


def cholesky_solve(A, D, radius, gs, margins):
    """(A + diag(sqrt(D / radius)^2)) step = -gs, unpivoted, in the device's loop order; None when a pivot is not positive and finite."""
    P = len(gs)
    L = np.zeros((P, P))
    with np.errstate(all="ignore"):
        for i in range(P):
            for j in range(i + 1):
                s = A[i, j]
                if i == j:
                    l = np.sqrt(D[i] / radius)
                    s = s + l * l
                diag = s
                for m in range(j):
                    s = s - L[i, m] * L[j, m]
                if i == j:
                    margins[4] = min(margins[4], abs(s) / diag if (np.isfinite(s) and diag > 0.0) else 0.0)
                    if not (s > 0.0) or not np.isfinite(s):
                        return None
                    L[i, i] = np.sqrt(s)
                else:
                    L[i, j] = s / L[j, j]
        w = np.zeros(P)
        for i in range(P):
            s = -gs[i]
            for m in range(i):
                s = s - L[i, m] * w[m]
            w[i] = s / L[i, i]
        for i in range(P - 1, -1, -1):
            s = w[i]
            for m in range(i + 1, P):
                s = s - L[m, i] * w[m]
            w[i] = s / L[i, i]
    return w


def refine(cam, xy, X, mask, qvec, tvec, flags, opts=None, perturb=0.0):
    """The restatement of one problem.  cam: a capi.Camera or (model_id, params).  Returns a dict: success, termination,
    num_iterations, num_successful_steps, num_invalid_steps, num_residual_blocks, initial_cost, final_cost, qvec, tvec,
    camera_params [12], steps (DSM_POSE_STEP_* per iteration), costs (the cost after every iteration), margins [5].
    perturb > 0: the scaled system of every solve carries a seeded relative perturbation of that size (the conditioning probe)."""
    o = dict(DEFAULTS)
    o.update(opts or {})
    err = check_options(o)
    if err:
        raise ValueError(err)
    model, params = (cam.model_id, list(cam.params)) if hasattr(cam, "model_id") else cam
    npar = NUM_PARAMS[model]
    prm = np.zeros(12)
    prm[:len(params)] = np.asarray(params, np.float64)[:12]
    xy, X = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(X, np.float64).reshape(-1, 3)
    mask = np.asarray(mask, np.uint8).reshape(-1)
    q, t = np.array(qvec, np.float64), np.array(tvec, np.float64)
    n_in = int((mask != 0).sum())
    mg = [np.inf] * 5
    out = dict(success=True, termination=CONVERGENCE, num_iterations=0, num_successful_steps=0, num_invalid_steps=0,
               num_residual_blocks=n_in, initial_cost=0.0, final_cost=0.0, qvec=q, tvec=t, camera_params=prm, steps=[], costs=[],
               margins=mg)
    if n_in == 0:  # Ceres solves the empty problem and calls it usable; qvec is not normalised (pose.cc:244)
        return out
    free = free_indices(model, flags)
    k, P = len(free), 6 + len(free)
    b = o["loss_function_scale"] ** 2
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    q = q / n if n > 0.0 else np.array([1.0, 0.0, 0.0, 0.0])
    gtol, max_iter = o["gradient_tolerance"], o["max_num_iterations"]
    st = dict(s=None)

    def system(q, t, prm, first):
        cost, J, r = evaluate(model, prm, free, q, t, xy, X, mask, b)
        A, g = normal_equations(J, r, mask)
        cn = np.diag(A).copy()
        with np.errstate(all="ignore"):
            if first:
                st["s"] = 1.0 / (1.0 + np.sqrt(cn))
            s = st["s"]
            As = (s[:, None] * A) * s[None, :]
            gs = s * g
            D = np.minimum(np.maximum((s * s) * cn, MIN_DIAG), MAX_DIAG)
            qp = quat_plus(q, -g[:3])[0]
            m = float(np.max(np.abs(q - qp)))
            m = max(m, float(np.max(np.abs(t - (t - g[3:6])))))
            for j, pj in enumerate(free):
                m = max(m, abs(prm[pj] - (prm[pj] - g[6 + j])))
        return cost, As, gs, D, m

    cost, As, gs, D, gnorm = system(q, t, prm, True)
    out["initial_cost"] = cost
    radius, dec = 1e4, 2.0
    it = n_succ = n_inv = n_inv_total = 0
    term = None

    def finalize(fresh):
        nonlocal term
        if term is not None:
            return
        if it >= max_iter:
            term = NO_CONVERGENCE
        elif fresh:
            mg[1] = min(mg[1], margin(gnorm, gtol))
            if gnorm <= gtol:
                term = CONVERGENCE
        if term is None and radius < MIN_RADIUS:
            term = CONVERGENCE

    if not np.isfinite(cost):
        term = FAILURE
    else:
        finalize(True)
    out["costs"].append(cost)
    while term is None:
        A_use, g_use = As, gs
        if perturb > 0.0:
            rng = np.random.default_rng(it)
            A_use = As * (1.0 + perturb * rng.standard_normal(As.shape))
            A_use = (A_use + A_use.T) / 2.0
            g_use = gs * (1.0 + perturb * rng.standard_normal(gs.shape))
        w = cholesky_solve(A_use, D, radius, g_use, mg)
        valid, cand_cost = False, np.inf
        if w is not None:
            with np.errstate(all="ignore"):
                mcc = 0.0
                for i in range(P):
                    a_s = 0.0
                    for j in range(P):
                        a_s = a_s + A_use[i, j] * w[j]
                    mcc = mcc + w[i] * (g_use[i] + a_s / 2.0)
                mcc = -mcc
                delta = st["s"] * w
                s2 = 0.0
                for i in range(P):
                    s2 = s2 + delta[i] * delta[i]
                cq = quat_plus(q, delta[:3])[0]
                ct = t + delta[3:6]
                cprm = prm.copy()
                for j, pj in enumerate(free):
                    cprm[pj] = prm[pj] + delta[6 + j]
            valid = bool(np.isfinite(mcc) and mcc > 0.0 and np.isfinite(s2))
            if valid:
                cand_cost = evaluate(model, cprm, free, cq, ct, xy, X, mask, b, jac=False)
        it += 1
        fresh = False
        if not (valid and np.isfinite(cand_cost)):
            n_inv += 1
            n_inv_total += 1
            out["steps"].append(INVALID)
            if n_inv >= MAX_INVALID:
                term = FAILURE
            else:
                radius /= dec
                dec *= 2.0
        else:
            n_inv = 0
            x2 = 0.0
            for i in range(4):
                x2 = x2 + q[i] * q[i]
            for i in range(3):
                x2 = x2 + t[i] * t[i]
            if k:
                for i in range(npar):
                    x2 = x2 + prm[i] * prm[i]
            step_norm, ptol = np.sqrt(s2), PARAMETER_TOLERANCE * (np.sqrt(x2) + PARAMETER_TOLERANCE)
            mg[3] = min(mg[3], margin(step_norm, ptol))
            change = cost - cand_cost
            if step_norm <= ptol:
                term = CONVERGENCE
                out["steps"].append(TOLERANCE)
            else:
                mg[2] = min(mg[2], margin(abs(change), FUNCTION_TOLERANCE * cost))
                if abs(change) <= FUNCTION_TOLERANCE * cost:
                    term = CONVERGENCE
                    out["steps"].append(TOLERANCE)
                else:
                    rho = change / mcc
                    mg[0] = min(mg[0], abs(change - MIN_REL_DECREASE * mcc) / max(cost, DBL_MIN))
                    if rho > MIN_REL_DECREASE:
                        out["steps"].append(ACCEPTED)
                        n_succ += 1
                        q, t, prm, cost = cq, ct, cprm, cand_cost
                        tmp = 2.0 * rho - 1.0
                        radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - tmp * tmp * tmp))
                        dec = 2.0
                        fresh = True
                        _, As, gs, D, gnorm = system(q, t, prm, False)
                    else:
                        out["steps"].append(REJECTED)
                        radius /= dec
                        dec *= 2.0
        finalize(fresh and term is None)
        out["costs"].append(cost)
    out.update(success=term != FAILURE, termination=term, num_iterations=it, num_successful_steps=n_succ,
               num_invalid_steps=n_inv_total, final_cost=cost, qvec=q, tvec=t, camera_params=prm)
    return out


def is_clear(margins, bar=CLEAR_MARGIN):
    return all(m >= bar for m in margins)


def stable_under_rounding(args, opts, out=None, tol=1e-10):
    """DESIGN.md 12's conditioning probe: the same run with the scaled system of every solve perturbed by 1e-15 relative must
    reproduce every decision and the cost after every iteration to `tol`."""
    a = out if out is not None else refine(*args, opts=opts)
    b = refine(*args, opts=opts, perturb=1e-15)
    if a["steps"] != b["steps"] or a["termination"] != b["termination"]:
        return False
    ca, cb = np.array(a["costs"]), np.array(b["costs"])
    return bool(np.all(np.abs(ca - cb) <= tol * np.abs(ca)))


def cauchy_cost(cam, xy, X, mask, qvec, tvec, scale=1.0):
    """1/2 sum rho(|r|^2) of a pose, in plain numpy sums (what the chain test compares)."""
    model, params = (cam.model_id, list(cam.params)) if hasattr(cam, "model_id") else cam
    q = np.asarray(qvec, np.float64)
    q = q / np.linalg.norm(q)
    prm = np.zeros(12)
    prm[:len(params)] = np.asarray(params, np.float64)[:12]
    m = np.asarray(mask, bool)
    w = quat_rotate(np.tile(q, (int(m.sum()), 1)), np.asarray(X, np.float64).reshape(-1, 3)[m]) + np.asarray(tvec, np.float64)
    x, y, _, _ = project_with_jacobian(model, list(prm[:NUM_PARAMS[model]]), w[:, 0] / w[:, 2], w[:, 1] / w[:, 2])
    xy = np.asarray(xy, np.float64).reshape(-1, 2)[m]
    s = (x - xy[:, 0]) ** 2 + (y - xy[:, 1]) ** 2
    return float(0.5 * cauchy(s, scale * scale)[0].sum())


def scipy_optimum(cam, xy, X, mask, qvec, tvec, flags, scale=1.0):
    """An independent minimum of the same cost: scipy.optimize.least_squares(loss='cauchy') over the same free tangent columns.
    scipy applies its loss to every scalar residual, Ceres to the squared norm of the 2-vector block, so scipy is given one scalar
    per point, |r_i|: then 1/2 scale^2 sum log(1 + (|r_i| / scale)^2) is the cost above."""
    from scipy.optimize import least_squares
    model, params = (cam.model_id, list(cam.params)) if hasattr(cam, "model_id") else cam
    free = free_indices(model, flags)
    q0 = np.asarray(qvec, np.float64)
    q0 = q0 / np.linalg.norm(q0)
    t0 = np.asarray(tvec, np.float64)
    prm0 = np.zeros(12)
    prm0[:len(params)] = np.asarray(params, np.float64)[:12]
    m = np.asarray(mask, bool)
    Xi, xyi = np.asarray(X, np.float64).reshape(-1, 3)[m], np.asarray(xy, np.float64).reshape(-1, 2)[m]
    sc = np.array([1.0] * 6 + [max(abs(prm0[j]), 1e-2) for j in free])

    def f(d):
        d = d * sc
        q = quat_plus(q0, d[:3])[0]
        prm = prm0.copy()
        for j, pj in enumerate(free):
            prm[pj] = prm0[pj] + d[6 + j]
        w = quat_rotate(np.tile(q, (len(Xi), 1)), Xi) + (t0 + d[3:6])
        x, y, _, _ = project_with_jacobian(model, list(prm[:NUM_PARAMS[model]]), w[:, 0] / w[:, 2], w[:, 1] / w[:, 2])
        return np.sqrt((x - xyi[:, 0]) ** 2 + (y - xyi[:, 1]) ** 2)

    sol = least_squares(f, np.zeros(6 + len(free)), loss="cauchy", f_scale=scale, method="trf", x_scale="jac", xtol=1e-13, ftol=1e-13,
                        gtol=1e-13, max_nfev=5000)
    return float(sol.cost)
