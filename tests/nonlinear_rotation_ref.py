"""numpy restatement of GlobalRotationAveraging() with the NONLINEAR estimator (dsm_view_graph_rotation_averaging_nonlinear,
DESIGN.md 20): the largest component, NonlinearRotationEstimator (one PairwiseRotationError per edge under one SoftLOneLoss,
ceres' Levenberg-Marquardt by DESIGN.md 12's rulings), FilterViewPairsFromOrientation, the largest component of what survives.

The residual is differentiated by forward-mode dual numbers (the `Dual` class of bundle_adjustment_ref) through ceres' three
conversions; a dual number branches on its value part, so the derivative is that of the branch that is evaluated.  Rows are
vectorised: every branch is evaluated on a safe argument and selected per row.  `WideDual` is the same algebra in any dtype
(numpy.longdouble measures the rounding scale of these formulas).  The linear system (J^T J + D / radius) step = -g is solved
densely; the device solves it by a preconditioned conjugate gradient.  The cost is invariant under one rotation applied to
every image and nothing holds that gauge, so two solvers agree on R_v R_v0^T and on edge rotations, not on the orientations."""
import numpy as np
import scipy.sparse as sp

from tests import rotation_averaging_ref as ra
from tests.bundle_adjustment_ref import CONVERGENCE, FAILURE, NO_CONVERGENCE, Dual, margin

MIN_RADIUS = 1e-32
DEFAULTS = dict(robust_loss_width=0.1, max_num_iterations=200, max_num_consecutive_invalid_steps=5, function_tolerance=1e-6,
                gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_trust_region_radius=1e4, max_trust_region_radius=1e16,
                min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_relative_rotation_difference_degrees=5.0)


# ---------------------------------------------------------------- dual numbers in any dtype
class WideDual(Dual):
    """bundle_adjustment_ref.Dual without the cast to float64: value [n], derivatives [n, K] in the dtype they come in."""

    def __init__(self, v, d):
        self.v, self.d = np.asarray(v), np.asarray(d)

    def _lift(self, x):
        if isinstance(x, Dual):
            return x
        return WideDual(np.broadcast_to(np.asarray(x, self.v.dtype), self.v.shape), np.zeros_like(self.d))

    def __add__(self, o):
        o = self._lift(o)
        return WideDual(self.v + o.v, self.d + o.d)

    __radd__ = __add__

    def __sub__(self, o):
        o = self._lift(o)
        return WideDual(self.v - o.v, self.d - o.d)

    def __rsub__(self, o):
        return self._lift(o) - self

    def __neg__(self):
        return WideDual(-self.v, -self.d)

    def __mul__(self, o):
        o = self._lift(o)
        return WideDual(self.v * o.v, self.d * o.v[:, None] + self.v[:, None] * o.d)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = self._lift(o)
        r = self.v / o.v
        return WideDual(r, (self.d - r[:, None] * o.d) / o.v[:, None])

    def __rtruediv__(self, o):
        return self._lift(o) / self


def _chain(a, f, df):
    return type(a)(f, df[:, None] * a.d)


def _sqrt(a):
    s = np.sqrt(a.v)
    return _chain(a, s, 0.5 / s)


def _atan2(y, x):
    den = x.v * x.v + y.v * y.v
    return type(y)(np.arctan2(y.v, x.v), (x.v[:, None] * y.d - y.v[:, None] * x.d) / den[:, None])


def _where(m, a, b):
    return type(a)(np.where(m, a.v, b.v), np.where(m[:, None], a.d, b.d))


def _const(like, c):
    return type(like)(np.full(like.v.shape, c, like.v.dtype), np.zeros_like(like.d))


# ---------------------------------------------------------------- ceres' conversions over duals (rows; R[i][j])
def angle_axis_to_rotation_dual(aa):
    th2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2]
    big = th2.v > np.finfo(np.float64).eps
    one = _const(th2, 1.0)
    th = _sqrt(_where(big, th2, one))
    wx, wy, wz = aa[0] / th, aa[1] / th, aa[2] / th
    c, s = _chain(th, np.cos(th.v), -np.sin(th.v)), _chain(th, np.sin(th.v), np.cos(th.v))
    omc = 1.0 - c
    B = [[c + wx * wx * omc, wx * wy * omc - wz * s, wy * s + wx * wz * omc],
         [wz * s + wx * wy * omc, c + wy * wy * omc, -(wx * s) + wy * wz * omc],
         [-(wy * s) + wx * wz * omc, wx * s + wy * wz * omc, c + wz * wz * omc]]
    S = [[one, -aa[2], aa[1]], [aa[2], one, -aa[0]], [-aa[1], aa[0], one]]  # I + [w]x: its own derivative, not the limit
    return [[_where(big, B[i][j], S[i][j]) for j in range(3)] for i in range(3)]


def rotation_to_quaternion_dual(R):
    tr = R[0][0] + R[1][1] + R[2][2]
    pos = tr.v >= 0.0
    one = _const(tr, 1.0)
    t = _sqrt(_where(pos, tr + 1.0, one))
    t2 = 0.5 / t
    q = [t * 0.5, (R[2][1] - R[1][2]) * t2, (R[0][2] - R[2][0]) * t2, (R[1][0] - R[0][1]) * t2]
    i = np.where(R[1][1].v > R[0][0].v, 1, 0)
    dv = np.stack([R[0][0].v, R[1][1].v, R[2][2].v], 1)
    i = np.where(R[2][2].v > dv[np.arange(len(i)), i], 2, i)
    for b in range(3):
        m = ~pos & (i == b)
        if not m.any():
            continue
        j, k = (b + 1) % 3, (b + 2) % 3
        t = _sqrt(_where(m, R[b][b] - R[j][j] - R[k][k] + 1.0, one))
        t2 = 0.5 / t
        alt = [None] * 4
        alt[b + 1] = t * 0.5
        alt[0] = (R[k][j] - R[j][k]) * t2
        alt[j + 1] = (R[j][b] + R[b][j]) * t2
        alt[k + 1] = (R[k][b] + R[b][k]) * t2
        q = [_where(m, alt[c], q[c]) for c in range(4)]
    return q


def quaternion_to_angle_axis_dual(q):
    s2 = q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    pos = s2.v > 0.0
    st = _sqrt(_where(pos, s2, _const(s2, 1.0)))
    neg = q[0].v < 0.0
    two = _where(neg, _atan2(-st, -q[0]), _atan2(st, q[0])) * 2.0
    k = _where(pos, two / st, _const(s2, 2.0))
    return [q[1] * k, q[2] * k, q[3] * k]


def _matmul_t(A, B):
    """A B^T, the sums left to right"""
    return [[A[i][0] * B[j][0] + A[i][1] * B[j][1] + A[i][2] * B[j][2] for j in range(3)] for i in range(3)]


def soft_l1(s, width):
    """ceres::SoftLOneLoss(width) at s: rho, rho', rho'' [n, 3]"""
    b = width * width
    total = 1.0 + s / b
    tmp = np.sqrt(total)
    rho1 = np.maximum(np.finfo(np.float64).tiny, 1.0 / tmp)
    return np.stack([2.0 * b * (tmp - 1.0), rho1, -(rho1 / b) / (2.0 * total)], 1)


def corrector(sq_norm, rho):
    """ceres' Corrector in full: (residual_scaling, alpha_sq_norm, first_branch).  The Jacobian becomes
    sqrt(rho') (J - alpha_sq_norm r r^T J), the residual residual_scaling r."""
    sqrt_rho1 = np.sqrt(rho[:, 1])
    first = (sq_norm == 0.0) | (rho[:, 2] <= 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        D = 1.0 + 2.0 * sq_norm * rho[:, 2] / rho[:, 1]
        alpha = 1.0 - np.sqrt(D)
        scaling = np.where(first, sqrt_rho1, sqrt_rho1 / (1.0 - alpha))
        alpha_sq = np.where(first, 0.0, alpha / sq_norm)
    return scaling, alpha_sq, first


def pairwise_rotation_error(a1, a2, a12, width=0.1, dtype=np.float64, corrected=True):
    """PairwiseRotationError (weight 1) on rows of angle-axis triples: (residuals [n, 3], jacobians [n, 2, 3, 3] with respect to
    rotation 1 and rotation 2, rho [n, 3] at the uncorrected |r|^2); corrected: after the loss corrector."""
    a1, a2, a12 = (np.asarray(v, dtype).reshape(-1, 3) for v in (a1, a2, a12))
    n = len(a1)
    cls = Dual if dtype == np.float64 else WideDual
    eye = np.eye(6, dtype=dtype)
    w1 = [cls(a1[:, c].copy(), np.tile(eye[c], (n, 1))) for c in range(3)]
    w2 = [cls(a2[:, c].copy(), np.tile(eye[3 + c], (n, 1))) for c in range(3)]
    w12 = [cls(a12[:, c].copy(), np.zeros((n, 6), dtype)) for c in range(3)]
    with np.errstate(invalid="ignore", divide="ignore"):
        M1, M2, M12 = (angle_axis_to_rotation_dual(w) for w in (w1, w2, w12))
        err = _matmul_t(_matmul_t(M2, M1), M12)
        aa = quaternion_to_angle_axis_dual(rotation_to_quaternion_dual(err))
    r = np.stack([c.v for c in aa], 1)
    J = np.stack([c.d for c in aa], 1)  # [n, 3, 6]
    s = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
    rho = soft_l1(s, dtype(width))
    if corrected:
        scaling, alpha_sq, _ = corrector(s, rho)
        sq1 = np.sqrt(rho[:, 1])
        rtJ = np.einsum("nr,nrc->nc", r, J)
        J = sq1[:, None, None] * (J - alpha_sq[:, None, None] * r[:, :, None] * rtJ[:, None, :])
        r = scaling[:, None] * r
    return r, np.stack([J[:, :, :3], J[:, :, 3:]], 1), rho


# ---------------------------------------------------------------- the call
def _graph(pairs, qvecs, use):
    """Step 1 as rotation_averaging_ref.rotation_averaging builds it: unique used edges (the first occurrence wins), the first
    component; component indices ascend with image id."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    qvecs = np.asarray(qvecs, np.float64).reshape(-1, 4)
    n = len(pairs)
    used = np.ones(n, bool) if use is None else np.asarray(use).astype(bool)
    state = np.zeros(n, np.uint8)
    seen, uniq = set(), []
    for e in np.nonzero(used)[0]:
        a, b = int(pairs[e, 0]), int(pairs[e, 1])
        if a == b:
            raise ValueError("image_id1 == image_id2")
        key = (min(a, b), max(a, b))
        if key not in seen:
            seen.add(key)
            uniq.append(e)
    if not uniq:
        return None, state
    uniq = np.array(uniq)
    ids = np.unique(pairs[uniq].reshape(-1))
    vi, vj = np.searchsorted(ids, pairs[uniq, 0]), np.searchsorted(ids, pairs[uniq, 1])
    in1, n_comp = ra.largest_component(len(ids), zip(vi, vj))
    inside = in1[vi]
    state[uniq[~inside]] = 1
    cidx = np.cumsum(in1) - 1
    E = uniq[inside]
    ei, ej = cidx[vi[inside]], cidx[vj[inside]]
    # the canonical block order: (lo, hi)
    o = np.lexsort((np.maximum(ei, ej), np.minimum(ei, ej)))
    E, ei, ej = E[o], ei[o], ej[o]
    return dict(cimg=ids[in1], E=E, ei=ei, ej=ej, r12=ra.quaternion_to_angle_axis(qvecs[E]), n_comp=n_comp), state


def rotation_averaging_nonlinear(pairs, qvecs, use=None, initial=None, options=None, perturb=0.0):
    """Returns a dict shaped like capi.Context.rotation_averaging_nonlinear (report: a dict) plus `accepted` (per LM
    iteration) and `margins`.  perturb > 0: J^T J and g of every solve carry a seeded relative perturbation of that size."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    n = len(np.asarray(pairs).reshape(-1, 2))
    rel_out = np.zeros((n, 3))
    g, state = _graph(pairs, qvecs, use)
    rep = {"num_components": 0, "num_images": 0, "num_edges": 0, "termination": NO_CONVERGENCE, "num_iterations": 0,
           "num_successful_steps": 0, "num_rejected_steps": 0, "num_invalid_steps": 0, "num_filtered_edges": 0, "num_final_images": 0,
           "initial_cost": 0.0, "final_cost": 0.0}
    if g is None:
        return {"image_ids": np.zeros(0, np.uint32), "orientations": np.zeros((0, 3)), "in_final_cc": np.zeros(0, bool),
                "edge_state": state, "relative_rotations": rel_out, "report": rep, "trace": np.zeros((0, 6)), "accepted": [],
                "margins": {}}
    cimg, E, ei, ej, r12 = g["cimg"], g["E"], g["ei"], g["ej"], g["r12"]
    N, M = len(cimg), len(E)
    rep.update(num_components=g["n_comp"], num_images=N, num_edges=M)
    R = np.zeros((N, 3))
    if initial is not None:
        iid = np.asarray(initial["image_ids"], np.int64)
        pos = np.searchsorted(iid, cimg)
        if np.any(np.diff(iid) <= 0) or np.any(pos >= len(iid)) or np.any(iid[np.minimum(pos, len(iid) - 1)] != cimg):
            raise ValueError("initial does not cover the component")
        R = np.asarray(initial["orientations"], np.float64).reshape(-1, 3)[pos].copy()
    width = opt["robust_loss_width"]
    rows = (3 * np.arange(M)[:, None, None] + np.arange(3)[None, :, None]) + np.zeros((1, 1, 3), np.int64)
    cols = np.concatenate([(3 * ei[:, None, None] + np.arange(3)[None, None, :]) + np.zeros((1, 3, 1), np.int64),
                           (3 * ej[:, None, None] + np.arange(3)[None, None, :]) + np.zeros((1, 3, 1), np.int64)]).reshape(-1)
    rows = np.concatenate([rows, rows]).reshape(-1)

    def evaluate(R, first, s):
        r, J, rho = pairwise_rotation_error(R[ei], R[ej], r12, width)
        Jm = sp.csr_matrix((np.concatenate([J[:, 0].reshape(-1), J[:, 1].reshape(-1)]), (rows, cols)), shape=(3 * M, 3 * N))
        rv = r.reshape(-1)
        grad = Jm.T @ rv
        cn = np.asarray(Jm.multiply(Jm).sum(0)).reshape(-1)
        if first:
            s = 1.0 / (1.0 + np.sqrt(cn))
        Js = Jm @ sp.diags(s)
        D = np.clip(s * s * cn, opt["min_lm_diagonal"], opt["max_lm_diagonal"])
        return rv, Js, s * grad, D, float(np.max(np.abs(grad), initial=0.0)), s, float(0.5 * rho[:, 0].sum())

    def cost_of(R):
        return float(0.5 * pairwise_rotation_error(R[ei], R[ej], r12, width)[2][:, 0].sum())

    margins = {"rho": np.inf, "gradient": np.inf, "function": np.inf}
    rv, Js, gs, D, gnorm, s, cost = evaluate(R, True, None)
    rep["initial_cost"] = cost
    radius, dec = opt["initial_trust_region_radius"], 2.0
    it = n_invalid = 0
    trace, acc_list = [], []
    term = None

    def finalize(fresh, rho_lm, accepted):
        nonlocal term
        if term is None:
            if it >= opt["max_num_iterations"]:
                term = NO_CONVERGENCE
            elif fresh:
                margins["gradient"] = min(margins["gradient"], margin(gnorm, opt["gradient_tolerance"]))
                if gnorm <= opt["gradient_tolerance"]:
                    term = CONVERGENCE
            if term is None and radius < MIN_RADIUS:
                term = CONVERGENCE
        trace.append([cost, radius, rho_lm, 0, accepted, gnorm])

    if not np.isfinite(cost):
        term = FAILURE
        trace.append([cost, radius, np.nan, 0, 1, gnorm])
    else:
        finalize(True, np.nan, 1)
    while term is None:
        lm2 = np.sqrt(D / radius) ** 2
        A = (Js.T @ Js).toarray()
        b = -gs
        if perturb > 0.0:
            rng = np.random.default_rng(it)
            A = A * (1.0 + perturb * rng.standard_normal(A.shape))
            A = (A + A.T) / 2.0
            b = b * (1.0 + perturb * rng.standard_normal(b.shape))
        step = np.linalg.solve(A + np.diag(lm2), b)
        js = Js @ step
        mcc = -float((js * (rv + js / 2.0)).sum())
        delta = s * step
        cand = R + delta.reshape(N, 3)
        cand_cost = cost_of(cand)
        it += 1
        accepted, rho_lm = 0, np.nan
        s2 = float(delta @ delta)
        if not (np.isfinite(mcc) and mcc > 0.0 and np.isfinite(s2) and np.isfinite(cand_cost)):
            n_invalid += 1
            rep["num_invalid_steps"] += 1
            if n_invalid >= opt["max_num_consecutive_invalid_steps"]:
                term = FAILURE
            else:
                radius /= dec
                dec *= 2.0
        else:
            n_invalid = 0
            if np.sqrt(s2) <= opt["parameter_tolerance"] * (np.sqrt(float((R * R).sum())) + opt["parameter_tolerance"]):
                term = CONVERGENCE
            else:
                margins["function"] = min(margins["function"], margin(abs(cost - cand_cost), opt["function_tolerance"] * cost))
                if abs(cost - cand_cost) <= opt["function_tolerance"] * cost:
                    term = CONVERGENCE
                else:
                    rho_lm = (cost - cand_cost) / mcc
                    margins["rho"] = min(margins["rho"], abs((cost - cand_cost) - opt["min_relative_decrease"] * mcc) /
                                         max(cost, np.finfo(float).tiny))
                    if rho_lm > opt["min_relative_decrease"]:
                        accepted = 1
                        rep["num_successful_steps"] += 1
                        R = cand
                        tmp = 2.0 * rho_lm - 1.0
                        radius = min(opt["max_trust_region_radius"], radius / max(1.0 / 3.0, 1.0 - tmp ** 3))
                        dec = 2.0
                        rv, Js, gs, D, gnorm, s, cost = evaluate(R, False, s)
                    else:
                        rep["num_rejected_steps"] += 1
                        radius /= dec
                        dec *= 2.0
        acc_list.append(accepted)
        finalize(bool(accepted), rho_lm, accepted)
    rep.update(termination=term, num_iterations=it, final_cost=cost, final_trust_region_radius=radius,
               min_rho_margin=margins["rho"], min_gradient_margin=margins["gradient"], min_function_margin=margins["function"])
    # steps 3 and 4 (rotation_averaging_ref)
    thr = opt["max_relative_rotation_difference_degrees"] * ra.DEG2RAD
    loop = ra.multiply_rotations(-r12, ra.multiply_rotations(R[ej], -R[ei]))
    sq = np.sum(loop * loop, axis=1)
    keep = sq <= thr * thr
    state[E] = np.where(keep, 3, 2)
    Ri, Rj = ra.angle_axis_to_rotation(R[ei]), ra.angle_axis_to_rotation(R[ej])
    rel = ra.rotation_to_angle_axis(np.matmul(Rj, np.transpose(Ri, (0, 2, 1))))
    rel_out[E[keep]] = rel[keep]
    rep["num_filtered_edges"] = int((~keep).sum())
    fin, _ = ra.largest_component(N, zip(ei[keep], ej[keep]))
    rep["num_final_images"] = int(fin.sum())
    margins["filter"] = float(np.min(np.abs(sq - thr * thr) / (thr * thr))) if thr > 0 else np.inf
    return {"image_ids": cimg.astype(np.uint32), "orientations": R, "in_final_cc": fin, "edge_state": state,
            "relative_rotations": rel_out, "report": rep, "trace": np.array(trace, np.float64), "accepted": acc_list, "margins": margins}


def relative_to_first(orientations):
    """R_v R_v0^T as angle-axis: the orientations with the gauge taken out (v0: the component's smallest image id)."""
    Rm = ra.angle_axis_to_rotation(orientations)
    return ra.rotation_to_angle_axis(np.matmul(Rm, Rm[0].T[None]))


def clear_by_margins(out, margin=1e-9, filter_margin=1e-6):
    """No decision of the run sits at its threshold: the LM margins (function and gradient relative, the acceptance margin in
    cost) against `margin`, the filter's (relative to the squared threshold) against `filter_margin`."""
    m = out["margins"]
    return all(v >= margin for k, v in m.items() if k != "filter") and m.get("filter", np.inf) >= filter_margin


PROBE_TOL = 3e-10


def stable_under_rounding(pairs, qvecs, use=None, initial=None, options=None, out=None, tol=PROBE_TOL):
    """The conditioning probe: the restatement again with J^T J and g perturbed by 1e-15 relative must reproduce
    every decision and the cost trace to `tol`.  The device's trace is held to 1e-9; the probe is three times tighter, so a scene
    that passes it leaves the device a margin of 7e-10 for its own rounding.  DESIGN.md 12 probes to 1e-10; that does not hold
    here: the damped system is singular but for D / radius, a 1e-15 change of it moves the step by 1e-15 times a
    condition number of 1e6 to 4e7, and the restatement's own trace moves by up to 2e-10 on the scenes of the device tests."""
    a = out if out is not None else rotation_averaging_nonlinear(pairs, qvecs, use, initial, options)
    b = rotation_averaging_nonlinear(pairs, qvecs, use, initial, options, perturb=1e-15)
    if a["accepted"] != b["accepted"] or a["report"]["termination"] != b["report"]["termination"]:
        return False
    if not np.array_equal(a["edge_state"], b["edge_state"]):
        return False
    ta, tb = a["trace"][:, 0], b["trace"][:, 0]
    return bool(np.all(np.abs(ta - tb) <= tol * np.abs(ta)))


def scipy_optimum(pairs, qvecs, start, use=None, width=0.1):
    """scipy.optimize.least_squares(loss="soft_l1", f_scale=width) over the same cost from `start` (orientations [N, 3] of the
    first component): one residual |r_e| per edge, so that scipy's per-residual loss is ceres' per-block loss.  Returns the
    final cost 1/2 sum rho(|r_e|^2)."""
    from scipy.optimize import least_squares
    g, _ = _graph(pairs, qvecs, use)
    ei, ej, r12, N = g["ei"], g["ej"], g["r12"], len(g["cimg"])

    def fun(x):
        R = x.reshape(N, 3)
        r = pairwise_rotation_error(R[ei], R[ej], r12, width, corrected=False)[0]
        return np.sqrt((r * r).sum(1))

    sol = least_squares(fun, np.asarray(start, np.float64).reshape(-1), method="trf", loss="soft_l1", f_scale=width, xtol=1e-15,
                        ftol=1e-15, gtol=1e-15, max_nfev=200)
    return float(sol.cost)
