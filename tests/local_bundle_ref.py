"""A sequential numpy restatement of dsm_adjust_local_bundles in the device's summation order: the canonical
order of a problem (points by id, images by content, cameras by first use), the loss with Ceres' corrector stated in full, the
explicit reduced camera system, the right-looking Cholesky, the fixed-order workgroup sums.  The projection, the problem's
blocks and `Plus` are bundle_adjustment_ref's.  Every decision margin is recorded."""
import numpy as np

from tests.bundle_adjustment_ref import (CONVERGENCE, FAILURE, MAX_DIAG, MAX_RADIUS, MIN_DIAG, MIN_RADIUS, MIN_REL_DECREASE,
                                         NO_CONVERGENCE, NUM_PARAMS, TWO_FOCAL, Problem, margin, project_with_jacobian, quat_matrix,
                                         quat_plus, quat_rotate)

LOSS_TRIVIAL, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2
MAX_REDUCED_DIM = 128
DEFAULTS = dict(max_num_iterations=25, max_num_consecutive_invalid_steps=10, gradient_tolerance=10.0, function_tolerance=0.0,
                parameter_tolerance=0.0, refine_focal_length=1, refine_principal_point=0, refine_extra_params=1,
                loss_function_type=LOSS_SOFT_L1, loss_function_scale=1.0)
TINY = np.finfo(np.float64).tiny
T = 256  # threads of the device's workgroup


def loss(kind, scale, s):
    """rho(s), rho'(s), rho''(s) of ceres::TrivialLoss / SoftLOneLoss / CauchyLoss for s [n]."""
    b = scale * scale
    c = 1.0 / b
    if kind == LOSS_TRIVIAL:
        return s.copy(), np.ones_like(s), np.zeros_like(s)
    total = 1.0 + s * c
    if kind == LOSS_SOFT_L1:
        tmp = np.sqrt(total)
        r1 = np.maximum(TINY, 1.0 / tmp)
        return 2.0 * b * (tmp - 1.0), r1, -(c * r1) / (2.0 * total)
    if kind == LOSS_CAUCHY:
        inv = 1.0 / total
        return b * np.log(total), np.maximum(TINY, inv), -c * (inv * inv)
    raise ValueError(kind)


def corrector(sq_norm, rho1, rho2):
    """ceres::internal::Corrector's constructor in full: (sqrt_rho1, residual_scaling, alpha_sq_norm, branch) per residual
    block.  Branch 1 (rho'' <= 0, or a zero residual): residuals and Jacobian rows are both scaled by sqrt(rho'); branch 2
    solves 1/2 alpha^2 - alpha - rho''/rho' s = 0 and additionally projects the Jacobian."""
    sqrt_rho1 = np.sqrt(rho1)
    first = (sq_norm == 0.0) | (rho2 <= 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        D = 1.0 + 2.0 * sq_norm * rho2 / rho1
        alpha = 1.0 - np.sqrt(np.maximum(D, 0.0))
        scaling2 = sqrt_rho1 / (1.0 - alpha)
        asn2 = alpha / sq_norm
    return sqrt_rho1, np.where(first, sqrt_rho1, scaling2), np.where(first, 0.0, asn2), np.where(first, 1, 2)


def block_sum(vals):
    """The workgroup's fixed-order sum: thread t adds its elements t, t + 256, ... in order; the xor butterfly 32 .. 1 inside
    each wave of 64; then ((w0 + w1) + w2) + w3."""
    vals = np.asarray(vals, np.float64)
    acc = np.zeros(T)
    for k in range(0, len(vals), T):
        chunk = vals[k:k + T]
        acc[:len(chunk)] += chunk
    return butterfly(acc)


def butterfly(acc):
    idx = np.arange(T)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[idx ^ o]
    return float(((acc[0] + acc[64]) + acc[128]) + acc[192])


def canonical(scene):
    """The problem in the device's canonical order: points with an observation by id, images with an observation by content
    (flags, pose bits, the camera's model / constancy / parameter bits, then the observations by point rank), cameras by first
    use, each track by canonical image.  Returns (scene', image_index, camera_index, point_index) into the input."""
    models = np.asarray(scene["camera_model_ids"], np.int64).reshape(-1)
    C = len(models)
    poff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in models])]).astype(np.int64)
    prm = np.asarray(scene["camera_params"], np.float64).reshape(-1)
    icam = np.asarray(scene["image_camera"], np.int64).reshape(-1)
    N = len(icam)
    q = np.asarray(scene["qvec"], np.float64).reshape(N, 4)
    t = np.asarray(scene["tvec"], np.float64).reshape(N, 3)
    toff = np.asarray(scene["track_offsets"], np.int64).reshape(-1)
    P = len(toff) - 1
    oimg = np.asarray(scene["obs_image"], np.int64).reshape(-1)
    oxy = np.asarray(scene["obs_xy"], np.float64).reshape(-1, 2)
    flag = lambda k, n: np.zeros(n, np.uint8) if scene.get(k) is None else np.asarray(scene[k], np.uint8).reshape(n)
    cpose, cmask, pconst, cconst = flag("image_constant_pose", N), flag("image_constant_tvec", N), flag("point_constant", P), flag("camera_constant", C)
    ids = np.arange(P, dtype=np.uint64) if scene.get("point_ids") is None else np.asarray(scene["point_ids"], np.uint64).reshape(-1)
    porder = np.argsort(ids, kind="stable")
    assert len(np.unique(ids)) == P, "a repeated point id"
    prank = np.empty(P, np.int64)
    prank[porder] = np.arange(P)
    bits = lambda x: [int(b) for b in np.asarray(x, np.float64).reshape(-1).view(np.uint64)]
    iobs = [[] for _ in range(N)]
    for p in range(P):
        for k in range(toff[p], toff[p + 1]):
            iobs[oimg[k]].append((int(prank[p]), int(k)))
    keys = {}
    for i in range(N):
        if not iobs[i]:
            continue
        iobs[i].sort()
        assert len({r for r, _ in iobs[i]}) == len(iobs[i]), "one image observes one point twice"
        c = icam[i]
        key = [int(cpose[i] != 0), int(cmask[i])] + bits(q[i]) + bits(t[i]) + [int(models[c]), int(cconst[c] != 0)] + bits(prm[poff[c]:poff[c + 1]])
        for r, k in iobs[i]:
            key += [r] + bits(oxy[k])
        keys[i] = key
    iorder = sorted(keys, key=lambda i: keys[i])
    inew = {i: r for r, i in enumerate(iorder)}
    corder = []
    for i in iorder:
        if icam[i] not in corder:
            corder.append(int(icam[i]))
    cnew = {c: r for r, c in enumerate(corder)}
    pts = [int(p) for p in porder if toff[p + 1] > toff[p]]
    tracks = [sorted((inew[int(oimg[k])], int(k)) for k in range(toff[p], toff[p + 1])) for p in pts]
    out = {"camera_model_ids": models[corder].astype(np.int32),
           "camera_params": np.concatenate([prm[poff[c]:poff[c + 1]] for c in corder]) if corder else np.zeros(0),
           "camera_constant": cconst[corder], "image_camera": np.array([cnew[int(icam[i])] for i in iorder], np.uint32),
           "qvec": q[iorder].copy(), "tvec": t[iorder].copy(), "image_constant_pose": cpose[iorder], "image_constant_tvec": cmask[iorder],
           "point_ids": ids[pts], "xyz": np.asarray(scene["xyz"], np.float64).reshape(-1, 3)[pts].copy(), "point_constant": pconst[pts],
           "track_offsets": np.concatenate([[0], np.cumsum([len(tr) for tr in tracks])]).astype(np.uint32),
           "obs_image": np.array([i for tr in tracks for i, _ in tr], np.uint32),
           "obs_xy": oxy[[k for tr in tracks for _, k in tr]].reshape(-1, 2)}
    return out, np.array(iorder, np.int64), np.array(corder, np.int64), np.array(pts, np.int64)


class LocalProblem(Problem):
    """bundle_adjustment_ref.Problem with camera_constant: such a camera has no free index whatever the refine flags say."""

    def __init__(self, scene, opt):
        super().__init__(scene, opt)
        cc = scene.get("camera_constant")
        if cc is not None:
            for c in np.nonzero(np.asarray(cc).reshape(-1))[0]:
                self.cam_free[c] = []
        col = self.ne + int((self.qcol >= 0).sum() + (self.tcol >= 0).sum())
        self.ccol = []
        for free in self.cam_free:
            self.ccol.append(np.arange(col, col + len(free)))
            col += len(free)
        self.nf = col - self.ne
        self.cam_var = np.array([len(f) > 0 for f in self.cam_free], bool)
        # the 18 f slots of every observation: qvec 3, tvec 3, the camera's free parameters; -1 = constant.  Columns count
        # from 0 inside the reduced system
        self.fcol = -np.ones((self.n, 18), np.int64)
        oi = self.obs_img
        self.fcol[:, 0:3] = np.where(self.qcol[oi] >= 0, self.qcol[oi] - self.ne, -1)
        self.fcol[:, 3:6] = np.where(self.tcol[oi] >= 0, self.tcol[oi] - self.ne, -1)
        for o in range(self.n):
            cols = self.ccol[self.icam[oi[o]]]
            self.fcol[o, 6:6 + len(cols)] = cols - self.ne

    def rows(self, st, kind, scale):
        """Per observation: residual r [n, 2], rho [n], and the corrected E [n, 2, 3], F [n, 2, 18], r [n, 2]."""
        q, t, X, prm = st["qvec"], st["tvec"], st["xyz"], st["camera_params"]
        oi, op = self.obs_img, self.obs_pt
        w = quat_rotate(q[oi], X[op])
        Pc = w + t[oi]
        u, v = Pc[:, 0] / Pc[:, 2], Pc[:, 1] / Pc[:, 2]
        n = self.n
        r, E, F = np.zeros((n, 2)), np.zeros((n, 2, 3)), np.zeros((n, 2, 18))
        for c in np.unique(self.icam[oi]) if n else []:
            sel = np.nonzero(self.icam[oi] == c)[0]
            x, y, dx, dy = project_with_jacobian(self.models[c], prm[self.poff[c]:self.poff[c + 1]], u[sel], v[sel])
            r[sel, 0], r[sel, 1] = x - self.obs_xy[sel, 0], y - self.obs_xy[sel, 1]
            z = Pc[sel, 2]
            iz = 1.0 / z
            duP = np.stack([iz, 0.0 * z, -Pc[sel, 0] * iz * iz], 1)
            dvP = np.stack([0.0 * z, iz, -Pc[sel, 1] * iz * iz], 1)
            JP = np.stack([dx[:, :1] * duP + dx[:, 1:2] * dvP, dy[:, :1] * duP + dy[:, 1:2] * dvP], 1)
            R = quat_matrix(q[oi[sel]])
            ws, Z = w[sel], np.zeros(len(sel))
            Dq = 2.0 * np.stack([np.stack([Z, ws[:, 2], -ws[:, 1]], 1), np.stack([-ws[:, 2], Z, ws[:, 0]], 1), np.stack([ws[:, 1], -ws[:, 0], Z], 1)], 1)
            mm = lambda A, B: (A[:, :, 0:1] * B[:, 0:1, :] + A[:, :, 1:2] * B[:, 1:2, :]) + A[:, :, 2:3] * B[:, 2:3, :]
            E[sel] = mm(JP, R)
            F[sel, :, 0:3] = mm(JP, Dq)
            F[sel, :, 3:6] = JP
            for jj, pj in enumerate(self.cam_free[c]):
                F[sel, 0, 6 + jj], F[sel, 1, 6 + jj] = dx[:, 2 + pj], dy[:, 2 + pj]
        s = r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]
        rho, rho1, rho2 = loss(kind, scale, s)
        if kind == LOSS_TRIVIAL:
            return r, rho, E, F, r.copy(), np.ones(n, np.int64)
        sq, scaling, asn, branch = corrector(s, rho1, rho2)
        assert (branch == 1).all(), "the restatement implements the corrector's first branch only"
        return r, rho, sq[:, None, None] * E, sq[:, None, None] * F, scaling[:, None] * r, branch


def _cholesky(S, margins):
    """S = U'U right-looking, the upper triangle in place; None when a pivot is not positive and finite."""
    R = len(S)
    U = np.triu(S).copy()
    diag = np.diag(S).copy()
    for j in range(R):
        pv = U[j, j]
        margins["pivot"] = min(margins["pivot"], abs(pv) / diag[j] if np.isfinite(pv) and diag[j] > 0.0 else 0.0)
        if not (pv > 0.0 and np.isfinite(pv)):
            return None
        u = np.sqrt(pv)
        U[j, j] = u
        U[j, j + 1:] = U[j, j + 1:] / u
        U[j + 1:, j + 1:] -= np.triu(np.outer(U[j, j + 1:], U[j, j + 1:]))
    return U


def _solve(U, b):
    R = len(b)
    x = b.copy()
    for j in range(R):
        x[j] = x[j] / U[j, j]
        x[j + 1:] -= U[j, j + 1:] * x[j]
    for j in range(R - 1, -1, -1):
        x[j] = x[j] / U[j, j]
        x[:j] -= U[:j, j] * x[j]
    return x


def adjust_local_bundle(scene, options=None, perturb=0.0, dense_check=None):
    """The restatement for one problem.  Returns a dict: camera_params, qvec, tvec, xyz (the caller's order), result (dict),
    margins (dict), trace [iterations + 1, 5], steps (per iteration 'a' accepted / 'r' rejected / 'i' invalid / 't' tolerance).
    perturb > 0: S and its right-hand side carry a seeded relative perturbation of that size (the conditioning probe).
    dense_check: a list that receives, per solve, (full damped normal matrix, its right-hand side, the step of the explicit
    reduced system, J'J of the unscaled corrected Jacobian) for the CPU tests that compare the two and bound the optimum."""
    opt = dict(DEFAULTS)
    opt.update(options or {})
    kind, scale = opt["loss_function_type"], opt["loss_function_scale"]
    sc, imap, cmap, pmap = canonical(scene)
    pb = LocalProblem(sc, opt)
    R, P, n = pb.nf, len(pb.pt_var), pb.n
    if R > MAX_REDUCED_DIM:
        raise ValueError("reduced camera system of %d columns" % R)
    N = len(pb.icam)
    st = {"qvec": sc["qvec"] / np.linalg.norm(sc["qvec"], axis=1, keepdims=True) if N else sc["qvec"], "tvec": sc["tvec"].copy(),
          "xyz": sc["xyz"].copy(), "camera_params": sc["camera_params"].copy()}
    margins = {"acceptance": np.inf, "gradient": np.inf, "pivot": np.inf, "point_pivot": np.inf}
    n_eff = 3 * int(pb.pt_var.sum()) + R
    out_scene = {k: np.array(np.asarray(scene[k], np.float64), copy=True) for k in ("camera_params", "qvec", "tvec", "xyz")}
    out_scene["qvec"], out_scene["tvec"], out_scene["xyz"] = out_scene["qvec"].reshape(-1, 4), out_scene["tvec"].reshape(-1, 3), out_scene["xyz"].reshape(-1, 3)
    res = dict(solved=int(n > 0), termination=CONVERGENCE, num_iterations=0, num_successful_steps=0, num_invalid_steps=0, reduced_dim=R,
               num_residuals=2 * n, num_effective_parameters=n_eff, initial_cost=0.0, final_cost=0.0,
               initial_mean_reprojection_error=0.0, final_mean_reprojection_error=0.0)
    if n == 0:
        return dict(out_scene, result=res, margins=margins, trace=np.zeros((0, 5)), steps="")
    toff = np.asarray(sc["track_offsets"], np.int64)
    pv = np.nonzero(pb.pt_var)[0]

    def evaluate(st):
        r, rho, E, F, rc, _ = pb.rows(st, kind, scale)
        return block_sum(0.5 * rho), block_sum(np.sqrt(r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])), E, F, rc

    def normal(E, F, rc, first, sc_e, sc_f):
        EtE, Etr = np.zeros((P, 6)), np.zeros((P, 3))
        for p in pv:  # the track in order
            for o in range(toff[p], toff[p + 1]):
                e0, e1 = E[o, 0], E[o, 1]
                EtE[p] += np.array([e0[0] * e0[0] + e1[0] * e1[0], e0[1] * e0[0] + e1[1] * e1[0], e0[1] * e0[1] + e1[1] * e1[1],
                                    e0[2] * e0[0] + e1[2] * e1[0], e0[2] * e0[1] + e1[2] * e1[1], e0[2] * e0[2] + e1[2] * e1[2]])
                Etr[p] += e0 * rc[o, 0] + e1 * rc[o, 1]
        # dense corrected F over the reduced columns, and F'F / F'r as in-order sums over the observations
        Fd = np.zeros((n, 2, R))
        for sl in range(18):
            ok = pb.fcol[:, sl] >= 0
            Fd[ok, 0, pb.fcol[ok, sl]] = F[ok, 0, sl]
            Fd[ok, 1, pb.fcol[ok, sl]] = F[ok, 1, sl]
        G = np.zeros((R, R))
        for a in range(R):
            G[a] = np.cumsum(Fd[:, 0, a:a + 1] * Fd[:, 0, :] + Fd[:, 1, a:a + 1] * Fd[:, 1, :], axis=0)[-1]
        g = np.cumsum(Fd[:, 0, :] * rc[:, 0:1] + Fd[:, 1, :] * rc[:, 1:2], axis=0)[-1] if R else np.zeros(0)
        cn_e, cn_f = EtE[:, [0, 2, 5]], np.diag(G).copy()
        if first:
            sc_e, sc_f = 1.0 / (1.0 + np.sqrt(cn_e)), 1.0 / (1.0 + np.sqrt(cn_f))
        D_e, D_f = np.clip((sc_e * sc_e) * cn_e, MIN_DIAG, MAX_DIAG), np.clip((sc_f * sc_f) * cn_f, MIN_DIAG, MAX_DIAG)
        full_g = np.zeros(pb.ne + R)
        full_g[pb.ecol[pv].reshape(-1)] = Etr[pv].reshape(-1)
        full_g[pb.ne:] = g
        return dict(EtE=EtE, Etr=Etr, G=G, g=g, sc_e=sc_e, sc_f=sc_f, D_e=D_e, D_f=D_f, Fd=Fd, gnorm=pb.gradient_max_norm(st, full_g))

    def step(nm, E, rc, radius, it):
        """(delta_e [P, 3], delta_f [R], model_cost_change, |delta|^2) or None for an invalid linear solve."""
        se, sf = nm["sc_e"], nm["sc_f"]
        Vinv = np.zeros((P, 6))
        ok = True
        for p in pv:
            w, s0, s1, s2 = nm["EtE"][p], se[p, 0], se[p, 1], se[p, 2]
            l = np.sqrt(nm["D_e"][p] / radius)
            v00, v10, v11 = (s0 * w[0]) * s0 + l[0] * l[0], (s1 * w[1]) * s0, (s1 * w[2]) * s1 + l[1] * l[1]
            v20, v21, v22 = (s2 * w[3]) * s0, (s2 * w[4]) * s1, (s2 * w[5]) * s2 + l[2] * l[2]
            with np.errstate(all="ignore"):
                d0 = v00
                m10, m20 = v10 / d0, v20 / d0
                d1 = v11 - m10 * v10
                m21 = (v21 - m20 * v10) / d1
                d2 = (v22 - m20 * v20) - m21 * (m21 * d1)
                for d, vd in ((d0, v00), (d1, v11), (d2, v22)):
                    margins["point_pivot"] = min(margins["point_pivot"], abs(d) / vd if np.isfinite(d) and vd > 0.0 else 0.0)
                    ok = ok and bool(d > 0.0 and np.isfinite(d))
                n20 = m10 * m21 - m20
                i0, i1, i2 = 1.0 / d0, 1.0 / d1, 1.0 / d2
                Vinv[p] = [(i0 + (m10 * m10) * i1) + (n20 * n20) * i2, -m10 * i1 - (n20 * m21) * i2, i1 + (m21 * m21) * i2, n20 * i2, -m21 * i2, i2]
        if not ok:
            return None
        l = np.sqrt(nm["D_f"] / radius)
        S = (sf[:, None] * nm["G"]) * sf[None, :] + np.diag(l * l)
        rhs = -(sf * nm["g"])
        Fd = nm["Fd"]
        for p in pv:  # canonical point order
            W = np.zeros((3, R))
            for o in range(toff[p], toff[p + 1]):
                for c in range(3):
                    W[c] += E[o, 0, c] * Fd[o, 0] + E[o, 1, c] * Fd[o, 1]
            W = (se[p][:, None] * W) * sf[None, :]
            vi = Vinv[p]
            Z = np.stack([(vi[0] * W[0] + vi[1] * W[1]) + vi[3] * W[2], (vi[1] * W[0] + vi[2] * W[1]) + vi[4] * W[2],
                          (vi[3] * W[0] + vi[4] * W[1]) + vi[5] * W[2]])
            S -= (np.outer(W[0], Z[0]) + np.outer(W[1], Z[1])) + np.outer(W[2], Z[2])
            ge = se[p] * nm["Etr"][p]
            rhs += (Z[0] * ge[0] + Z[1] * ge[1]) + Z[2] * ge[2]
        S = np.triu(S) + np.triu(S, 1).T
        if perturb > 0.0 and R:
            rng = np.random.default_rng(it)
            S = S * (1.0 + perturb * rng.standard_normal(S.shape))
            S = np.triu(S) + np.triu(S, 1).T
            rhs = rhs * (1.0 + perturb * rng.standard_normal(rhs.shape))
        U = _cholesky(S, margins)
        if U is None:
            return None
        dz = _solve(U, rhs)
        df = sf * dz
        de = np.zeros((P, 3))
        for p in pv:
            t = np.zeros(3)
            for o in range(toff[p], toff[p + 1]):
                f0 = f1 = 0.0
                for a in np.nonzero(pb.fcol[o] >= 0)[0]:
                    f0 += Fd[o, 0, pb.fcol[o, a]] * df[pb.fcol[o, a]]
                    f1 += Fd[o, 1, pb.fcol[o, a]] * df[pb.fcol[o, a]]
                t += E[o, 0] * f0 + E[o, 1] * f1
            b = se[p] * (nm["Etr"][p] + t)
            vi = Vinv[p]
            y = -np.array([(vi[0] * b[0] + vi[1] * b[1]) + vi[3] * b[2], (vi[1] * b[0] + vi[2] * b[1]) + vi[4] * b[2],
                           (vi[3] * b[0] + vi[4] * b[1]) + vi[5] * b[2]])
            de[p] = se[p] * y
        acc = np.zeros(T)
        for a in range(R):
            acc[a % T] += df[a] * df[a]
        for p in pv:
            acc[p % T] += (de[p, 0] * de[p, 0] + de[p, 1] * de[p, 1]) + de[p, 2] * de[p, 2]
        s2 = butterfly(acc)
        j = np.zeros((n, 2))
        for c in range(3):
            j += np.where(pb.pt_var[pb.obs_pt][:, None], E[:, :, c] * de[pb.obs_pt, c:c + 1], 0.0)
        for sl in range(18):
            okc = pb.fcol[:, sl] >= 0
            col = np.where(okc, pb.fcol[:, sl], 0)
            j += np.where(okc[:, None], Fd[np.arange(n), :, col] * df[col][:, None], 0.0) if R else 0.0
        mcc = -block_sum(j[:, 0] * (rc[:, 0] + j[:, 0] / 2.0) + j[:, 1] * (rc[:, 1] + j[:, 1] / 2.0))
        if dense_check is not None:
            Je = np.zeros((2 * n, 3 * P))
            for o in range(n):
                Je[2 * o:2 * o + 2, 3 * pb.obs_pt[o]:3 * pb.obs_pt[o] + 3] = E[o] * se[pb.obs_pt[o]]
            Jf = Fd.reshape(2 * n, R) * sf
            keep = np.concatenate([np.repeat(pb.pt_var, 3), np.ones(R, bool)])
            J = np.concatenate([Je, Jf], 1)[:, keep]
            Dd = np.concatenate([nm["D_e"].reshape(-1), nm["D_f"]])[keep]
            Ju = J / np.concatenate([se.reshape(-1), sf])[keep]  # the unscaled Jacobian
            dense_check.append((J.T @ J + np.diag(Dd / radius), -(J.T @ rc.reshape(-1)), np.concatenate([(de / se)[pv].reshape(-1), dz]), Ju.T @ Ju))
        return de, df, mcc, s2

    cost, err, E, F, rc = evaluate(st)
    res["initial_cost"], res["initial_mean_reprojection_error"] = cost, err / n
    radius, dec = 1e4, 2.0
    it = n_succ = n_inv = n_inv_total = 0
    term, trace, steps = None, [], ""
    gnorm = 0.0

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
        trace.append([cost, radius, rho_lm, accepted, gnorm])

    if n_eff == 0:  # Ceres reduces the problem to an empty program
        term = CONVERGENCE
        trace.append([cost, radius, np.nan, 1, 0.0])
    elif not np.isfinite(cost):
        term = FAILURE
        trace.append([cost, radius, np.nan, 1, 0.0])
    else:
        nm = normal(E, F, rc, True, None, None)
        gnorm = nm["gnorm"]
        finalize(True, np.nan, 1)
    while term is None:
        sol = step(nm, E, rc, radius, it)
        valid, cand_cost = False, np.inf
        if sol is not None:
            de, df, mcc, s2 = sol
            valid = bool(np.isfinite(mcc) and mcc > 0.0 and np.isfinite(s2))
        if valid:
            delta = np.zeros(pb.ne + R)
            delta[pb.ecol[pv].reshape(-1)] = de[pv].reshape(-1)
            delta[pb.ne:] = df
            cand = pb.plus(st, delta)
            cand_cost, cand_err, cE, cF, crc = evaluate(cand)
            valid = bool(np.isfinite(cand_cost))
        it += 1
        accepted, rho_lm = 0, np.nan
        if not valid:
            n_inv += 1
            n_inv_total += 1
            steps += "i"
            if n_inv >= opt["max_num_consecutive_invalid_steps"]:
                term = FAILURE
            else:
                radius /= dec
                dec *= 2.0
        else:
            n_inv = 0
            if np.sqrt(s2) <= opt["parameter_tolerance"] * (np.sqrt(pb.x_norm2(st)) + opt["parameter_tolerance"]):
                term = CONVERGENCE
                steps += "t"
            elif abs(cost - cand_cost) <= opt["function_tolerance"] * cost:
                term = CONVERGENCE
                steps += "t"
            else:
                rho_lm = (cost - cand_cost) / mcc
                margins["acceptance"] = min(margins["acceptance"], abs((cost - cand_cost) - MIN_REL_DECREASE * mcc) / max(cost, TINY))
                if rho_lm > MIN_REL_DECREASE:
                    accepted = 1
                    n_succ += 1
                    steps += "a"
                    st, cost, err, E, F, rc = cand, cand_cost, cand_err, cE, cF, crc
                    tmp = 2.0 * rho_lm - 1.0
                    radius = min(MAX_RADIUS, radius / max(1.0 / 3.0, 1.0 - tmp ** 3))
                    dec = 2.0
                    if term is None:
                        nm = normal(E, F, rc, False, nm["sc_e"], nm["sc_f"])
                        gnorm = nm["gnorm"]
                else:
                    steps += "r"
                    radius /= dec
                    dec *= 2.0
        finalize(bool(accepted) and term is None, rho_lm, accepted)
    res.update(termination=term, num_iterations=it, num_successful_steps=n_succ, num_invalid_steps=n_inv_total, final_cost=cost,
               final_mean_reprojection_error=err / n)
    if n_eff > 0:  # back to the caller's order; a problem with no variable block keeps its input bits
        out_scene["qvec"][imap] = st["qvec"]
        vi = imap[pb.qcol[:, 0] >= 0]
        out_scene["tvec"][vi] = st["tvec"][pb.qcol[:, 0] >= 0]
        out_scene["xyz"][pmap[pb.pt_var]] = st["xyz"][pb.pt_var]
        models = np.asarray(scene["camera_model_ids"], np.int64).reshape(-1)
        soff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in models])]).astype(np.int64)
        for r, c in enumerate(cmap):
            if pb.cam_var[r]:
                out_scene["camera_params"][soff[c]:soff[c + 1]] = st["camera_params"][pb.poff[r]:pb.poff[r + 1]]
    return dict(out_scene, result=res, margins=margins, trace=np.array(trace, np.float64), steps=steps)


def stable_under_rounding(scene, options, out=None, tol=1e-10):
    """DESIGN.md 12's conditioning probe: the run again with S and its right-hand side perturbed by 1e-15 relative must
    reproduce every decision and the cost trace to `tol`."""
    a = out if out is not None else adjust_local_bundle(scene, options)
    b = adjust_local_bundle(scene, options, perturb=1e-15)
    if a["steps"] != b["steps"] or a["result"]["termination"] != b["result"]["termination"]:
        return False
    ta, tb = a["trace"][:, 0], b["trace"][:, 0]
    return bool(np.all(np.abs(ta - tb) <= tol * np.abs(ta)))


def is_clear(scene, options, out=None):
    """The restatement's verdict: every margin at least 1e-9 and stable under the probe."""
    out = out if out is not None else adjust_local_bundle(scene, options)
    return bool(min(out["margins"].values()) >= 1e-9 and stable_under_rounding(scene, options, out))
