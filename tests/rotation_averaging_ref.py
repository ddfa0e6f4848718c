"""numpy restatement of GlobalRotationAveraging() as DistributedMapperController runs it with its defaults
(reconstruct_largest_cc, ROBUST_L1L2): the largest connected component, RobustRotationEstimator (L1 regression by ADMM, then
IRLS), FilterViewPairsFromOrientation, the largest component of what survives ("Global rotation averaging").

Every system A^T W A = L_w (x) I3 is solved by a dense Cholesky of the grounded scalar Laplacian L_w with three right-hand
sides (fine up to a few thousand images).  For larger graphs whose structure is known, `partition` (independent blocks of
images plus a small separator set) solves every system directly by block elimination instead: a batched Cholesky of the
blocks and a dense Schur complement on the separator.  ceres' rotation conversions are restated from the published formulas, vectorised over
rows.  Every stopping decision is recorded with its value and its margin to the threshold (`decisions`), so that a fixture
sitting on a knife edge shows up as a fixture problem.  The tie rule between equal-size components (the one holding the
smallest image id wins) is this project's choice.  The device's cold-restart rule of its warm-started solver (a column
restarts from x = 0 when ||rhs - L x_prev||^2 > ||rhs||^2) does not change the answer; it is recorded as decision "cold" so
that a test can show which fixtures take that path."""
import numpy as np

DEG2RAD = np.pi / 180.0


# ---------------------------------------------------------------- ceres' conversions (row-major matrices, [n, ...] rows)
def quaternion_to_angle_axis(q):
    q = np.asarray(q, np.float64).reshape(-1, 4)
    s2 = (q[:, 1] * q[:, 1] + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
    k = np.full(len(q), 2.0)
    pos = s2 > 0.0
    st = np.sqrt(s2[pos])
    ct = q[pos, 0]
    two = 2.0 * np.where(ct < 0.0, np.arctan2(-st, -ct), np.arctan2(st, ct))
    k[pos] = two / st
    return q[:, 1:4] * k[:, None]


def angle_axis_to_rotation(aa):
    aa = np.asarray(aa, np.float64).reshape(-1, 3)
    th2 = (aa[:, 0] * aa[:, 0] + aa[:, 1] * aa[:, 1]) + aa[:, 2] * aa[:, 2]
    R = np.empty((len(aa), 3, 3))
    big = th2 > np.finfo(np.float64).eps
    th = np.sqrt(np.where(big, th2, 1.0))
    wx, wy, wz = aa[:, 0] / th, aa[:, 1] / th, aa[:, 2] / th
    c, s = np.cos(th), np.sin(th)
    R[:, 0, 0] = c + wx * wx * (1.0 - c)
    R[:, 1, 0] = wz * s + wx * wy * (1.0 - c)
    R[:, 2, 0] = -wy * s + wx * wz * (1.0 - c)
    R[:, 0, 1] = wx * wy * (1.0 - c) - wz * s
    R[:, 1, 1] = c + wy * wy * (1.0 - c)
    R[:, 2, 1] = wx * s + wy * wz * (1.0 - c)
    R[:, 0, 2] = wy * s + wx * wz * (1.0 - c)
    R[:, 1, 2] = -wx * s + wy * wz * (1.0 - c)
    R[:, 2, 2] = c + wz * wz * (1.0 - c)
    sm = ~big
    if sm.any():
        a = aa[sm]
        one, z = np.ones(len(a)), a
        R[sm] = np.stack([np.stack([one, -z[:, 2], z[:, 1]], 1), np.stack([z[:, 2], one, -z[:, 0]], 1),
                          np.stack([-z[:, 1], z[:, 0], one], 1)], 1)
    return R


def rotation_to_quaternion(R):
    R = np.asarray(R, np.float64).reshape(-1, 3, 3)
    q = np.empty((len(R), 4))
    tr = (R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]
    p = tr >= 0.0
    t = np.sqrt(tr[p] + 1.0)
    q[p, 0] = 0.5 * t
    t = 0.5 / t
    q[p, 1] = (R[p, 2, 1] - R[p, 1, 2]) * t
    q[p, 2] = (R[p, 0, 2] - R[p, 2, 0]) * t
    q[p, 3] = (R[p, 1, 0] - R[p, 0, 1]) * t
    # trace < 0: the branch of the largest diagonal entry (the first one on ties), row by row in one pass per branch
    d = R[:, [0, 1, 2], [0, 1, 2]]
    i = np.where(d[:, 1] > d[:, 0], 1, 0)
    i = np.where(d[:, 2] > d[np.arange(len(R)), i], 2, i)
    for b in range(3):
        m = ~p & (i == b)
        if not m.any():
            continue
        j, k = (b + 1) % 3, (b + 2) % 3
        M = R[m]
        t = np.sqrt(((M[:, b, b] - M[:, j, j]) - M[:, k, k]) + 1.0)
        q[m, b + 1] = 0.5 * t
        t = 0.5 / t
        q[m, 0] = (M[:, k, j] - M[:, j, k]) * t
        q[m, j + 1] = (M[:, j, b] + M[:, b, j]) * t
        q[m, k + 1] = (M[:, k, b] + M[:, b, k]) * t
    return q


def rotation_to_angle_axis(R):
    return quaternion_to_angle_axis(rotation_to_quaternion(R))


def multiply_rotations(a, b):
    """MultiplyRotations (src/math/rotation.cpp:157-167)."""
    return rotation_to_angle_axis(np.matmul(angle_axis_to_rotation(a), angle_axis_to_rotation(b)))


# ---------------------------------------------------------------- graph helpers
def largest_component(n, edges):
    """(flags [n], number of components): union-find; ties -> the component holding the smallest vertex."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(v) for v in range(n)], np.int64)
    size = np.bincount(roots, minlength=n)
    best = int(np.argmax(size))  # first maximum = smallest root = smallest member
    return roots == best, int(len(np.unique(roots)))


def _laplacian(N, ei, ej, w):
    L = np.zeros((N, N))
    np.add.at(L, (ei, ei), w)
    np.add.at(L, (ej, ej), w)
    np.add.at(L, (ei, ej), -w)
    np.add.at(L, (ej, ei), -w)
    return L[1:, 1:]


def _at(N, ei, ej, v):
    """A^T v for edge vectors v [M, 3]: +v at image 2, -v at image 1; row 0 (the constant image) dropped."""
    out = np.zeros((N, 3))
    np.add.at(out, ej, v)
    np.add.at(out, ei, -v)
    return out[1:]


def _at_sum(N, ei, ej, v):
    """_at by per-image sums (np.bincount): the same value up to the order of the additions, and far faster on large graphs."""
    out = np.stack([np.bincount(ej, v[:, c], N) - np.bincount(ei, v[:, c], N) for c in range(3)], 1)
    return out[1:]


def _chol_solve(L, rhs):
    C = np.linalg.cholesky(L)
    y = np.linalg.solve(C, rhs)
    return np.linalg.solve(C.T, y)


class BlockFactor:
    """The grounded Laplacian L_w of a graph whose images split into independent blocks (no edge joins two blocks) and a
    separator, factorised by block elimination: L = [[A, B], [B^T, S]] with A block-diagonal; every block by a batched Cholesky
    A_k = C_k C_k^T, the separator by a dense Cholesky of S - sum_k B_k^T A_k^-1 B_k.  One block holding every image is
a dense Cholesky whose repeated solves are cheap.  `groups` is a list of [n_blocks, size]
    arrays of component indices, `sep` an array of component indices; image 0 (the grounded one) must be in neither."""

    def __init__(self, N, ei, ej, w, groups, sep):
        self.N, self.groups, self.sep = N, groups, np.asarray(sep, np.int64)
        ns = len(self.sep)
        kind = np.full(N, -2, np.int64)  # -2 unassigned, -1 separator, >= 0 group
        blk = np.zeros(N, np.int64)
        pos = np.zeros(N, np.int64)
        kind[self.sep] = -1
        pos[self.sep] = np.arange(ns)
        for g, G in enumerate(groups):
            if np.any(kind[G] != -2):
                raise ValueError("an image is in two sets of the partition")
            kind[G] = g
            blk[G] = np.arange(len(G))[:, None]
            pos[G] = np.arange(G.shape[1])[None, :]
        if kind[0] != -2 or np.any(kind[1:] == -2):
            raise ValueError("the partition must hold every image but the grounded one, once")
        d = np.zeros(N)
        np.add.at(d, ei, w)
        np.add.at(d, ej, w)
        A = [np.zeros((len(G), G.shape[1], G.shape[1])) for G in groups]
        Bm = [np.zeros((len(G), G.shape[1], ns)) for G in groups]
        S = np.zeros((ns, ns))
        for g, G in enumerate(groups):
            A[g][np.arange(len(G))[:, None], np.arange(G.shape[1])[None, :], np.arange(G.shape[1])[None, :]] = d[G]
        S[np.arange(ns), np.arange(ns)] = d[self.sep]
        inner = (ei != 0) & (ej != 0)
        a, b, we = ei[inner], ej[inner], w[inner]
        for u, v in ((a, b), (b, a)):  # both triangles of L
            ku, kv = kind[u], kind[v]
            m = (ku == -1) & (kv == -1)
            np.add.at(S, (pos[u[m]], pos[v[m]]), -we[m])
            for g in range(len(groups)):
                m = (ku == g) & (kv == g)
                if np.any(blk[u[m]] != blk[v[m]]):
                    raise ValueError("an edge joins two blocks")
                np.add.at(A[g], (blk[u[m]], pos[u[m]], pos[v[m]]), -we[m])
                m = (ku == g) & (kv == -1)
                np.add.at(Bm[g], (blk[u[m]], pos[u[m]], pos[v[m]]), -we[m])
            if np.any((ku >= 0) & (kv >= 0) & (ku != kv)):
                raise ValueError("an edge joins two blocks")
        # the inverses of the triangular factors are formed once: every solve is then two products per level
        self.Ci = [np.linalg.inv(np.linalg.cholesky(Ag)) for Ag in A]
        self.Y = [Ci @ Bg for Ci, Bg in zip(self.Ci, Bm)]  # C_k^-1 B_k
        schur = S - sum(np.tensordot(Y, Y, axes=([0, 1], [0, 1])) for Y in self.Y)
        self.Csi = np.linalg.inv(np.linalg.cholesky(schur)) if ns else np.zeros((0, 0))

    def solve(self, rhs):
        """L x = rhs for rhs [N - 1, 3] (rows 1..N-1 of the component), returns [N - 1, 3]."""
        full = np.vstack([np.zeros((1, 3)), rhs])
        x = np.zeros((self.N, 3))
        yr = [Ci @ full[G] for Ci, G in zip(self.Ci, self.groups)]  # C_k^-1 r_k
        rs = full[self.sep] - sum(np.tensordot(Y, y, axes=([0, 1], [0, 1])) for Y, y in zip(self.Y, yr))
        xs = self.Csi.T @ (self.Csi @ rs)
        x[self.sep] = xs
        for Ci, G, Y, y in zip(self.Ci, self.groups, self.Y, yr):
            x[G] = np.transpose(Ci, (0, 2, 1)) @ (y - Y @ xs)
        return x[1:]


def _partition_groups(partition, cimg):
    """(blocks, separator) of image ids -> (groups of component indices by block size, separator indices); the grounded image
    (component index 0) is dropped from whichever set holds it, images outside the component are dropped."""
    blocks, sep = partition
    where = {int(i): k for k, i in enumerate(cimg)}
    by_size = {}
    for blk in blocks:
        c = [where[int(i)] for i in blk if int(i) in where and where[int(i)] != 0]
        if c:
            by_size.setdefault(len(c), []).append(c)
    groups = [np.array(by_size[k], np.int64) for k in sorted(by_size)]
    sep_c = np.array([where[int(i)] for i in sep if int(i) in where and where[int(i)] != 0], np.int64)
    return groups, sep_c


def rotation_averaging(pairs, qvecs, use=None, max_num_l1_iterations=5, max_num_irls_iterations=100, l1_thr=0.001, irls_thr=0.001,
                       sigma=5.0 * DEG2RAD, admm_initial=5, rho=1.0, alpha=1.0, abs_tol=1e-4, rel_tol=1e-2, filter_degrees=5.0,
                       partition=None):
    """Returns a dict shaped like capi.Context.rotation_averaging plus `decisions`: a list of (name, value, threshold).
    `partition` = (blocks, separator) of image ids: solve by block elimination (BlockFactor) instead of a dense Cholesky."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    qvecs = np.asarray(qvecs, np.float64).reshape(-1, 4)
    n = len(pairs)
    used = np.ones(n, bool) if use is None else np.asarray(use).astype(bool)
    state = np.zeros(n, np.uint8)
    rel_out = np.zeros((n, 3))
    dec = []
    rep = {"num_components": 0, "num_images": 0, "num_edges": 0, "num_l1_iterations": 0, "admm_iterations": [], "num_irls_iterations": 0,
           "num_filtered_edges": 0, "num_final_images": 0}
    seen, uniq = set(), []
    for e in np.nonzero(used)[0]:
        a, b = int(pairs[e, 0]), int(pairs[e, 1])
        if a == b:
            raise ValueError("image_id1 == image_id2")
        key = (min(a, b), max(a, b))
        if key not in seen:
            seen.add(key)
            uniq.append(e)
    empty = {"image_ids": np.zeros(0, np.uint32), "orientations": np.zeros((0, 3)), "in_final_cc": np.zeros(0, bool),
             "edge_state": state, "relative_rotations": rel_out, "report": rep, "decisions": dec}
    if not uniq:
        return empty
    uniq = np.array(uniq)
    ids = np.unique(pairs[uniq].reshape(-1))
    vi = np.searchsorted(ids, pairs[uniq, 0])
    vj = np.searchsorted(ids, pairs[uniq, 1])
    in1, rep["num_components"] = largest_component(len(ids), zip(vi, vj))
    inside = in1[vi]
    state[uniq[~inside]] = 1
    cidx = np.cumsum(in1) - 1
    cimg = ids[in1]
    E = uniq[inside]
    ei, ej = cidx[vi[inside]], cidx[vj[inside]]
    N, M = len(cimg), len(E)
    rep["num_images"], rep["num_edges"] = N, M
    r12 = quaternion_to_angle_axis(qvecs[E])
    R = np.zeros((N, 3))

    def residuals():
        inner = multiply_rotations(r12, R[ei])
        return multiply_rotations(-R[ej], inner).reshape(M, 3)

    def rotate(x):
        R[1:] = multiply_rotations(R[1:], x)
        return float(np.sum(np.sqrt(np.sum(x * x, axis=1)))) / (N - 1)

    at = _at if partition is None else _at_sum
    x_prev = np.zeros((N - 1, 3))

    def record_cold(w, rhs):
        """the device's warm-start rule per column: cold iff ||rhs - L x_prev||^2 > ||rhs||^2 (an all-zero x_prev is an exact tie)"""
        xf = np.vstack([np.zeros((1, 3)), x_prev])
        r = rhs - at(N, ei, ej, w[:, None] * (xf[ej] - xf[ei]))
        for c in range(3):
            if np.any(x_prev[:, c] != 0.0):
                dec.append(("cold", float(np.sum(r[:, c] * r[:, c])), float(np.sum(rhs[:, c] * rhs[:, c]))))

    b = residuals()
    if partition is None:
        L0 = _laplacian(N, ei, ej, np.ones(M))
        C0 = np.linalg.cholesky(L0)

        def solve0(rhs):
            return np.linalg.solve(C0.T, np.linalg.solve(C0, rhs))

        def solve_w(w, rhs):
            return _chol_solve(_laplacian(N, ei, ej, w), rhs)
    else:
        groups, sep_c = _partition_groups(partition, cimg)
        solve0 = BlockFactor(N, ei, ej, np.ones(M), groups, sep_c).solve

        def solve_w(w, rhs):
            return BlockFactor(N, ei, ej, w, groups, sep_c).solve(rhs)

    cap = admm_initial
    pabs, dabs = np.sqrt(3.0 * M) * abs_tol, np.sqrt(3.0 * (N - 1)) * abs_tol
    for it in range(max_num_l1_iterations):
        z = np.zeros((M, 3))
        u = np.zeros((M, 3))
        bn = np.sqrt(np.sum(b * b))
        n_it = 0
        for t in range(cap):
            rhs = at(N, ei, ej, (b + z) - u)
            record_cold(np.ones(M), rhs)
            x = x_prev = solve0(rhs)
            xf = np.vstack([np.zeros((1, 3)), x])
            ax = xf[ej] - xf[ei]
            ah = alpha * ax + (1.0 - alpha) * (z + b)
            zo = z
            v = (ah - b) + u
            z = np.maximum(0.0, v - 1.0 / rho) - np.maximum(0.0, -v - 1.0 / rho)
            u = u + ((ah - z) - b)
            r_norm = np.sqrt(np.sum(((ax - z) - b) ** 2))
            s_norm = np.sqrt(np.sum((-rho * at(N, ei, ej, z - zo)) ** 2))
            max_norm = max(np.sqrt(np.sum(ax * ax)), np.sqrt(np.sum(z * z)), bn)
            pe = pabs + rel_tol * max_norm
            de = dabs + rel_tol * np.sqrt(np.sum((rho * at(N, ei, ej, u)) ** 2))
            n_it = t + 1
            dec.append(("admm_r", r_norm, pe))
            dec.append(("admm_s", s_norm, de))
            if r_norm < pe and s_norm < de:
                break
        rep["admm_iterations"].append(n_it)
        rep["num_l1_iterations"] = it + 1
        step = rotate(x)
        b = residuals()
        dec.append(("l1_step", step, l1_thr))
        rep["last_l1_step"] = step
        if step <= l1_thr:
            break
        cap *= 2
    for it in range(max_num_irls_iterations):
        e2 = np.sum(b * b, axis=1)
        tmp = e2 + sigma * sigma
        w = sigma / (tmp * tmp)
        rhs = at(N, ei, ej, w[:, None] * b)
        record_cold(w, rhs)
        x = x_prev = solve_w(w, rhs)
        step = rotate(x)
        b = residuals()
        rep["num_irls_iterations"] = it + 1
        rep["last_irls_step"] = step
        dec.append(("irls_step", step, irls_thr))
        if step < irls_thr:
            break
    thr = filter_degrees * DEG2RAD
    comp = multiply_rotations(R[ej], -R[ei])
    loop = multiply_rotations(-r12, comp)
    sq = np.sum(loop * loop, axis=1)
    keep = sq <= thr * thr
    for k in range(M):
        dec.append(("filter", sq[k], thr * thr))
    state[E] = np.where(keep, 3, 2)
    Ri, Rj = angle_axis_to_rotation(R[ei]), angle_axis_to_rotation(R[ej])
    rel = rotation_to_angle_axis(np.matmul(Rj, np.transpose(Ri, (0, 2, 1))))
    rel_out[E[keep]] = rel[keep]
    rep["num_filtered_edges"] = int((~keep).sum())
    fin, _ = largest_component(N, zip(ei[keep], ej[keep]))
    rep["num_final_images"] = int(fin.sum())
    return {"image_ids": cimg.astype(np.uint32), "orientations": R, "in_final_cc": fin, "edge_state": state, "relative_rotations": rel_out,
            "report": rep, "decisions": dec}


def min_margin(decisions):
    """Smallest margin over the recorded decisions: |value - threshold| / threshold, or |value| where the threshold is 0."""
    return min(abs(v - t) / t if t != 0 else abs(v) for _, v, t in decisions) if decisions else np.inf


def cold_restarts(decisions):
    """Number of recorded solve columns whose warm start was worse than zero (the device restarts them from x = 0)."""
    return sum(1 for name, v, t in decisions if name == "cold" and v > t)


def angle_between(a, b):
    """Angle (rad) of R(a)^T R(b), row by row: the gap between two angle-axis vectors."""
    Ra, Rb = angle_axis_to_rotation(a), angle_axis_to_rotation(b)
    return np.linalg.norm(rotation_to_angle_axis(np.matmul(np.transpose(Ra, (0, 2, 1)), Rb)), axis=1)
