"""numpy / scalar-Python restatement of SfMAligner (src/controllers/sfm_aligner.cpp:34-417) as dsm_align_clusters restates
it, with a margin recorded for every decision, and a seeded synthetic scene of overlapping cluster
reconstructions with planted Sim3s.

Rules restated: the common registered images and the separators; FindCommon3DPoints' correspondences in the canonical order
(ascending point id of the second cluster, then (image_id, point2D_idx)); PROSAC (ProsacSampler's n(k) with T_N = 20000,
std::mt19937 + libstdc++'s uniform_int_distribution<int>, MLE cost, strict best update, ComputeMaxIterations unless fewer than
4 inliers); Umeyama with scaling (Eigen 3.3: S(2) = -1 when det U det V < 0, c = sigma . S / src_var) inside FindRTS; the
refits of FindSimilarityTransform; msd (CheckReprojError); the edge rules; the largest component, Kruskal on float weights,
FindAnchorNode and ComputePath with the tie rules of DESIGN.md 11.

Numerics: the 3 x 3 SVD is LAPACK's here and Eigen's JacobiSVD on the device, so models agree to rounding, not to the bit;
the residuals and the MLE costs are evaluated in the device's order (costs summed in index order).  The margins say where
rounding could flip a decision:
  residual  min |r - threshold| / threshold over every residual PROSAC scored (the inlier tests its choices depend on)
  cost      min |cost - best| / best over the strict-best tests whose outcome could matter: between two costs without an
            inlier (both exactly N * threshold) there is none; a near-tie between two trials of one inlier count (a track
            seen in two common images gives a correspondence twice, so samples repeat coordinates, and degenerate samples
            tie) leaves the iteration cap alone and only counts when no clearly better model (gap >= CLEAR) follows it
  weight    |weight - max_reprojection_error| / max_reprojection_error
  float     the distance of the double weight to the nearest float32 rounding boundary, relative to the weight"""
import math
import random

import numpy as np

DBL_MAX = np.finfo(np.float64).max
EPS = np.finfo(np.float64).eps
BATCH = 256


def default_options(**kw):
    o = dict(threshold=0.1, max_reprojection_error=1.8, failure_probability=0.01, min_iterations=100, max_iterations=5000,
             random_seed=0)
    o.update(kw)
    return o


# ---------------------------------------------------------------- std::mt19937 + uniform_int_distribution<int>
class MT19937:
    """std::mt19937(seed): init_genrand, then Python's own MT19937 core (the same generator) from that state."""

    def __init__(self, seed=5489):
        mt = [seed & 0xFFFFFFFF]
        for i in range(1, 624):
            mt.append((1812433253 * (mt[-1] ^ (mt[-1] >> 30)) + i) & 0xFFFFFFFF)
        self._r = random.Random()
        self._r.setstate((3, tuple(mt + [624]), None))

    def __call__(self):
        return self._r.getrandbits(32)


def rand_int(g, hi):
    """uniform_int_distribution<int>(0, hi)(mt19937), libstdc++ (Lemire's method on 32-bit draws), hi >= 0."""
    rng = hi + 1
    product = g() * rng
    low = product & 0xFFFFFFFF
    if low < rng:
        threshold = ((1 << 32) - rng) % rng
        while low < threshold:
            product = g() * rng
            low = product & 0xFFFFFFFF
    return product >> 32


def pair_seed(i, j, user_seed=0):
    """dsm_pair_seed (csrc/capi.hip)."""
    a, b = min(i, j), max(i, j)
    h = (2147483647 * a + b) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 33
    h = (h * 0xFF51AFD7ED558CCD) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 33
    h = (h * 0xC4CEB9FE1A85EC53) & 0xFFFFFFFFFFFFFFFF
    h ^= h >> 33
    return (h & 0xFFFFFFFF) ^ user_seed


def align_seed(i, j, direction, user_seed=0):
    return pair_seed(i, j, user_seed) ^ (0x85EBCA6B if direction else 0)


# ---------------------------------------------------------------- PROSAC tables
def prosac_table(N, kmax):
    """ProsacSampler::Sample's n and branch (True: 4 of the top n, False: 3 of the top n - 1 plus n) for k = 1 .. kmax."""
    t_n = 20000.0
    n = 4
    for i in range(4):
        t_n *= float(n - i) / (N - i)
    t_n_prime = 1.0
    ns, br = np.zeros(kmax, np.int64), np.zeros(kmax, bool)
    for t in range(1, kmax + 1):
        if t > t_n_prime and n < N:
            t_n_plus1 = (t_n * (n + 1.0)) / (n + 1.0 - 4)
            t_n_prime += math.ceil(t_n_plus1 - t_n)
            t_n = t_n_plus1
            n += 1
        ns[t - 1] = n
        br[t - 1] = t_n_prime < t
    return ns, br


def max_iter_table(N, o):
    """ComputeMaxIterations(4, c / N, log(failure_probability)) for c = 0 .. N (c < 4 never read)."""
    lf = math.log(o["failure_probability"])
    out = np.zeros(N + 1, np.int64)
    out[0] = o["max_iterations"]
    for c in range(1, N + 1):
        r = float(c) / float(N)
        if r == 1.0:
            out[c] = o["min_iterations"]
            continue
        lp = math.log(1.0 - math.pow(r, 4.0)) - EPS
        num = lf / lp
        out[c] = int(max(float(o["min_iterations"]), min(num, float(o["max_iterations"]))))
    return out


def draw_sample(g, n, branch):
    s = []
    if branch:
        for _ in range(4):
            r = rand_int(g, n - 1)
            while r in s:
                r = rand_int(g, n - 1)
            s.append(r)
    else:
        for _ in range(3):
            r = rand_int(g, n - 2)
            while r in s:
                r = rand_int(g, n - 2)
            s.append(r)
        s.append(n)
    return s


# ---------------------------------------------------------------- Umeyama / FindRTS (batched)
def det3(m):
    """Eigen's 3 x 3 determinant order, m [..., 3, 3]."""
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 2, 1] * m[..., 1, 2])
            - m[..., 1, 0] * (m[..., 0, 1] * m[..., 2, 2] - m[..., 2, 1] * m[..., 0, 2])
            + m[..., 2, 0] * (m[..., 0, 1] * m[..., 1, 2] - m[..., 1, 1] * m[..., 0, 2]))


def find_rts(mean1, mean2, sigma, var, s, R, t):
    """FindRTS from Umeyama's moments, batched over the leading axis; (s, R, t) in / out with FindRTS' failure paths."""
    U, sv, Vt = np.linalg.svd(sigma)
    V = np.swapaxes(Vt, -1, -2)
    S = np.ones(sv.shape)
    S[det3(U) * det3(V) < 0.0, 2] = -1.0
    Rr = np.zeros(sigma.shape)
    for i in range(3):
        for j in range(3):
            Rr[..., i, j] = (U[..., i, 0] * S[..., 0]) * V[..., j, 0] + (U[..., i, 1] * S[..., 1]) * V[..., j, 1] + \
                            (U[..., i, 2] * S[..., 2]) * V[..., j, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (1.0 / var) * (sv[..., 0] * S[..., 0] + sv[..., 1] * S[..., 1] + sv[..., 2] * S[..., 2])
        cR = Rr * c[..., None, None]
        tt = mean2 - ((c[..., None] * Rr[..., :, 0]) * mean1[..., None, 0] + (c[..., None] * Rr[..., :, 1]) * mean1[..., None, 1]
                      + (c[..., None] * Rr[..., :, 2]) * mean1[..., None, 2])
        det = det3(cR)
        s, R, t = s.copy(), cR.copy(), t.copy()
        ok = ~(det < 0.0)
        S3 = np.power(np.where(ok, det, 1.0), 1.0 / 3.0)
        s[ok] = S3[ok]
        ok2 = ok & ~(S3 < EPS)
        R[ok2] = cR[ok2] / S3[ok2][:, None, None]
        t[ok2] = tt[ok2]
    return s, R, t


def fit4(a, b):
    """the 4-point model of every trial: a, b [B, 4, 3] -> (s [B], R [B, 3, 3], t [B, 3]) from Sim3()."""
    B = a.shape[0]
    m1 = (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]) * 0.25
    m2 = (((b[:, 0] + b[:, 1]) + b[:, 2]) + b[:, 3]) * 0.25
    sig = np.zeros((B, 3, 3))
    var3 = np.zeros((B, 3))
    for q in range(4):
        d1, d2 = a[:, q] - m1, b[:, q] - m2
        var3 += d1 * d1
        sig += d2[:, :, None] * d1[:, None, :]
    sig = 0.25 * sig
    var = ((var3[:, 0] + var3[:, 1]) + var3[:, 2]) * 0.25
    return find_rts(m1, m2, sig, var, np.ones(B), np.broadcast_to(np.eye(3), (B, 3, 3)).copy(), np.zeros((B, 3)))


def fit_all(a, b, s, R, t):
    """FindRTS over all given correspondences (a, b [m, 3]) from (s, R, t); fewer than 3: unchanged."""
    m = len(a)
    if m < 3:
        return s, R, t
    on = 1.0 / m
    m1, m2 = a.sum(0) * on, b.sum(0) * on
    d1, d2 = a - m1, b - m2
    sig = on * (d2.T @ d1)
    v = (d1 * d1).sum(0)
    var = ((v[0] + v[1]) + v[2]) * on
    s2, R2, t2 = find_rts(m1[None], m2[None], sig[None], np.array([var]), np.array([s]), R[None], t[None])
    return float(s2[0]), R2[0], t2[0]


def residuals(s, R, t, a, b):
    """||s R a + t - b|| in the device's order, for models [B] x points [N] -> [B, N]."""
    A = s[:, None, None] * R
    d = []
    for i in range(3):
        y = A[:, i, 0, None] * a[None, :, 0] + A[:, i, 1, None] * a[None, :, 1]
        y = y + A[:, i, 2, None] * a[None, :, 2]
        d.append((y + t[:, i, None]) - b[None, :, i])
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


# ---------------------------------------------------------------- PROSAC, refit, msd
CLEAR = 1e-9  # a relative cost gap from which on no rounding of the model flips a strict-best test


def prosac(a, b, seed, o):
    """RansacSimilarity: returns the best model, iterations, the residual / cost margins and the best MLE cost."""
    N = len(a)
    thr = o["threshold"]
    ns, br = prosac_table(N, o["max_iterations"])
    assert ns.max() <= N - 1
    mt = max_iter_table(N, o)
    g = MT19937(seed)
    k, max_it = 0, o["max_iterations"]
    best, best_model, best_cnt = DBL_MAX, (1.0, np.eye(3), np.zeros(3)), 0
    rmin = cmin = pending = math.inf
    rows = max(1, min(BATCH, 4000000 // max(N, 1)))
    while True:
        nb = min(BATCH, max_it - k)
        samp = np.array([draw_sample(g, int(ns[k + q]), bool(br[k + q])) for q in range(nb)])
        s, R, t = fit4(a[samp], b[samp])
        cost, cnt, rm = np.zeros(nb), np.zeros(nb, np.int64), np.zeros(nb)
        for r0 in range(0, nb, rows):
            with np.errstate(invalid="ignore"):
                res = residuals(s[r0:r0 + rows], R[r0:r0 + rows], t[r0:r0 + rows], a, b)
                inl = res < thr
                cost[r0:r0 + rows] = np.cumsum(np.where(inl, res, thr), axis=1)[:, -1]
                cnt[r0:r0 + rows] = inl.sum(1)
                rm[r0:r0 + rows] = np.fmin.reduce(np.abs(res - thr), axis=1, initial=math.inf)
        done = False
        for q in range(nb):
            rmin = min(rmin, rm[q])
            # an exact tie is no hazard when both costs are N * threshold (no inlier: the residual margin covers it) or both
            # trials drew the same ordered sample (the same model bits in either implementation)
            if best != DBL_MAX and (cnt[q] or best_cnt):
                m = abs(cost[q] - best) / max(best, np.finfo(float).tiny)
                if cnt[q] != best_cnt:
                    cmin = min(cmin, m)  # a flip would change the iteration cap
                elif cost[q] < best and m >= CLEAR:
                    pending = math.inf  # a clear new best: both implementations hold it, earlier near-ties are moot
                else:
                    pending = min(pending, m)
            if cost[q] < best:
                best, best_cnt = cost[q], cnt[q]
                best_model = (float(s[q]), R[q].copy(), t[q].copy())
                if cnt[q] >= 4:
                    max_it = min(int(mt[cnt[q]]), max_it)
            if k + q + 1 >= max_it:
                iters = k + q + 1
                done = True
                break
        if done:
            return best_model, iters, rmin / thr, min(cmin, pending), best
        k += nb


def find_similarity(a, b, seed, o):
    """FindSimilarityTransform (refits as DESIGN.md 11): (s, R, t), msd (DBL_MAX: fewer than 4 inliers; NaN: N <= 2),
    inliers, iterations, residual margin, cost margin."""
    N = len(a)
    thr = o["threshold"]
    s, R, t = 1.0, np.eye(3), np.zeros(3)
    out = dict(inliers=0, iterations=0, residual_margin=math.inf, cost_margin=math.inf, prosac_cost=math.nan, prosac_s=1.0,
               prosac_R=np.eye(3), prosac_t=np.zeros(3))
    if N <= 2:
        out.update(s=s, R=R, t=t, msd=math.nan)
        return out
    if N > 5:
        (s, R, t), it, rmg, cmg, cost = prosac(a, b, seed, o)
        out.update(prosac_cost=cost, prosac_s=s, prosac_R=R.copy(), prosac_t=t.copy())
        with np.errstate(invalid="ignore"):
            inl = residuals(np.array([s]), R[None], t[None], a, b)[0] < thr
        out.update(inliers=int(inl.sum()), iterations=it, residual_margin=rmg, cost_margin=cmg)
        s, R, t = fit_all(a[inl], b[inl], s, R, t)
        if inl.sum() < 4:
            out.update(s=s, R=R, t=t, msd=DBL_MAX)
            return out
    if N <= 5 or out["inliers"] <= 5:
        s, R, t = fit_all(a, b, s, R, t)
    with np.errstate(invalid="ignore"):
        msd = float(residuals(np.array([s]), R[None], t[None], a, b)[0].sum() / N)
    out.update(s=s, R=R, t=t, msd=msd)
    return out


# ---------------------------------------------------------------- the join
def common_images(clusters):
    K = len(clusters)
    regs = [set(int(x) for x in c["image_ids"]) for c in clusters]
    common = {}
    for i in range(K):
        for j in range(i + 1, K):
            n = len(regs[i] & regs[j])
            if n:
                common[(i, j)] = n
    seps = sorted(set().union(*[regs[i] & regs[j] for (i, j) in common])) if common else []
    return common, seps


def join(clusters):
    """(i, j) -> (idx_i, idx_j): point indices of the correspondences in canonical order, from a sort of all observations."""
    K = len(clusters)
    img, p2d, cl, pt, rank = [], [], [], [], []
    for c, cd in enumerate(clusters):
        ob = np.asarray(cd["obs"], np.int64).reshape(-1, 3)
        ids = np.asarray(cd["point_ids"], np.uint64)
        rk = np.empty(len(ids), np.int64)
        rk[np.argsort(ids, kind="stable")] = np.arange(len(ids))
        img.append(ob[:, 0]), p2d.append(ob[:, 1]), cl.append(np.full(len(ob), c)), pt.append(ob[:, 2])
        rank.append(rk[ob[:, 2]] if len(ob) else np.zeros(0, np.int64))
    img, p2d, cl, pt, rank = (np.concatenate(x) if K else np.zeros(0, np.int64) for x in (img, p2d, cl, pt, rank))
    order = np.lexsort((cl, p2d, img))
    img, p2d, cl, pt, rank = img[order], p2d[order], cl[order], pt[order], rank[order]
    key = img * (1 << 32) + p2d
    heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
    lens = np.diff(np.r_[heads, len(key)])
    E = []
    for L in range(2, int(lens.max()) + 1 if len(lens) else 0):
        h = heads[lens == L]
        for x in range(L):
            for y in range(x + 1, L):
                u, v = h + x, h + y
                E.append(np.stack([cl[u], cl[v], rank[v], img[u], p2d[u], pt[u], pt[v]], 1))
    out = {}
    if not E:
        return out
    E = np.concatenate(E)
    E = E[np.lexsort((E[:, 4], E[:, 3], E[:, 2], E[:, 1], E[:, 0]))]
    pk = E[:, 0] * K + E[:, 1]
    hs = np.flatnonzero(np.r_[True, pk[1:] != pk[:-1]])
    for a, b in zip(hs, np.r_[hs[1:], len(E)]):
        out[(int(E[a, 0]), int(E[a, 1]))] = (E[a:b, 5], E[a:b, 6])
    return out


def join_literal(clusters, i, j):
    """FindCommon3DPoints itself for one pair, with j's points in ascending id and track elements by (image, point2D_idx)."""
    ci, cj = clusters[i], clusters[j]
    common = set(int(x) for x in ci["image_ids"]) & set(int(x) for x in cj["image_ids"])
    of_i = {(int(a), int(b)): int(p) for a, b, p in np.asarray(ci["obs"]).reshape(-1, 3)}
    tracks = {}
    for a, b, p in np.asarray(cj["obs"]).reshape(-1, 3):
        tracks.setdefault(int(p), []).append((int(a), int(b)))
    src, ref = [], []
    for p in sorted(tracks, key=lambda q: int(cj["point_ids"][q])):
        for el in sorted(tracks[p]):
            if el[0] in common and el in of_i:
                src.append(of_i[el])
                ref.append(p)
    return np.array(src, np.int64), np.array(ref, np.int64)


# ---------------------------------------------------------------- the graph
def float_margin(w):
    f = np.float32(w)
    lo = (float(np.nextafter(f, np.float32(-np.inf))) + float(f)) / 2.0
    hi = (float(f) + float(np.nextafter(f, np.float32(np.inf)))) / 2.0
    return min(w - lo, hi - w) / abs(w) if w != 0 else math.inf


def graph(K, edges, sims):
    """edges: [(float32 weight, i, j)]; sims[(a, b)] = (s, R, t) of a -> b.  Largest component (ties: smaller index),
    Kruskal (ties (min, max)), FindAnchorNode (two nodes: the smaller goes), ComputePath."""
    uf = list(range(K))

    def find(x):
        while uf[x] != x:
            uf[x] = uf[uf[x]]
            x = uf[x]
        return x

    for w, i, j in edges:
        a, b = find(i), find(j)
        if a != b:
            uf[max(a, b)] = min(a, b)
    size = [0] * K
    for c in range(K):
        size[find(c)] += 1
    root = 0
    for c in range(K):
        if size[c] > size[root]:
            root = c
    inc = [find(c) == root for c in range(K)]
    ce = sorted([e for e in edges if inc[e[1]]], key=lambda e: (e[0], e[1], e[2]))
    uf = list(range(K))
    adj = [[] for _ in range(K)]
    mst = []
    for w, i, j in ce:
        a, b = find(i), find(j)
        if a == b:
            continue
        uf[a] = b
        adj[i].append(j)
        adj[j].append(i)
        mst.append((i, j))
    parent = [-1] * K
    deg = [len(x) for x in adj]
    alive = sum(1 for d in deg if d)
    gone = [False] * K
    anchor = 0
    while alive > 1:
        if alive == 2:
            leaves = [min(c for c in range(K) if deg[c] and not gone[c])]
        else:
            leaves = [c for c in range(K) if not gone[c] and deg[c] == 1]
        if not leaves:
            break
        for c in leaves:
            for nb in adj[c]:
                if not gone[nb]:
                    parent[c] = nb
                    anchor = nb
                    deg[nb] -= 1
                    break
            gone[c] = True
            alive -= 1
    S = np.ones(K)
    Rs = np.tile(np.eye(3), (K, 1, 1))
    ts = np.zeros((K, 3))
    for c in range(K):
        if not inc[c] or c == anchor:
            continue
        s, R, t = 1.0, np.eye(3), np.zeros(3)
        u = c
        while u != anchor:
            es, eR, et = sims[(u, parent[u])]
            s = es * s
            nR = np.zeros((3, 3))
            nt = np.zeros(3)
            for i in range(3):
                for j in range(3):
                    nR[i, j] = eR[i, 0] * R[0, j] + eR[i, 1] * R[1, j] + eR[i, 2] * R[2, j]
                sR = [es * eR[i, 0], es * eR[i, 1], es * eR[i, 2]]
                nt[i] = (sR[0] * t[0] + sR[1] * t[1] + sR[2] * t[2]) + et[i]
            R, t = nR, nt
            u = parent[u]
        S[c], Rs[c], ts[c] = s, R, t
    return dict(anchor=anchor, in_component=np.array(inc), mst_parent=np.array([parent[c] if inc[c] else -1 for c in range(K)]),
                s=S, R=Rs, t=ts, mst=mst)


def align(clusters, options=None, seeds=None):
    """SfMAligner::Align up to the transforms, as dsm_align_clusters.  seeds: None or [K, K] (a -> b)."""
    o = options or default_options()
    K = len(clusters)
    common, seps = common_images(clusters)
    corr = join(clusters)
    xyz = [np.asarray(c["xyz"], np.float64).reshape(-1, 3) for c in clusters]
    pairs, edges, sims = [], [], {}
    for (i, j) in sorted(common):
        if common[(i, j)] < 2:
            continue
        ii, jj = corr.get((i, j), (np.zeros(0, np.int64), np.zeros(0, np.int64)))
        a, b = xyz[i][ii], xyz[j][jj]
        N = len(a)
        rec = dict(i=i, j=j, num_common_images=common[(i, j)], num_correspondences=N, edge=False)
        dirs = []
        for d in (0, 1):
            x, y, (p, q) = (a, b, (i, j)) if d == 0 else (b, a, (j, i))
            seed = int(seeds[p][q]) if seeds is not None else align_seed(i, j, d, o["random_seed"])
            dirs.append(find_similarity(x, y, seed, o))
        for key in ("msd", "s", "inliers", "iterations", "residual_margin", "cost_margin", "prosac_cost", "prosac_s", "prosac_R",
                    "prosac_t"):
            rec[key] = [dirs[0][key], dirs[1][key]]
        rec["R"], rec["t"] = [dirs[0]["R"], dirs[1]["R"]], [dirs[0]["t"], dirs[1]["t"]]
        rec["weight"] = math.nan
        rec["weight_margin"] = rec["float_margin"] = math.inf
        if N >= 3:
            w = rec["msd"][1] if rec["msd"][0] < rec["msd"][1] else rec["msd"][0]  # std::max
            rec["weight"] = w
            if not (math.isnan(rec["msd"][0]) or math.isnan(rec["msd"][1]) or w == DBL_MAX):
                rec["weight_margin"] = abs(w - o["max_reprojection_error"]) / o["max_reprojection_error"]
                if w <= o["max_reprojection_error"]:
                    rec["edge"] = True
                    rec["float_margin"] = float_margin(w)
                    edges.append((np.float32(w), i, j))
                    sims[(i, j)] = (dirs[0]["s"], dirs[0]["R"], dirs[0]["t"])
                    sims[(j, i)] = (dirs[1]["s"], dirs[1]["R"], dirs[1]["t"])
        rec["margin"] = min(min(rec["residual_margin"]), min(rec["cost_margin"]), rec["weight_margin"], rec["float_margin"])
        pairs.append(rec)
    res = graph(K, edges, sims)
    res.update(pairs=pairs, separators=np.array(seps, np.uint32), num_edges=len(edges))
    return res


# ---------------------------------------------------------------- the synthetic scene
def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(n_images=60, n_clusters=4, overlap=6, points_per_image=60, track=4, noise=0.003, wrong=0.05, drop=0.1, extent=3.0,
          seed=0, wrong_per_cluster=None):
    """A sequence of n_images; every ground-truth point is seen by `track` consecutive images (point2D_idx dense per image).
    Cluster c registers a window of consecutive images (windows overlap by `overlap` images) and holds every point with at
    least 2 kept observations in it, as x_c = s_c R_c X + t_c + noise (the planted Sim3).  A fraction `wrong` of each
    cluster's points gets another point's coordinates (a wrong association); a fraction `drop` of observations is dropped.
    Point ids are random and unique per cluster; points and observations are shuffled."""
    rng = np.random.default_rng(seed)
    n_pts = n_images * points_per_image // track
    X = rng.uniform(-extent, extent, (n_pts, 3))
    first = rng.integers(0, n_images - track + 1, n_pts)
    obs_img, obs_pt = [], []
    for p in range(n_pts):
        for k in range(track):
            obs_img.append(first[p] + k)
            obs_pt.append(p)
    obs_img, obs_pt = np.array(obs_img), np.array(obs_pt)
    p2d = np.zeros(len(obs_img), np.int64)
    cnt = np.zeros(n_images, np.int64)
    for e in rng.permutation(len(obs_img)):
        p2d[e] = cnt[obs_img[e]]
        cnt[obs_img[e]] += 1
    step = (n_images - overlap) / n_clusters
    clusters, planted = [], []
    for c in range(n_clusters):
        lo, hi = int(round(c * step)), min(n_images, int(round((c + 1) * step)) + overlap)
        s = float(rng.uniform(0.5, 2.0))
        R = random_rotation(rng)
        t = rng.uniform(-5, 5, 3)
        planted.append((s, R, t))
        keep = (obs_img >= lo) & (obs_img < hi) & (rng.random(len(obs_img)) >= drop)
        pts, counts = np.unique(obs_pt[keep], return_counts=True)
        pts = pts[counts >= 2]
        local = {int(p): q for q, p in enumerate(pts)}
        xyz = s * (X[pts] @ R.T) + t + rng.normal(0, noise, (len(pts), 3))
        w = wrong if wrong_per_cluster is None else wrong_per_cluster[c]
        bad = rng.random(len(pts)) < w
        if bad.any():
            xyz[bad] = s * (rng.uniform(-extent, extent, (int(bad.sum()), 3)) @ R.T) + t
        sel = keep & np.isin(obs_pt, pts)
        ob = np.stack([obs_img[sel], p2d[sel], [local[int(p)] for p in obs_pt[sel]]], 1) if sel.any() else np.zeros((0, 3), np.int64)
        ids = rng.choice(1 << 40, len(pts), replace=False).astype(np.uint64)
        perm = rng.permutation(len(pts))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        ob = ob[rng.permutation(len(ob))]
        if len(ob):
            ob[:, 2] = inv[ob[:, 2]]
        clusters.append(dict(image_ids=np.arange(lo, hi, dtype=np.uint32), point_ids=ids[perm], xyz=xyz[perm],
                             obs=ob.astype(np.uint32)))
    return clusters, planted


def planted_relative(planted, a, b):
    """the Sim3 a -> b implied by the planted transforms: x_b = s R x_a + t."""
    sa, Ra, ta = planted[a]
    sb, Rb, tb = planted[b]
    s = sb / sa
    R = Rb @ Ra.T
    return s, R, tb - s * (R @ ta)
