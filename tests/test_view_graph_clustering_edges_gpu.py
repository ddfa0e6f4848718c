"""View-graph clustering on the device (dsm_view_graph_cluster) where tests/test_view_graph_clustering_gpu.py
does not go: the sizes of the project's target (10 000 images in 100 clusters), the chunk cap, one-row tiles and short last
chunks of the Gram kernel, ncv == N, disconnected graphs and repeated eigenvalues, the k-means iteration cap and near-duplicate
rows, eigen_tolerance, ids next to 2^32 and the input rules.  (An empty centre inside the device's Lloyd iterations is not here:
no seeded graph gave one with clear margins; see test_kmeans_records_an_empty_centre on the CPU side.)

Every spectral case goes through independent_check: the residuals ||L x - theta x||, X^T X and the Rayleigh quotients
recomputed in np.longdouble from the returned vectors with an L = D_cnt - S built here from the raw pair list, and the
Ritz values against scipy's spectrum of that L.  Nothing in it trusts a number the device reports about itself."""
import math
import time

import numpy as np
import pytest

from tests import view_graph_clustering_ref as ref
from tests.test_view_graph_clustering_cpu import (clear_share, components, planted, planted_sparse, same_partition, scale_case,
                                                  twin_blocks)
from tests.test_view_graph_clustering_gpu import (EV_RTOL, MARGIN, _opts, check_same, check_same_where_clear, check_spectrum,
                                                  random_graph, sequence_graph)

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
EPS23 = EPS ** (2.0 / 3.0)
DENSE_BELOW = 2500  # images below which the reference spectrum is a dense eigh

# The constants of independent_check's bounds (u = EPS, n = images, m = ncv, ||L|| = the infinity norm of L):
# C_RES: the device forms L X as (L Q) Z and X as Q Z: one sparse row sum (at most n terms) and two m-term sums per entry,
#   then d = LX - theta X and the sum of squares in double.  Each is a dot product of length <= n with relative error
#   <= n u against ||L|| ||x||; four such steps (spmm, the two block products, the residual itself) stack to 4 n u ||L||.
#   The longdouble recomputation's own error is 2^-11 of that and is covered by the same term.
C_RES = 4.0
# C_ORTH: Cholesky QR twice leaves ||Q^T Q - I||_2 <= 6 (n m + m (m + 1)) u (Yamamoto et al. 2015, Theorem 3.2, reached
#   after the shifted pass: Fukaya et al. 2020); Z of the Jacobi sweeps and the product Q Z add (m + 1) m u <= the second
#   term again and one more n m u: 8 in all.
C_ORTH = 8.0
# C_REF: LAPACK / ARPACK's backward error in the reference eigenvalues, 100 u ||L|| (the figure check_spectrum uses).
C_REF = 100.0


def build_L(pairs, weights, use=None):
    """(ids ascending, rows, cols, values sorted by row, row starts) of L = D_cnt - S from the raw list: the first occurrence
    of an unordered pair is the edge, D counts edges, S holds weights.  Written apart from the restatement's prepare()."""
    seen, edges = set(), []
    for e, ((a, b), w) in enumerate(zip(np.asarray(pairs, np.int64).reshape(-1, 2).tolist(), np.asarray(weights).tolist())):
        if use is not None and not use[e]:
            continue
        key = (a, b) if a < b else (b, a)
        if key not in seen:
            seen.add(key)
            edges.append((key[0], key[1], w))
    ids = sorted({v for a, b, _ in edges for v in (a, b)})
    pos = {v: i for i, v in enumerate(ids)}
    i = np.array([pos[a] for a, _, _ in edges])
    j = np.array([pos[b] for _, b, _ in edges])
    w = np.array([w for _, _, w in edges], np.float64)
    n = len(ids)
    cnt = np.bincount(np.concatenate([i, j]), minlength=n).astype(np.float64)
    rows = np.concatenate([i, j, np.arange(n)])
    cols = np.concatenate([j, i, np.arange(n)])
    vals = np.concatenate([-w, -w, cnt])
    o = np.argsort(rows, kind="stable")
    rows, cols, vals = rows[o], cols[o], vals[o]
    starts = np.searchsorted(rows, np.arange(n))  # every image has its diagonal entry: no empty row
    return np.array(ids, np.int64), rows, cols, vals, starts


def matvec_ld(rows, cols, vals, starts, X):
    """L X in np.longdouble, eight columns at a time."""
    X = X.astype(np.longdouble)
    v = vals.astype(np.longdouble)[:, None]
    out = np.empty_like(X)
    for c in range(0, X.shape[1], 8):
        out[:, c:c + 8] = np.add.reduceat(v * X[cols, c:c + 8], starts, axis=0)
    return out


def reference_spectrum(n, rows, cols, vals, nev):
    """The nev algebraically smallest eigenpairs of L: dense eigh below DENSE_BELOW images, else scipy's eigsh.  L is
    indefinite (D counts, S weighs), so the wanted end is the algebraically smallest one, not the one near 0: Lanczos on L
    with which="SA", to machine precision."""
    import scipy.sparse as sp
    L = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    if n < DENSE_BELOW:
        lam, V = np.linalg.eigh(L.toarray())
        return lam[:nev], V[:, :nev]
    import scipy.sparse.linalg as spla
    lam, V = spla.eigsh(L, k=nev, which="SA", tol=0, ncv=max(3 * nev, 40), v0=np.ones(n) / math.sqrt(n))
    o = np.argsort(lam)
    return lam[o], V[:, o]


def independent_check(dev, pairs, weights, use=None, tol=1e-10, unique=True, name=""):
    """Item by item what the module docstring says.  `unique`: the k-dimensional invariant subspace is well defined, so the
    principal sine is bounded too (Davis-Kahan).  Returns the figures it printed."""
    r = dev["report"]
    ids, rows, cols, vals, starts = build_L(pairs, weights, use)
    n, m = len(ids), int(r.ncv)
    X, theta = dev["eigenvectors"], dev["eigenvalues"]
    k = X.shape[1]
    assert np.array_equal(dev["image_ids"], ids) and X.shape == (n, k) and len(theta) == m
    norm_L = float(np.add.reduceat(np.abs(vals), starts).max())
    Xl, th = X.astype(np.longdouble), theta[:k].astype(np.longdouble)
    LX = matvec_ld(rows, cols, vals, starts, X)
    res = np.sqrt(((LX - Xl * th) ** 2).sum(0)).astype(np.float64)
    scale = np.maximum(EPS23, np.abs(theta[:k]))
    recomp = C_RES * n * EPS * norm_L
    # 1a. the recomputed residuals meet the stopping rule: ratio <= tol (1 + slack), slack = recomp / (tol scale) per column
    slack = float((recomp / (tol * scale)).max())
    ratio = float((res / scale).max())
    assert (res <= tol * scale + recomp).all(), (name, ratio, tol, slack)
    # 1b. ... and agree with the ratio the device reports: |max a - max b| <= max |a - b| <= recomp / scale
    agree = abs(ratio - r.max_eigen_residual_ratio)
    assert r.max_eigen_residual_ratio <= tol
    assert agree <= float((recomp / scale).max()), (name, ratio, r.max_eigen_residual_ratio)
    assert abs(float(res.max()) - r.max_eigen_residual) <= recomp, (name, res.max(), r.max_eigen_residual)
    # 2. orthonormality
    G = (Xl.T @ Xl).astype(np.float64)
    orth = float(np.abs(G - np.eye(k)).max())
    orth_bound = C_ORTH * (n * m + m * (m + 1)) * EPS
    assert orth <= orth_bound, (name, orth, orth_bound)
    # 3. Rayleigh quotients: |rho - theta| = |x^T r| / x^T x <= ||r|| / ||x||
    rho = ((Xl * LX).sum(0) / (Xl * Xl).sum(0)).astype(np.float64)
    rq = np.abs(rho - theta[:k])
    assert (rq <= res / np.sqrt(np.diag(G)) + recomp).all(), (name, rq.max())
    # 4. the Ritz values are the k smallest eigenvalues: an orthonormal block with residual matrix R has k eigenvalues of L
    # within ||R||_2 <= sqrt(k) max ||r_j|| of its Ritz values (Kahan 1967; Parlett, Theorem 11.5.1), in order
    lam, V = reference_spectrum(n, rows, cols, vals, min(k + 1, n))
    th_err = float(np.abs(theta[:k] - lam[:k]).max())
    th_bound = math.sqrt(k) * float(res.max()) / (1.0 - orth_bound) + C_REF * EPS * norm_L
    assert th_err <= th_bound, (name, th_err, th_bound)
    out = {"n": n, "k": k, "ncv": m, "norm_L": norm_L, "ratio": ratio, "reported": r.max_eigen_residual_ratio, "slack": slack,
           "agree": agree, "orth": orth, "orth_bound": orth_bound, "rq": float(rq.max()), "theta_err": th_err,
           "theta_bound": th_bound, "iterations": int(r.eigen_iterations), "device_ms": float(r.device_ms)}
    if unique and len(lam) > k:
        # 5. Davis-Kahan: sin <= ||R||_2 / gap, gap between the Ritz values and the rest of L's spectrum
        gap = float(lam[k] - max(lam[k - 1], theta[k - 1]))
        assert gap > 0
        sine = ref.principal_sine(X, V[:, :k])
        sine_bound = (math.sqrt(k) * float(res.max()) + C_REF * EPS * norm_L) / gap + orth_bound
        assert sine <= sine_bound, (name, sine, sine_bound)
        out.update(sine=sine, sine_bound=sine_bound, gap=gap)
    print("independent_check %s: %s" % (name, " ".join("%s=%.3g" % kv for kv in out.items())))
    return out


def run_both(dsm, pairs, w, ub, use=None, name="", tol=None, **kw):
    """The device and the restatement on one graph; the independent check, the subspace against the restatement's, the
    labels where the margins are clear."""
    okw = dict(kw)
    if tol is not None:
        okw["eigen_tolerance"] = tol
    dev = dsm.cluster_view_graph(pairs, w, use=use, options=_opts(num_images_ub=ub, **okw))
    exp = ref.cluster(pairs, w, use=use, num_images_ub=ub, **kw)
    independent_check(dev, pairs, w, use, tol or 1e-10, name=name)
    full = check_same_where_clear(dev, exp)
    return dev, exp, full


# ---------------------------------------------------------------- 1. the existing fixtures through the independent check
EXISTING = {
    "planted_6": (lambda: planted(6, 100, 1)[:2], 100),
    "planted_20": (lambda: planted(20, 100, 4)[:2], 100),
    "random_1000": (lambda: random_graph(1000, 8, 21), 100),
    "sequence_400": (lambda: sequence_graph(400, 4, 22), 100),
}


@pytest.mark.parametrize("name", sorted(EXISTING))
def test_existing_fixtures_pass_the_independent_check(dsm, name):
    build, ub = EXISTING[name]
    pairs, w = build()
    dev = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=ub))
    independent_check(dev, pairs, w, name=name)


# ---------------------------------------------------------------- 2. scale
def _scale(dsm, name):
    pairs, w, ub, exp = scale_case(name)
    t = time.time()
    dev = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=ub))
    wall = time.time() - t
    fig = independent_check(dev, pairs, w, name=name)
    k = exp["k"]
    ev = exp["eigenvalues"]
    assert np.all(np.abs(dev["eigenvalues"][:k] - ev[:k]) <= EV_RTOL * np.maximum(np.abs(ev[:k]), 1.0))
    gap = ev[k] - ev[k - 1]
    sine = ref.principal_sine(dev["eigenvectors"], exp["subspace"])
    assert sine <= 2 * fig["sine_bound"], (sine, fig["sine_bound"])  # both sides within the bound of the true subspace
    assert gap > 0
    draws, share = clear_share(exp, MARGIN)
    assert draws and share >= 0.9
    full = check_same_where_clear(dev, exp)
    r = dev["report"]
    print("scale %s: device_ms=%.1f wall_s=%.2f eigen_iterations=%d kmeans_iterations=%d operator_applications=%d full=%s"
          % (name, r.device_ms, wall, r.eigen_iterations, r.kmeans_iterations, r.operator_applications, full))
    return dev, exp


def test_scale_10000_images_100_clusters(dsm):
    dev, _ = _scale(dsm, "10000_k100")
    r = dev["report"]
    assert (r.num_images, r.num_clusters, r.ncv) == (10000, 100, 200)


def test_scale_chunk_cap_64_and_one_row_last_chunk(dsm):
    dev, exp = _scale(dsm, "16593_cap64")  # ceil(16593 / 256) = 65 > 64; chunk_rows 260 -> 272, 62 chunks, 16593 - 61 * 272 = 1
    assert (dev["report"].num_images, dev["report"].ncv) == (16593, 8)
    assert ref.min_margin(exp) >= MARGIN  # the full comparison ran


@pytest.mark.parametrize("name", ["1601_one_row_tile", "257_short_chunk"])
def test_scale_one_row_last_tile(dsm, name):
    dev, exp = _scale(dsm, name)
    assert dev["report"].num_images % 16 == 1
    assert ref.min_margin(exp) >= MARGIN


# ---------------------------------------------------------------- 3. ncv == N: no filter, Rayleigh-Ritz on the full space
def small_graph(n, seed):
    pairs, w = random_graph(n, 3, seed)
    assert len(np.unique(pairs)) == n
    return pairs, w


# (N, num_images_ub): 2k >= N > k wherever an integer k = N // ub allows it.  N = 17 allows none (k = 8 gives 2k = 16, k = 17
# is refused), so it runs with ncv = N - 1, the filter damping a single eigenvalue, and N = 16 stands in for the large case.
@pytest.mark.parametrize("n,ub", [(6, 2), (10, 2), (16, 2), (17, 2), (6, 3), (10, 3)])
def test_block_as_wide_as_the_graph(dsm, n, ub):
    pairs, w = small_graph(n, 70 + n)
    k = n // ub
    dev, exp, _ = run_both(dsm, pairs, w, ub, name="ncv_%d_%d" % (n, ub))
    r = dev["report"]
    assert r.ncv == min(2 * k, n)
    if 2 * k >= n:
        assert r.ncv == n
        # theta is the whole spectrum of the dense L, to rounding: Q spans everything, so the only errors are Q's departure
        # from orthonormal (C_ORTH (n m + m (m + 1)) u) and Jacobi's backward error (m u), both times ||L||
        L = ref.laplacian(n, ref.prepare(pairs, w)[1])
        lam = np.linalg.eigvalsh(L)
        norm_L = np.abs(L).sum(1).max()
        bound = (C_ORTH * (n * n + n * (n + 1)) + n + C_REF) * EPS * norm_L
        err = np.abs(dev["eigenvalues"] - lam).max()
        print("ncv == N = %d: theta error %.3g (bound %.3g), %d iterations" % (n, err, bound, r.eigen_iterations))
        assert err <= bound, (err, bound)


# ---------------------------------------------------------------- 4. degenerate spectra
def _repeat_and_shuffle(dsm, pairs, w, opts, first, seed):
    """Byte-identical results from a repeat and from a shuffled, half-flipped input list."""
    keys = ("image_ids", "labels", "offsets", "eigenvalues", "eigenvectors")
    again = dsm.cluster_view_graph(pairs, w, options=opts)
    for key in keys + ("edge_cluster",):
        assert first[key].tobytes() == again[key].tobytes(), key
    rng = np.random.default_rng(seed)
    o = rng.permutation(len(pairs))
    sp = pairs[o].copy()
    flip = rng.random(len(o)) < 0.5
    sp[flip] = sp[flip][:, ::-1]
    c = dsm.cluster_view_graph(sp, w[o], options=opts)
    for key in keys:
        assert first[key].tobytes() == c[key].tobytes(), key
    return c, np.argsort(o)


def test_exactly_k_components(dsm):
    pairs, w, truth = planted_sparse([100, 100, 100], 5, 81, n_weak=0)
    assert components(pairs) == 3
    dev, exp, full = run_both(dsm, pairs, w, 100, name="k_components")
    assert full
    assert same_partition(dev["labels"], dev["image_ids"], truth)
    assert dev["report"].num_lost_edges == 0 and (dev["edge_cluster"] >= 0).all()


def test_fewer_than_k_components(dsm):
    pairs, w, truth = planted_sparse([200, 200], 5, 82, n_weak=0)
    assert components(pairs) == 2
    dev, exp, _ = run_both(dsm, pairs, w, 100, name="2_components_k4")
    assert dev["report"].num_clusters == 4
    comp = np.array([truth[v] for v in dev["image_ids"].tolist()])
    assert all(len(set(comp[dev["labels"] == c].tolist())) <= 1 for c in range(4))  # no cluster spans two components


def test_more_than_k_components(dsm):
    pairs, w, truth = planted_sparse([60] * 5, 4, 83, n_weak=0)
    assert components(pairs) == 5
    dev, exp, _ = run_both(dsm, pairs, w, 100, name="5_components_k3")  # distinct weights: the three lowest blocks, unique
    assert dev["report"].num_clusters == 3


def _either_status(dsm, pairs, w, ub, tol, name):
    """A graph whose wanted subspace is not unique: DSM_OK with a result that passes the independent check and does not depend
    on repeats or the input order, or DSM_ERR_NOT_CONVERGED (6) with the residual message.  Returns the status seen."""
    from dagsfm_amd import capi
    opts = _opts(num_images_ub=ub, eigen_tolerance=tol)
    t = time.time()
    try:
        dev = dsm.cluster_view_graph(pairs, w, options=opts)
    except capi.DsmError as e:
        print("status %s tol=%g: NOT_CONVERGED after %.2f s: %s" % (name, tol, time.time() - t, e))
        assert "residual" in str(e) and "dsm error 6:" in str(e), str(e)
        with pytest.raises(capi.DsmError) as again:  # the same end from a repeat
            dsm.cluster_view_graph(pairs, w, options=opts)
        assert str(again.value) == str(e)
        return "NOT_CONVERGED"
    print("status %s tol=%g: OK after %.2f s, %d iterations" % (name, tol, time.time() - t, dev["report"].eigen_iterations))
    independent_check(dev, pairs, w, tol=tol, unique=False, name=name)
    _repeat_and_shuffle(dsm, pairs, w, opts, dev, 84)
    return "OK"


@pytest.mark.parametrize("tol", [1e-10, 1e-2])
def test_more_than_k_components_of_a_true_laplacian(dsm, tol):
    """Unit weights make L the graph Laplacian: eigenvalue 0 five times, k = 3.  The stopping rule divides by
    max(eps^(2/3), |theta|), so at theta = 0 the default tolerance asks for a residual of 4e-21."""
    pairs, w, _ = planted_sparse([60] * 5, 4, 83, n_weak=0, unit_weights=True)
    _either_status(dsm, pairs, w, 100, tol, "laplacian_5_components_k3")


@pytest.mark.parametrize("tol", [1e-10, 1e-2])
def test_exactly_k_components_of_a_true_laplacian(dsm, tol):
    pairs, w, truth = planted_sparse([100, 100, 100], 5, 81, n_weak=0, unit_weights=True)
    _either_status(dsm, pairs, w, 100, tol, "laplacian_3_components_k3")


def test_twin_blocks_repeat_an_eigenvalue_across_the_boundary(dsm):
    pairs, w = twin_blocks(150, 5, 85)
    assert components(pairs) == 2
    lam = np.linalg.eigvalsh(ref.laplacian(300, ref.prepare(pairs, w)[1]))
    assert abs(lam[3] - lam[2]) <= 1e-9 and lam[4] - lam[3] > 1.0  # k = 3 cuts the second pair
    assert _either_status(dsm, pairs, w, 100, 1e-10, "twin_blocks") in ("OK", "NOT_CONVERGED")


def test_zero_weight_edges(dsm):
    pairs, w = random_graph(600, 6, 86)
    w = w.copy()
    w[np.random.default_rng(87).random(len(w)) < 0.3] = 0
    assert (w == 0).sum() > 500
    dev, exp, _ = run_both(dsm, pairs, w, 100, name="zero_weights")
    check_spectrum(dev, exp)
    assert dev["report"].num_edges == len(pairs)  # counted in D, absent from S
    _repeat_and_shuffle(dsm, pairs, w, _opts(num_images_ub=100), dev, 88)


# ---------------------------------------------------------------- 5. k-means
# (graph, num_images_ub, Lloyd iterations of the restatement without a cap); every margin of both is >= MARGIN
KMEANS = {
    "sequence_600": (lambda: sequence_graph(600, 3, 51), 50, 14),
    "random_1000": (lambda: random_graph(1000, 8, 61), 100, 17),
}


@pytest.mark.parametrize("cap", [1, 7, 8, 9, 16])
@pytest.mark.parametrize("name", sorted(KMEANS))
def test_kmeans_iteration_cap(dsm, name, cap):
    build, ub, natural = KMEANS[name]
    pairs, w = build()
    dev = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=ub, max_kmeans_iterations=cap))
    exp = ref.cluster(pairs, w, num_images_ub=ub, max_kmeans_iterations=cap)
    assert ref.min_margin(exp) >= MARGIN
    assert exp["kmeans_iterations"] == min(cap, natural)
    assert dev["report"].kmeans_iterations == min(cap, natural)
    check_same(dev, exp)


def test_near_duplicate_rows(dsm):
    """Twelve groups of twins: images with the same neighbours and the same weights, whose spectral rows agree to rounding.
    The k-means++ weights are then exact zeros (the centres) next to squared distances of rounding size and ordinary ones."""
    pairs, w = duplicate_row_graph()
    dev, exp, _ = run_both(dsm, pairs, w, 100, name="twins")
    lab = dict(zip(dev["image_ids"].tolist(), dev["labels"].tolist()))
    for g in range(12):
        assert len({lab[1000 + 10 * g + t] for t in range(10)}) == 1  # twins stay together


def duplicate_row_graph():
    """300 images of random_graph plus 12 groups of 10 twins: every twin of group g is joined to the same 3 images with the
    same 3 weights, and to no other twin."""
    pairs, w = random_graph(300, 6, 89)
    rng = np.random.default_rng(90)
    extra, ew = [], []
    for g in range(12):
        nb = rng.choice(300, 3, replace=False)
        wt = rng.integers(100, 400, 3)
        for t in range(10):
            extra += [(1000 + 10 * g + t, int(v)) for v in nb]
            ew += wt.tolist()
    return np.concatenate([pairs, np.array(extra, np.uint32)]), np.concatenate([w, np.array(ew, np.int32)])


# ---------------------------------------------------------------- 6. options, ids, input hygiene
def test_eigen_tolerance(dsm):
    pairs, w = random_graph(1000, 8, 21)
    its = {}
    for tol in (1e-6, 1e-10, 1e-12):
        dev = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=100, eigen_tolerance=tol))
        independent_check(dev, pairs, w, tol=tol, name="tol_%g" % tol)
        its[tol] = dev["report"].eigen_iterations
    print("eigen iterations by tolerance:", its)
    assert its[1e-6] <= its[1e-10] <= its[1e-12]


@pytest.mark.parametrize("tol", [0.0, -1e-10, float("nan")])
def test_eigen_tolerance_out_of_range(dsm, tol):
    from dagsfm_amd import capi
    pairs, w = random_graph(300, 6, 11)
    with pytest.raises(capi.DsmError) as e:
        dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=100, eigen_tolerance=tol))
    assert "dsm error 1:" in str(e.value) and "option out of range" in str(e.value)


def test_ids_next_to_2_pow_32(dsm):
    pairs, w = random_graph(1000, 8, 21)
    big = np.sort(np.random.default_rng(91).choice(5000, 1000, replace=False)).astype(np.uint32) + np.uint32(2 ** 32 - 5000)
    assert big.max() >= 2 ** 32 - 50 and big.dtype == np.uint32
    hi = big[pairs]  # ascending in the small ids: the same vertex order
    a = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=100))
    b = dsm.cluster_view_graph(hi, w, options=_opts(num_images_ub=100))
    independent_check(b, hi, w, name="ids_2_pow_32")
    assert np.array_equal(b["image_ids"], big[a["image_ids"]])
    # the start block hashes the ids, so the two runs converge along different paths to the same subspace: the partitions
    # agree wherever the restatement's margins are clear, the numbering included (it follows the k-means++ draws)
    exp = ref.cluster(hi, w, num_images_ub=100)
    check_same_where_clear(b, exp)
    n = len(exp["labels"])
    clear = (exp["lloyd_margins"].reshape(-1, n) >= MARGIN).all(axis=0)
    assert np.array_equal(a["labels"][clear], b["labels"][clear])


def test_duplicate_pairs_in_both_orientations(dsm):
    pairs, w = random_graph(600, 6, 92)
    rng = np.random.default_rng(93)
    dup = rng.choice(len(pairs), 400, replace=False)
    rev = pairs[dup][:, ::-1].copy()
    rev[:200] = rev[:200][:, ::-1]  # half of the repeats in the same orientation
    all_pairs = np.concatenate([pairs, rev])
    all_w = np.concatenate([w, rng.integers(15, 500, 400).astype(np.int32)])  # other weights: they must not count
    base = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=100))
    dev = dsm.cluster_view_graph(all_pairs, all_w, options=_opts(num_images_ub=100))
    independent_check(dev, all_pairs, all_w, name="duplicates")
    assert (dev["edge_cluster"][len(pairs):] == -1).all()
    assert dev["report"].num_edges == len(pairs)
    for key in ("image_ids", "labels", "offsets", "eigenvalues", "eigenvectors"):
        assert base[key].tobytes() == dev[key].tobytes(), key
    assert base["edge_cluster"].tobytes() == dev["edge_cluster"][:len(pairs)].tobytes()
    # with a mask that hides the first occurrences, the later ones are the edges, with their own weights
    use = np.ones(len(all_pairs), np.uint8)
    use[dup] = 0
    dev2, exp2, _ = run_both(dsm, all_pairs, all_w, 100, use=use, name="duplicates_masked")
    assert (dev2["edge_cluster"][dup] == -1).all() and (dev2["edge_cluster"][len(pairs):] != -1).all()


def test_use_mask_that_empties_the_list(dsm):
    pairs, w = random_graph(300, 6, 11)
    dev = dsm.cluster_view_graph(pairs, w, use=np.zeros(len(pairs), np.uint8), options=_opts(num_images_ub=100))
    assert len(dev["image_ids"]) == 0 and len(dev["labels"]) == 0 and len(dev["clusters"]) == 0
    assert (dev["edge_cluster"] == -1).all() and len(dev["edge_cluster"]) == len(pairs)
    assert dev["report"].num_images == 0 and dev["eigenvalues"] is None


def test_labels_in_out_of_range(dsm):
    from dagsfm_amd import capi
    pairs, w = random_graph(300, 6, 11)
    lab = np.zeros(300, np.uint32)
    lab[17] = 300
    with pytest.raises(capi.DsmError) as e:
        dsm.cluster_view_graph(pairs, w, labels_in=lab, options=_opts(num_images_ub=100))
    assert "dsm error 1:" in str(e.value) and "label" in str(e.value)
    lab[17] = 299  # the largest legal label: 300 clusters, 298 of them empty
    dev = dsm.cluster_view_graph(pairs, w, labels_in=lab, options=_opts(num_images_ub=100))
    assert dev["report"].num_clusters == 300 and len(dev["clusters"][299]) >= 1 and len(dev["clusters"][150]) == 0
