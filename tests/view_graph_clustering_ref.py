"""numpy restatement of the view-graph clustering (dsm_view_graph_cluster; DistributedMapperController::ClusteringScenes,
src/controllers/distributed_mapper_controller.cpp:633-657; DESIGN.md 10, "View-graph clustering").

SPECTRAL (src/clustering/spectral_cluster.cpp:52-176): the dense L = D_cnt - S (D_cnt counts the edges of an image, S holds
the weights), numpy.linalg.eigh (scipy's eigsh above SPARSE_ABOVE images) for its k algebraically smallest eigenvectors, then KMeans (src/clustering/kmeans.h:158-235)
with k-means++ driven by a restatement of libstdc++'s std::mt19937_64, uniform_int_distribution<size_t> and
discrete_distribution<size_t> (GCC 11).  Cut's bookkeeping and Expand (src/clustering/image_clustering.cpp:68-128, 159-199,
451-624) with the device's free choices: cluster pairs in ascending (c1, c2) order, equal weights in input order.

Every decision that rounding could flip is recorded with its margin: the distance of each discrete_distribution draw to its
nearest cumulative boundary, and the gap between the nearest and the second-nearest centre of each Lloyd assignment."""
import math

import numpy as np

MASK64 = (1 << 64) - 1


class MT19937_64:
    """std::mt19937_64 (the 64-bit Mersenne twister of C++11 [rand.predef]); default_seed 5489."""
    N, M = 312, 156
    MATRIX_A = 0xB5026F5AA96619E9
    UPPER, LOWER = 0xFFFFFFFF80000000, 0x7FFFFFFF

    def __init__(self, seed=5489):
        mt = [0] * self.N
        mt[0] = seed & MASK64
        for i in range(1, self.N):
            mt[i] = (6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & MASK64
        self.mt = np.array(mt, np.uint64)
        self.idx = self.N

    def _twist(self):
        mt = self.mt
        n, m = self.N, self.M
        up, lo, A = np.uint64(self.UPPER), np.uint64(self.LOWER), np.uint64(self.MATRIX_A)
        one = np.uint64(1)
        for lo_i, hi_i in ((0, n - m), (n - m, n - 1)):  # the reference recurrence, in two vectorisable halves
            i = np.arange(lo_i, hi_i)
            # the second half reads mt[i + m - n], written by the first half: sequential order is kept by the split
            y = (mt[i] & up) | (mt[i + 1] & lo)
            mt[i] = mt[(i + m) % n] ^ (y >> one) ^ np.where(y & one, A, np.uint64(0))
        y = (mt[n - 1] & up) | (mt[0] & lo)
        mt[n - 1] = mt[m - 1] ^ (y >> one) ^ (A if int(y) & 1 else np.uint64(0))
        self.idx = 0

    def __call__(self):
        if self.idx >= self.N:
            self._twist()
        y = int(self.mt[self.idx])
        self.idx += 1
        y ^= (y >> 29) & 0x5555555555555555
        y ^= (y << 17) & 0x71D67FFFEDA60000
        y ^= (y << 37) & 0xFFF7EEE000000000
        y ^= y >> 43
        return y & MASK64


def uniform_int(rng, a, b):
    """std::uniform_int_distribution<size_t>(a, b)(mt19937_64): libstdc++'s 128-bit multiply-shift (Lemire) downscaling."""
    urange = b - a
    if urange == MASK64:
        return rng()
    erange = urange + 1
    product = rng() * erange
    low = product & MASK64
    if low < erange:
        threshold = ((1 << 64) - erange) % erange
        while low < threshold:
            product = rng() * erange
            low = product & MASK64
    return a + (product >> 64)


def generate_canonical(rng):
    """std::generate_canonical<double, 53>(mt19937_64): one word / 2^64 (the word rounded to double), below 1."""
    r = float(rng()) / 18446744073709551616.0
    return r if r < 1.0 else math.nextafter(1.0, 0.0)


def discrete(rng, weights):
    """std::discrete_distribution<size_t>(weights)(rng): (index, margin).  libstdc++ normalises by the sequential sum,
    accumulates the partial sums, sets the last to 1 and takes lower_bound of one canonical draw.  margin: the distance of
    the draw to its nearest cumulative boundary (inf when there is no boundary)."""
    w = np.asarray(weights, np.float64)
    if len(w) < 2:
        return 0, math.inf
    total = 0.0
    for x in w.tolist():  # std::accumulate order
        total += x
    cp = np.cumsum(w / total)  # sequential partial sums
    cp[-1] = 1.0
    p = generate_canonical(rng)
    i = int(np.searchsorted(cp, p, side="left"))
    lo = cp[i - 1] if i > 0 else -math.inf
    return i, float(min(cp[i] - p if i < len(cp) - 1 else math.inf, p - lo))


# ---------------------------------------------------------------- graph preparation (the library's input rules)
def prepare(pairs, weights, use=None):
    """Unique used edges (the first occurrence of an unordered pair wins), images by ascending id.  Returns (ids, edges) with
    edges [E, 4] = (vertex of image_id1, vertex of image_id2, weight, input index) in input order."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    w = np.asarray(weights, np.int64).reshape(-1)
    sel = np.ones(len(p), bool) if use is None else np.asarray(use, bool)
    idx = np.nonzero(sel)[0]
    ids = np.unique(p[idx].reshape(-1))
    vi = np.searchsorted(ids, p[idx, 0])
    vj = np.searchsorted(ids, p[idx, 1])
    key = np.minimum(vi, vj) * (len(ids) + 1) + np.maximum(vi, vj)
    _, first = np.unique(key, return_index=True)
    first = np.sort(first)
    edges = np.stack([vi[first], vj[first], w[idx[first]], idx[first]], axis=1)
    return ids, edges


def laplacian(N, edges):
    """Dense L = D_cnt - S (spectral_cluster.cpp:73-82, 150-176: degrees count edges)."""
    L = np.zeros((N, N))
    i, j, w = edges[:, 0], edges[:, 1], edges[:, 2].astype(np.float64)
    np.add.at(L, (i, j), -w)
    np.add.at(L, (j, i), -w)
    np.add.at(L, (i, i), 1.0)
    np.add.at(L, (j, j), 1.0)
    return L


def _sq_dists(X, C):
    out = np.empty((len(X), len(C)))
    for s in range(0, len(X), 512):
        d = X[s:s + 512, None, :] - C[None, :, :]
        out[s:s + 512] = (d * d).sum(-1)
    return out


def kmeans(X, k, max_iterations=0):
    """KMeans (kmeans.h:158-235, KMEANS_INIT_PP) on the rows of X: (assignment, Lloyd iterations, draw margins, Lloyd margins).
    Lloyd margins: per iteration, the gap between the nearest and the second-nearest non-NaN centre of every point."""
    N = len(X)
    rng = MT19937_64()
    centers = [X[uniform_int(rng, 0, N - 1)]]
    dists = np.full(N, np.finfo(np.float64).max)
    draw_margins = []
    for _ in range(1, k):
        d = _sq_dists(X, np.array(centers[-1:]))[:, 0]
        dists = np.where(d < dists, d, dists)
        i, mg = discrete(rng, dists)
        draw_margins.append(mg)
        centers.append(X[i])
    C = np.array(centers)
    assign = np.full(N, k, np.int64)
    lloyd_margins = []
    empty = []
    it = 0
    while True:
        D = _sq_dists(X, C)
        D = np.where(np.isnan(D), np.inf, D)
        new = np.argmin(D, axis=1)  # the first minimum: NearestCenterID's strict <
        part = np.partition(D, 1, axis=1)[:, :2] if k > 1 else np.concatenate([D, np.full((N, 1), np.inf)], axis=1)
        lloyd_margins.append(part[:, 1] - part[:, 0])
        changed = bool((new != assign).any())
        assign = new
        C = np.full((k, X.shape[1]), np.nan)
        for c in range(k):
            mem = assign == c
            if mem.any():
                C[c] = X[mem].sum(0) / mem.sum()
            else:
                empty.append((it, c))  # ComputeCenterOfMass divides 0 / 0: the centre is NaN from here on
        it += 1
        if not changed or (max_iterations and it >= max_iterations):
            break
    return assign, it, np.array(draw_margins), np.concatenate(lloyd_margins) if lloyd_margins else np.zeros(0), empty


SPARSE_ABOVE = 2500  # images above which spectral() leaves the dense eigh (about 10 s there) for the sparse path


def sparse_laplacian(N, edges):
    """L = D_cnt - S as scipy.sparse CSR (the same matrix as laplacian())."""
    import scipy.sparse as sp
    i, j, w = edges[:, 0], edges[:, 1], edges[:, 2].astype(np.float64)
    one = np.ones(len(i))
    rows = np.concatenate([i, j, i, j])
    cols = np.concatenate([j, i, i, j])
    return sp.coo_matrix((np.concatenate([-w, -w, one, one]), (rows, cols)), shape=(N, N)).tocsr()


def spectral_sparse(N, edges, k, extra=1):
    """The k + extra algebraically smallest eigenpairs of L, ascending: Lanczos on L itself (scipy eigsh, ARPACK, which =
    "SA", run to machine precision from a fixed start vector), then one Rayleigh-Ritz step on the orthonormalised vectors.
    No shift-invert: L is indefinite, the wanted end of its spectrum is an extreme one, and the factorisation of a shifted
    L fills in badly on graphs that expand."""
    import scipy.sparse.linalg as spla
    L = sparse_laplacian(N, edges)
    nev = min(k + extra, N - 1)
    _, V = spla.eigsh(L, k=nev, which="SA", tol=0, ncv=min(N, max(3 * nev, 40)), v0=np.ones(N) / math.sqrt(N))
    Q, _ = np.linalg.qr(V)
    H = Q.T @ (L @ Q)
    t, Z = np.linalg.eigh(0.5 * (H + H.T))
    return t, Q @ Z


def spectral(N, edges, k, sparse=None):
    """(eigenvalues, eigenvectors) of L ascending: all N of them by numpy.linalg.eigh, or (sparse; the default above
    SPARSE_ABOVE images) the first k + 1 by spectral_sparse."""
    if sparse is None:
        sparse = N > SPARSE_ABOVE
    if sparse:
        return spectral_sparse(N, edges, k)
    return np.linalg.eigh(laplacian(N, edges))


# ---------------------------------------------------------------- Cut + Expand
def cut_expand(N, edges, labels, n_clusters, n_pairs, image_overlap=50, completeness_ratio=0.5, expand=True):
    """Cut's grouping and Expand's AddLostEdgesBetweenClusters over vertex labels.  Returns (members: list of sets of
    vertices, edge_cluster [n_pairs], lost, readded, edges per cluster)."""
    members = [set() for _ in range(n_clusters)]
    for v in range(N):
        members[labels[v]].add(v)
    n_edges = [0] * n_clusters
    edge_cluster = np.full(n_pairs, -1, np.int32)
    lost = {}
    for i, j, w, orig in edges.tolist():
        c1, c2 = labels[i], labels[j]
        if c1 == c2:
            edge_cluster[orig] = c1
            n_edges[c1] += 1
        else:
            edge_cluster[orig] = -2
            lost.setdefault((min(c1, c2), max(c1, c2)), []).append((i, j, w, orig))
    n_lost = sum(len(v) for v in lost.values())
    sticky = [False] * n_clusters
    cr = np.float32(completeness_ratio)

    def satisfied(c):  # IsSatisfyCompletenessRatio: float32 ratio, sticky
        if sticky[c]:
            return True
        rep = sum(len(members[c] & members[j]) for j in range(n_clusters) if j != c)
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.float32(rep) / np.float32(len(members[c]))
        if ratio <= cr:
            return False
        sticky[c] = True
        return True

    readded = 0
    if expand and n_clusters > 1:
        for (c1, c2) in sorted(lost):
            if len(members[c1] & members[c2]) > image_overlap:
                continue
            if satisfied(c1) and satisfied(c2):
                continue
            le = sorted(lost[(c1, c2)], key=lambda e: -e[2])  # stable: equal weights in input order
            for src, dst, w, orig in le:
                a1 = dst if src in members[c1] else src
                a2 = dst if src in members[c2] else src
                c, a = (c2, a2) if len(members[c1]) > len(members[c2]) else (c1, a1)
                if not satisfied(c) and a not in members[c]:
                    members[c].add(a)
                    n_edges[c] += 1
                    edge_cluster[orig] = c
                    readded += 1
                if satisfied(c1) and satisfied(c2):
                    break
    return members, edge_cluster, n_lost, readded, n_edges


def cluster(pairs, weights, use=None, labels_in=None, num_images_ub=100, image_overlap=50, completeness_ratio=0.5, expand=True,
            max_kmeans_iterations=0, sparse=None):
    """dsm_view_graph_cluster restated.  Returns a dict with image_ids, labels, edge_cluster, clusters (sorted image ids per
    inter cluster), report-like counts, and for SPECTRAL the eigenvalues / eigenvectors and the decision margins."""
    n_pairs = len(np.asarray(pairs).reshape(-1, 2))
    ids, edges = prepare(pairs, weights, use)
    N = len(ids)
    k = max(1, N // num_images_ub)
    out = {"image_ids": ids, "k": k, "eigenvalues": None, "subspace": None, "draw_margins": np.zeros(0),
           "lloyd_margins": np.zeros(0), "kmeans_iterations": 0, "empty_centres": []}
    if labels_in is not None:
        labels = np.asarray(labels_in, np.int64)
        n_clusters = max(k, int(labels.max()) + 1 if N else 0)
    elif k > 1:
        evals, evecs = spectral(N, edges, k, sparse)
        labels, it, dm, lm, empty = kmeans(evecs[:, :k], k, max_kmeans_iterations)
        out.update(eigenvalues=evals, subspace=evecs[:, :k], draw_margins=dm, lloyd_margins=lm, kmeans_iterations=it,
                   empty_centres=empty)
        n_clusters = k
    else:
        labels = np.zeros(N, np.int64)
        n_clusters = k
    members, ec, n_lost, readded, n_edges = cut_expand(N, edges, labels.tolist(), n_clusters, n_pairs, image_overlap,
                                                       completeness_ratio, expand)
    out.update(labels=np.asarray(labels, np.int64), edge_cluster=ec, clusters=[ids[sorted(m)] for m in members],
               num_lost_edges=n_lost, num_readded_edges=readded, num_edges=len(edges),
               clustered_images_num=sum(len(m) for m in members), clustered_edges_num=sum(n_edges))
    return out


def min_margin(res):
    """The smallest recorded margin of a SPECTRAL run (inf when there was no decision)."""
    m = np.concatenate([np.asarray(res["draw_margins"], np.float64), np.asarray(res["lloyd_margins"], np.float64)])
    m = m[np.isfinite(m)]
    return float(m.min()) if len(m) else math.inf


def principal_sine(A, B):
    """The sine of the largest principal angle between the column spaces of A and B (orthonormal columns)."""
    return float(np.linalg.norm(A - B @ (B.T @ A), 2))  # ||(I - B B^T) A||_2, accurate for small angles
