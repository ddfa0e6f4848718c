"""numpy restatement of the reference's vocabulary training, in the reference's order of operations:

  VisualIndex::Quantize                      src/retrieval/visual_index.h:623-665
    flann::hierarchicalClustering            lib/FLANN/flann.hpp:424-432
    KMeansIndex::buildIndexImpl              lib/FLANN/algorithms/kmeans_index.h:329-345
    KMeansIndex::computeNodeStatistics       :496-530
    KMeansIndex::computeClustering           :544-713
    KMeansppCenterChooser::operator()        lib/FLANN/algorithms/center_chooser.h:224-290
    L2<uint8_t>::operator()                  lib/FLANN/algorithms/dist.h:149-177
    KMeansIndex::getMinVarianceClusters      kmeans_index.h:928-969
  InvertedIndex::ComputeHammingEmbedding     src/retrieval/inverted_index.h:184-217, inverted_file.h:275-291
    Median                                   src/util/math.h:211-229

Every float32 / float64 operation is element-wise numpy in the type the C++ expression has, sums run in the order the loops run.
tests/test_vocabulary_build_cpu.py and tests/test_vocabulary_build_edges_cpu.py pin this file to the reference's own binary; the
device is compared with it."""
import ctypes
import sys

import numpy as np

F32, F64 = np.float32, np.float64
RAND_MAX = 2147483647
_libc = None


def libc():
    global _libc
    if _libc is None:
        _libc = ctypes.CDLL(None)
        _libc.rand.restype = ctypes.c_int
        _libc.srand.argtypes = [ctypes.c_uint]
    return _libc


def libc_rand():
    return libc().rand()


def srand(seed):
    libc().srand(seed)


class Replay:
    """A recorded stream of draws, handed out again in order."""

    def __init__(self, draws):
        self.draws, self.pos = list(draws), 0

    def __call__(self):
        v = self.draws[self.pos]
        self.pos += 1
        return v


class Recorder:
    def __init__(self, rand=libc_rand):
        self.rand, self.draws = rand, []

    def __call__(self):
        v = self.rand()
        self.draws.append(v)
        return v


def l2_groups(diff):
    """dist.h:152-176 for float32 differences [..., 128]: result += d0*d0 + d1*d1 + d2*d2 + d3*d3, four at a time."""
    sq = diff * diff
    g = ((sq[..., 0::4] + sq[..., 1::4]) + sq[..., 2::4]) + sq[..., 3::4]
    result = np.zeros(diff.shape[:-1], F32)
    for k in range(g.shape[-1]):
        result = result + g[..., k]
    return result


def dist_u8_u8(a, b):
    """L2 of uint8 against uint8: (ResultType)(int - int); every partial sum is an integer below 2^24."""
    return l2_groups((a.astype(np.int32) - b.astype(np.int32)).astype(F32))


def dist_u8_f64(points, centres):
    """L2 of uint8 points [m,128] against double centres [b,128]: (float)(double(u8) - centre) -> [m, b]."""
    out = np.empty((len(points), len(centres)), F32)
    step = max(1, (1 << 22) // max(1, 128 * len(centres)))
    for s in range(0, len(points), step):
        p = points[s:s + step].astype(F64)
        out[s:s + step] = l2_groups((p[:, None, :] - centres[None, :, :]).astype(F32))
    return out


def dist_f32_u8(centre, points):
    """L2 of a float centre against uint8 points: float - float(u8), in float."""
    return l2_groups(centre.astype(F32)[None, :] - points.astype(F32))


def rand_int(high, rand):
    return int(F64(high) * (F64(rand()) / (F64(RAND_MAX) + F64(1.0))))


def rand_double(high, rand):
    return F64(0.0) + (F64(high) - F64(0.0)) * (F64(rand()) / (F64(RAND_MAX) + F64(1.0)))


def select_walk(rand_val, closest):
    """center_chooser.h:258-262 as written: the subtractive walk."""
    n = len(closest)
    rv = F64(rand_val)
    index = 0
    while index < n - 1:
        c = F64(closest[index])
        if rv <= c:
            break
        rv = rv - c
        index += 1
    return index


def select_prefix(rand_val, closest):
    """The same choice from an inclusive integer prefix sum: the first index < n - 1 whose prefix is >= rand_val, else n - 1."""
    n = len(closest)
    prefix = np.cumsum(np.asarray(closest, np.int64))
    hit = np.nonzero(prefix[:n - 1].astype(F64) >= F64(rand_val))[0]
    return int(hit[0]) if len(hit) else n - 1


def kmeanspp(points, k, rand):
    """center_chooser.h:224-290 (numLocalTries = 1) over the node's points in their current order; positions of the centres."""
    n = len(points)
    centres = np.zeros(k, np.int64)
    index = rand_int(n, rand)
    centres[0] = index
    closest = dist_u8_u8(points, points[index][None, :]).astype(np.int64)
    current_pot = F64(closest.sum())
    for c in range(1, k):
        index = select_prefix(rand_double(current_pot, rand), closest)
        closest = np.minimum(dist_u8_u8(points, points[index][None, :]).astype(np.int64), closest)
        current_pot = F64(closest.sum())
        centres[c] = index
    return centres


def swap_partition(order, belongs, branching):
    """kmeans_index.h:690-710 without the arithmetic: the order the swaps leave, and [start, end) of every child."""
    order, belongs = order.copy(), belongs.copy()
    n = len(order)
    end = 0
    ranges = []
    for c in range(branching):
        start = end
        for i in np.nonzero(belongs[start:] == c)[0] + start:
            # positions before i that held c were swapped down to `end` already; i itself still holds c
            assert belongs[i] == c
            order[i], order[end] = order[end], order[i]
            belongs[i], belongs[end] = belongs[end], belongs[i]
            end += 1
        ranges.append((start, end))
    assert end == n
    return order, ranges


def seq_sum_f32(values):
    """variance += dist, one float at a time."""
    return F32(0.0) if len(values) == 0 else np.cumsum(np.asarray(values, F32), dtype=F32)[-1]


class Node:
    __slots__ = ("parent", "pivot", "radius", "variance", "size", "childs", "index")


def cluster_node(desc, indices, off, m, branching, iterations, rand, node, nodes, stats=None):
    """computeClustering (kmeans_index.h:544-713) of indices[off:off + m]; appends the subtree to nodes in depth-first order.
    stats: a list that receives one record per clustered node (what the tests assert their cases reach); it changes no result."""
    node.size = m
    node.childs = []
    if m < branching:
        return
    idx = indices[off:off + m]
    pts = desc[idx]
    b = branching
    dcenters = pts[kmeanspp(pts, b, rand)].astype(F64)
    with np.errstate(all="ignore"):
        d = dist_u8_f64(pts, dcenters)
        belongs, sq = nan_argmin(d)
        radiuses = np.zeros(b, F32)
        np.maximum.at(radiuses, belongs[~np.isnan(sq)], sq[~np.isnan(sq)])
        count = np.bincount(belongs, minlength=b).astype(np.int64)
        converged, iteration, repairs = False, 0, 0
        while not converged and iteration < iterations:
            converged = True
            iteration += 1
            sums = np.zeros((b, 128), np.int64)
            np.add.at(sums, belongs, pts.astype(np.int64))
            dcenters = sums.astype(F64) * (F64(1.0) / count.astype(F64))[:, None]
            d = dist_u8_f64(pts, dcenters)
            new, sq = nan_argmin(d)
            radiuses = np.zeros(b, F32)
            np.maximum.at(radiuses, new[~np.isnan(sq)], sq[~np.isnan(sq)])
            if (new != belongs).any():
                converged = False
            belongs = new
            count = np.bincount(belongs, minlength=b).astype(np.int64)
            for i in range(b):
                if count[i] == 0:
                    j = (i + 1) % b
                    while count[j] <= 1:
                        j = (j + 1) % b
                    k = int(np.nonzero(belongs == j)[0][0])
                    belongs[k] = i
                    count[j] -= 1
                    count[i] += 1
                    converged = False
                    repairs += 1
        centers = dcenters.astype(F32)
        if stats is not None:
            stats.append({"node": node.index, "size": m, "branching": b, "iterations": iteration, "converged": converged,
                          "repairs": repairs, "nan_centres": int(np.isnan(centers).any(axis=1).sum())})
        dist_var = l2_groups(centers[belongs] - pts.astype(F32))
        order, ranges = swap_partition(np.arange(m), belongs, b)
        indices[off:off + m] = idx[order]
        dist_var = dist_var[order]
        if any(end - start == m for start, end in ranges):
            # without iterations no repair runs: identical points stay in one child, which is clustered into the same
            # children again -- the reference recurses until its stack is gone; the device refuses
            raise ValueError("the clustering does not end")
        for c in range(b):
            start, end = ranges[c]
            child = Node()
            child.parent = node.index
            child.index = len(nodes)
            child.radius = radiuses[c]
            child.pivot = centers[c]
            child.variance = seq_sum_f32(dist_var[start:end]) / F32(count[c])
            nodes.append(child)
            node.childs.append(child)
            cluster_node(desc, indices, off + start, end - start, b, iterations, rand, child, nodes, stats)


def nan_argmin(d):
    """kmeans_index.h:588-596: sq_dist = d[0]; for j >= 1: if (sq_dist > d[j]) take j.  A comparison with a NaN is false: a NaN
    candidate never wins, a NaN at j = 0 is never replaced."""
    m, b = d.shape
    if not np.isnan(d).any():
        best = np.argmin(d, axis=1)
        return best, d[np.arange(m), best]
    best = np.zeros(m, np.int64)
    sq = d[:, 0].copy()
    for j in range(1, b):
        take = sq > d[:, j]
        best[take] = j
        sq[take] = d[take, j]
    return best, sq


def build_tree(desc, branching, iterations, rand=libc_rand, stats=None):
    """KMeansIndex::buildIndexImpl: (nodes in depth-first order, the final indices permutation).  stats: see cluster_node."""
    sys.setrecursionlimit(max(sys.getrecursionlimit(), 20000))
    desc = np.ascontiguousarray(desc, np.uint8)
    n = len(desc)
    if iterations < 0:
        iterations = 2 ** 31 - 1
    indices = np.arange(n, dtype=np.int64)
    root = Node()
    root.parent, root.index = -1, 0
    with np.errstate(all="ignore"):
        # computeNodeStatistics: the mean is a float chain per dimension
        mean = np.cumsum(desc.astype(F32), axis=0, dtype=F32)[-1]
        mean = mean * (F32(1.0) / F32(n))
        dist = dist_f32_u8(mean, desc)
        root.radius = F32(max(F32(0.0), dist.max()))
        root.variance = seq_sum_f32(dist) / F32(n)
        root.pivot = mean
        nodes = [root]
        cluster_node(desc, indices, 0, n, branching, iterations, rand, root, nodes, stats)
    return nodes, indices


def min_variance_clusters(nodes, branching, clusters_length):
    """getMinVarianceClusters (kmeans_index.h:928-969) in float, the break included."""
    with np.errstate(all="ignore"):
        clusters = [nodes[0]]
        mean_variance = F32(nodes[0].variance * F32(nodes[0].size))
        while len(clusters) < clusters_length:
            min_variance = np.finfo(F32).max
            split = -1
            for i, c in enumerate(clusters):
                if c.childs:
                    variance = F32(mean_variance - F32(c.variance * F32(c.size)))
                    for ch in c.childs:
                        variance = F32(variance + F32(ch.variance * F32(ch.size)))
                    if variance < min_variance:
                        min_variance = variance
                        split = i
            if split == -1:
                break
            if branching + len(clusters) - 1 > clusters_length:
                break
            mean_variance = min_variance
            to_split = clusters[split]
            clusters[split] = to_split.childs[0]
            clusters += to_split.childs[1:]
    return clusters


def round_half_away(x):
    """std::round of non-negative floats, cast to uint8."""
    return np.floor(x.astype(F64) + 0.5).astype(np.uint8)


def quantize(desc, num_visual_words, branching, iterations, rand=libc_rand, stats=None):
    """VisualIndex::Quantize: (words [count][128] uint8, float centres, nodes, indices).  stats: see cluster_node."""
    nodes, indices = build_tree(desc, branching, iterations, rand, stats)
    clusters = min_variance_clusters(nodes, branching, num_visual_words)
    centres = np.stack([c.pivot for c in clusters]).astype(F32)
    return round_half_away(centres), centres, nodes, indices


def same_floats(a_bits, b_bits):
    """Equal float bits; a NaN (the centre of a cluster the last iteration emptied, 0 * inf) equals a NaN: its sign and payload
    are the processor's, not the algorithm's."""
    a, b = a_bits.view(np.float32), b_bits.view(np.float32)
    return a.shape == b.shape and bool(((a_bits == b_bits) | (np.isnan(a) & np.isnan(b))).all())


def tree_arrays(nodes):
    """What dsm_get_vocabulary_tree returns: parent, first child, size, variance bits, radius bits, pivots."""
    k = len(nodes)
    parent = np.array([nd.parent for nd in nodes], np.int32)
    first = np.array([nd.childs[0].index if nd.childs else -1 for nd in nodes], np.int32)
    size = np.array([nd.size for nd in nodes], np.int32)
    variance = np.array([nd.variance for nd in nodes], F32).view(np.uint32)
    radius = np.array([nd.radius for nd in nodes], F32).view(np.uint32)
    pivots = np.stack([nd.pivot for nd in nodes]).astype(F32).view(np.uint32).reshape(k, 128)
    return parent, first, size, variance, radius, pivots


# ---------------------------------------------------------------------------------------------------- Hamming embedding
def median_f32(elems):
    """Median (util/math.h:211-229) of floats, stored to a float threshold."""
    s = np.sort(np.asarray(elems, F32))
    mid = len(s) // 2
    if len(s) % 2 == 0:
        with np.errstate(over="ignore"):
            return F32(F64(F32(s[mid] + s[mid - 1])) / F64(2.0))
    return F32(s[mid])


def project(desc, projection):
    """projection [64][128] times float(descriptor), each sum left to right in float (k_vocab_signature's order)."""
    p = np.ascontiguousarray(projection, F32)
    d = desc.astype(F32)
    s = np.zeros((len(desc), 64), F32)
    for j in range(128):
        s = s + p[None, :, j] * d[:, j:j + 1]
    return s


def nearest_words(desc, words):
    """The exact nearest word, ties to the lower id (what dsm_retrieval_index assigns)."""
    w = words.astype(np.int64)
    out = np.empty(len(desc), np.int32)
    for s in range(0, len(desc), 256):
        d = desc[s:s + 256].astype(np.int64)
        dist = ((d[:, None, :] - w[None, :, :]) ** 2).sum(axis=2)
        out[s:s + 256] = np.argmin(dist, axis=1)
    return out


def train_embedding(desc, words, projection, word_ids=None):
    """InvertedIndex::ComputeHammingEmbedding: (thresholds [num_words][64] float32, has_embedding [num_words] uint8)."""
    desc = np.ascontiguousarray(desc, np.uint8)
    ids = nearest_words(desc, words) if word_ids is None else np.asarray(word_ids, np.int32)
    proj = project(desc, projection)
    thresholds = np.zeros((len(words), 64), F32)
    flags = np.zeros(len(words), np.uint8)
    for w in range(len(words)):
        rows = np.nonzero(ids == w)[0]
        if len(rows) < 5:  # kMinEntries
            continue
        for k in range(64):
            thresholds[w, k] = median_f32(proj[rows, k])
        flags[w] = 1
    return thresholds, flags
