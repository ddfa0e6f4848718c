"""View-graph clustering (dsm_view_graph_cluster; ClusteringScenes, src/controllers/distributed_mapper_controller.cpp:633-657),
CPU side: the restatement's libstdc++ random draws against std:: compiled here, planted partitions, the Expand rules on
hand-built cases, labels_in without Expand, the option defaults and the new symbols."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import view_graph_clustering_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def planted(n_blocks, size, seed, p_in=0.3, n_weak=2):
    """n_blocks dense blocks of `size` images (inlier counts 80..200) joined by n_weak weak edges (weight 1) per neighbouring
    block; image ids shuffled so that blocks are not id ranges."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n_blocks * size) * 3 + 7
    pairs, w, truth = [], [], {}
    for b in range(n_blocks):
        blk = ids[b * size:(b + 1) * size]
        for v in blk:
            truth[int(v)] = b
        for i in range(size):
            for j in range(i + 1, size):
                if j == i + 1 or rng.random() < p_in:
                    pairs.append((blk[i], blk[j]))
                    w.append(int(rng.integers(80, 201)))
        nxt = ids[((b + 1) % n_blocks) * size:((b + 1) % n_blocks + 1) * size]
        for _ in range(n_weak):
            pairs.append((blk[rng.integers(size)], nxt[rng.integers(size)]))
            w.append(1)
    return np.array(pairs, np.uint32), np.array(w, np.int32), truth


def same_partition(labels, ids, truth):
    lab = {}
    for v, l in zip(ids.tolist(), labels.tolist()):
        lab.setdefault(truth[v], set()).add(l)
    return all(len(s) == 1 for s in lab.values()) and len({next(iter(s)) for s in lab.values()}) == len(lab)


def planted_sparse(sizes, half, seed, n_weak=2, unit_weights=False):
    """Blocks of the given sizes, each a ring (i, i + 1) plus `half - 1` chords per image, half of them stretched to a random
    multiple of their length so that a block expands; inlier counts 80..200 (or 1 everywhere: the true graph Laplacian),
    neighbouring blocks joined by n_weak edges of weight 1 (0: the blocks are the connected components).  Ids shuffled.
    Cheap at any size: numpy only.  Returns (pairs, weights, truth: id -> block)."""
    rng = np.random.default_rng(seed)
    N = int(sum(sizes))
    ids = rng.permutation(N).astype(np.int64) * 3 + 7
    pairs, w, comp = [], [], np.zeros(N, np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    for b, size in enumerate(sizes):
        blk = ids[start[b]:start[b + 1]]
        comp[start[b]:start[b + 1]] = b
        i = np.repeat(np.arange(size), half)
        d = np.tile(np.arange(1, half + 1), size)
        j = (i + d * (1 + (rng.integers(0, 2, len(i)) * (d > 1)) * rng.integers(1, max(2, size // (2 * half)), len(i)))) % size
        key = np.minimum(i, j) * size + np.maximum(i, j)
        _, f = np.unique(key, return_index=True)
        f = f[i[f] != j[f]]
        pairs.append(np.stack([blk[i[f]], blk[j[f]]], 1))
        w.append(rng.integers(80, 201, len(f)))
        if n_weak and len(sizes) > 1:
            nxt = ids[start[(b + 1) % len(sizes)]:start[(b + 1) % len(sizes) + 1]]
            pairs.append(np.stack([blk[rng.integers(size, size=n_weak)], nxt[rng.integers(len(nxt), size=n_weak)]], 1))
            w.append(np.ones(n_weak, np.int64))
    truth = dict(zip(ids.tolist(), comp.tolist()))
    w = np.concatenate(w).astype(np.int32)
    return np.concatenate(pairs).astype(np.uint32), np.ones_like(w) if unit_weights else w, truth


def twin_blocks(size, half, seed):
    """Two disjoint blocks with the same edges and the same weights (ids 2 v and 2 v + 1): every eigenvalue of L is double."""
    p, w, _ = planted_sparse([size], half, seed, n_weak=0)
    _, inv = np.unique(p, return_inverse=True)
    v = inv.reshape(p.shape).astype(np.uint32)
    return np.concatenate([2 * v, 2 * v + 1]), np.concatenate([w, w])


def components(pairs, use=None):
    """Number of connected components of the used pairs (union-find)."""
    p = np.asarray(pairs, np.int64).reshape(-1, 2)
    if use is not None:
        p = p[np.asarray(use, bool)]
    parent = {int(v): int(v) for v in np.unique(p)}

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in p.tolist():
        parent[find(a)] = find(b)
    return len({find(a) for a in parent})


def clear_share(res, margin=1e-6):
    """(every k-means++ draw is clear, the share of points whose every Lloyd decision is clear) of a restatement result."""
    n = len(res["labels"])
    clear = (res["lloyd_margins"].reshape(-1, n) >= margin).all(axis=0)
    return bool((res["draw_margins"] >= margin).all()), float(clear.mean())


# The fixtures of tests/test_view_graph_clustering_edges_gpu.py: name -> (graph builder, num_images_ub).  The seeds were
# chosen on the restatement alone (the properties below), never on what the device returns.
SCALE = {
    "10000_k100": (lambda: planted(100, 100, 50), 100),                            # 40 row chunks, 12.5 Gram tiles per side
    "16593_cap64": (lambda: planted_sparse([4148, 4148, 4148, 4149], 6, 31), 4000),  # 64 chunks asked, 62 run, the last 1 row
    "1601_one_row_tile": (lambda: planted_sparse([400, 400, 400, 401], 5, 31), 400),  # 16 * 100 + 1
    "257_short_chunk": (lambda: planted_sparse([64, 64, 64, 65], 4, 31), 64),
}
_cache = {}


def scale_case(name):
    """(pairs, weights, num_images_ub, restatement result) of a SCALE fixture, computed once per process."""
    if name not in _cache:
        build, ub = SCALE[name]
        p, w, _ = build()
        _cache[name] = (p, w, ub, ref.cluster(p, w, num_images_ub=ub))
    return _cache[name]


# ---------------------------------------------------------------- libstdc++ draws
CPP = r'''
#include <cstdio>
#include <random>
#include <vector>
int main() {
  std::mt19937_64 g(std::mt19937_64::default_seed);
  for (int i = 0; i < 10000; ++i) std::printf("%llu\n", (unsigned long long)g());
  std::mt19937_64 u(std::mt19937_64::default_seed);
  const size_t hi[] = {0, 1, 2, 6, 9, 99, 999, 9999, 123456789, 18446744073709551614ull};
  for (size_t h : hi)
    for (int i = 0; i < 50; ++i) std::printf("%zu\n", std::uniform_int_distribution<size_t>(0, h)(u));
  std::mt19937_64 d(std::mt19937_64::default_seed);
  std::mt19937_64 wg(42);
  for (int t = 0; t < 40; ++t) {
    std::vector<double> w(1 + t * 7);
    for (size_t i = 0; i < w.size(); ++i) w[i] = (wg() % 3 == 0) ? 0.0 : (double)(wg() >> 11) * 0x1p-53 * (t + 1);
    w[0] += 1e-3;
    std::discrete_distribution<size_t> dd(w.begin(), w.end());
    for (int i = 0; i < 20; ++i) std::printf("%zu\n", dd(d));
  }
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ (libstdc++) to compile the std:: side")
def test_libstdcxx_draws_match_std(tmp_path):
    src = tmp_path / "draws.cpp"
    src.write_text(CPP)
    exe = tmp_path / "draws"
    subprocess.check_call(["g++", "-O1", "-std=c++17", str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    g = ref.MT19937_64()
    words = [g() for _ in range(10000)]
    assert words == out[:10000]
    pos = 10000
    u = ref.MT19937_64()
    for h in (0, 1, 2, 6, 9, 99, 999, 9999, 123456789, 18446744073709551614):
        got = [ref.uniform_int(u, 0, h) for _ in range(50)]
        assert got == out[pos:pos + 50], h
        pos += 50
    d = ref.MT19937_64()
    wg = ref.MT19937_64(42)
    for t in range(40):
        w = []
        for _ in range(1 + t * 7):
            if wg() % 3 == 0:
                w.append(0.0)
            else:
                w.append(float(wg() >> 11) * 2.0 ** -53 * (t + 1))
        w[0] += 1e-3
        got = [ref.discrete(d, w)[0] for _ in range(20)]
        assert got == out[pos:pos + 20], t
        assert all(w[i] > 0 for i in got)  # a zero weight is never drawn
        pos += 20
    assert pos == len(out)


# ---------------------------------------------------------------- planted partitions
@pytest.mark.parametrize("n_blocks,size,seed", [(6, 100, 1), (20, 100, 4)])
def test_restatement_recovers_planted_partition(n_blocks, size, seed):
    pairs, w, truth = planted(n_blocks, size, seed)
    res = ref.cluster(pairs, w, num_images_ub=size)
    assert res["k"] == n_blocks
    assert same_partition(res["labels"], res["image_ids"], truth)
    assert res["num_lost_edges"] == 2 * n_blocks
    assert ref.min_margin(res) > 0.0


def test_k_one_and_below_num_images_ub():
    pairs, w, _ = planted(2, 30, 3)
    for ub in (40, 100):  # 60 images: k = 1, and k = 0 treated as 1
        res = ref.cluster(pairs, w, num_images_ub=ub)
        assert res["k"] == 1 and (res["labels"] == 0).all() and res["eigenvalues"] is None
        assert len(res["clusters"]) == 1 and len(res["clusters"][0]) == 60


# ---------------------------------------------------------------- Expand rules on hand-built cases
def _run(pairs, w, labels, **kw):
    pairs = np.array(pairs, np.uint32)
    ids, _ = ref.prepare(pairs, w)
    lab = [labels[int(i)] for i in ids]
    return ref.cluster(pairs, np.array(w, np.int32), labels_in=lab, num_images_ub=1000, **kw)


def test_expand_adds_heaviest_lost_edge_to_smaller_cluster():
    # cluster 0 = {1, 2, 3}, cluster 1 = {4, 5}; lost edges (3, 4) w 10 and (2, 5) w 30
    pairs = [(1, 2), (2, 3), (4, 5), (3, 4), (2, 5)]
    w = [50, 50, 50, 10, 30]
    lab = {1: 0, 2: 0, 3: 0, 4: 1, 5: 1}
    res = _run(pairs, w, lab, image_overlap=3)
    # heaviest first: (2, 5) goes to the smaller cluster 1 (adds image 2); then cluster 1 = {2, 4, 5} has ratio 1/3 and
    # cluster 0's ratio 1/3: (3, 4): sizes 3 vs 3, the tie goes to cluster 1 (selected_image = 1 means cluster1 = c1 = 0)
    assert [c.tolist() for c in res["clusters"]] == [[1, 2, 3, 4], [2, 4, 5]]
    assert res["edge_cluster"].tolist() == [0, 0, 1, 0, 1]
    assert res["num_lost_edges"] == 2 and res["num_readded_edges"] == 2


def test_expand_overlap_cutoff():
    # cluster 0 = images 1..10, clusters 1 = 11..14 and 2 = 21..24.  Pairs (0, 1) and (0, 2) add images 1..4 to both small
    # clusters, so clusters 1 and 2 share 4 images when their own pair (11, 21) comes: above an overlap of 3 it is skipped.
    pairs = [(i, i + 1) for i in range(1, 10)] + [(11, 12), (12, 13), (13, 14), (21, 22), (22, 23), (23, 24)]
    w = [90] * len(pairs)
    lost = [(i, 10 + i) for i in range(1, 5)] + [(i, 20 + i) for i in range(1, 5)] + [(11, 21)]
    pairs += lost
    w += [50 - i for i in range(len(lost))]
    lab = {v: 0 for v in range(1, 11)}
    lab.update({v: 1 for v in range(11, 15)})
    lab.update({v: 2 for v in range(21, 25)})
    cut = _run(pairs, w, lab, image_overlap=3, completeness_ratio=1.0)
    assert [c.tolist() for c in cut["clusters"]] == [list(range(1, 11)), [1, 2, 3, 4, 11, 12, 13, 14], [1, 2, 3, 4, 21, 22, 23, 24]]
    assert cut["edge_cluster"][-1] == -2 and cut["num_readded_edges"] == 8
    # an overlap of 4 lets the pair through: the sizes tie (8, 8), so cluster 1 takes image 21
    free = _run(pairs, w, lab, image_overlap=4, completeness_ratio=1.0)
    assert free["clusters"][1].tolist() == [1, 2, 3, 4, 11, 12, 13, 14, 21]
    assert free["edge_cluster"][-1] == 1 and free["num_readded_edges"] == 9


def test_expand_sticky_completeness_ratio():
    # cluster 0 = {1, 2}, cluster 1 = {3, 4}: after one re-added image cluster 0 = {1, 2, 3}: repeated 1, ratio 1/3 > 0.25,
    # so it is satisfied and stays so; cluster 1 gets nothing because cluster 0 is the smaller one only on a tie
    pairs = [(1, 2), (3, 4), (1, 3), (2, 4)]
    w = [9, 9, 5, 4]
    lab = {1: 0, 2: 0, 3: 1, 4: 1}
    res = _run(pairs, w, lab, completeness_ratio=0.25)
    # first lost edge (1, 3) w 5: sizes 2 == 2 -> cluster 0 adds 3.  c0: 1/3 > 0.25 satisfied; c1 = {3, 4}: 1/2 > 0.25
    # satisfied -> return
    assert [c.tolist() for c in res["clusters"]] == [[1, 2, 3], [3, 4]]
    assert res["edge_cluster"].tolist() == [0, 1, 0, -2]
    loose = _run(pairs, w, lab, completeness_ratio=0.5)
    # ratio 1/3 <= 0.5 and 1/2 <= 0.5: not satisfied; (2, 4): sizes 3 > 2 -> cluster 1 adds 2 (ratio 2/3 > 0.5 afterwards)
    assert [c.tolist() for c in loose["clusters"]] == [[1, 2, 3], [2, 3, 4]]
    assert loose["edge_cluster"].tolist() == [0, 1, 0, 1]


def test_expand_weight_ties_keep_input_order():
    pairs = [(1, 2), (3, 4), (2, 3), (1, 4)]
    lab = {1: 0, 2: 0, 3: 1, 4: 1}
    a = _run(pairs, [9, 9, 5, 5], lab, completeness_ratio=0.2)
    b = _run([pairs[0], pairs[1], pairs[3], pairs[2]], [9, 9, 5, 5], lab, completeness_ratio=0.2)
    # one edge is added before both clusters are satisfied: the first in input order
    assert a["edge_cluster"].tolist() == [0, 1, 0, -2]
    assert b["edge_cluster"].tolist() == [0, 1, 0, -2]
    assert [c.tolist() for c in a["clusters"]] == [[1, 2, 3], [3, 4]]
    assert [c.tolist() for c in b["clusters"]] == [[1, 2, 4], [3, 4]]


def test_empty_cluster_counts_as_satisfied_and_stays_empty():
    pairs = [(1, 2), (3, 4), (2, 3)]
    lab = {1: 0, 2: 0, 3: 2, 4: 2}  # label 1 unused: an empty cluster
    res = _run(pairs, [9, 9, 5], lab)
    assert len(res["clusters"]) == 3 and len(res["clusters"][1]) == 0
    assert res["num_readded_edges"] == 1


def test_labels_in_without_expand_is_the_cut():
    pairs, w, truth = planted(4, 25, 5)
    ids, edges = ref.prepare(pairs, w)
    rng = np.random.default_rng(0)
    lab = rng.integers(0, 4, len(ids))
    res = ref.cluster(pairs, w, labels_in=lab, num_images_ub=25, expand=False)
    for c in range(4):
        assert res["clusters"][c].tolist() == sorted(ids[lab == c].tolist())
    li, lj = lab[edges[:, 0]], lab[edges[:, 1]]
    exp = np.where(li == lj, li, -2)
    assert res["edge_cluster"][edges[:, 3]].tolist() == exp.tolist()
    assert res["num_readded_edges"] == 0


# ---------------------------------------------------------------- the C-ABI without a device
def test_clustering_symbols_and_defaults():
    """The new entry points exist in both builds; the defaults are ImageClustering::Options' and Spectra's
    (image_clustering.h:126-132, SymEigsSolver.h:583)."""
    import ctypes
    from dagsfm_amd import capi
    for path in (capi.LIB_PATH, capi.CHECK_LIB_PATH):
        L = ctypes.CDLL(path)
        for s in ("dsm_view_graph_cluster", "dsm_default_clustering_options", "dsm_get_clustering_spectrum"):
            assert hasattr(L, s), s
    o = capi.default_clustering_options()
    assert (o.num_images_ub, o.image_overlap, o.completeness_ratio, o.expand) == (100, 50, 0.5, 1)
    assert (o.max_kmeans_iterations, o.max_eigen_iterations, o.eigen_tolerance) == (0, 0, 1e-10)


# ---------------------------------------------------------------- the sparse path and the fixtures of the edge tests
def _existing_fixtures():
    from tests.test_view_graph_clustering_gpu import random_graph, sequence_graph
    return {"planted_6": (planted(6, 100, 1)[:2], 100), "planted_20": (planted(20, 100, 4)[:2], 100),
            "random_1000": (random_graph(1000, 8, 21), 100), "sequence_400": (sequence_graph(400, 4, 22), 100)}


@pytest.mark.parametrize("name", ["planted_6", "planted_20", "random_1000", "sequence_400"])
def test_sparse_spectral_path_reproduces_the_dense_one(name):
    """eigsh against eigh on the fixtures of the device tests: eigenvalues to EV_RTOL, the principal sine within the bound
    the device is held to with both residuals at their backward error (100 eps ||L|| / gap each)."""
    from tests.test_view_graph_clustering_gpu import EV_RTOL
    (pairs, w), ub = _existing_fixtures()[name]
    ids, edges = ref.prepare(pairs, w)
    k = len(ids) // ub
    d, D = ref.spectral(len(ids), edges, k, sparse=False)
    s, S = ref.spectral(len(ids), edges, k, sparse=True)
    assert len(s) == k + 1 and S.shape == (len(ids), k + 1)
    assert np.all(np.abs(s - d[:k + 1]) <= EV_RTOL * np.maximum(np.abs(d[:k + 1]), 1.0))
    gap = d[k] - d[k - 1]
    assert gap > 0
    sine = ref.principal_sine(S[:, :k], D[:, :k])
    assert sine <= 2 * 100 * np.finfo(np.float64).eps * np.abs(d).max() / gap, sine
    a = ref.cluster(pairs, w, num_images_ub=ub, sparse=True)
    b = ref.cluster(pairs, w, num_images_ub=ub, sparse=False)
    clear = (b["lloyd_margins"].reshape(-1, len(ids)) >= 1e-6).all(axis=0)
    assert a["kmeans_iterations"] == b["kmeans_iterations"] and np.array_equal(a["labels"][clear], b["labels"][clear])


@pytest.mark.parametrize("name", sorted(SCALE))
def test_scale_fixtures_are_clear_of_rounding(name):
    """Connected, k as meant, every k-means++ draw clear and at least 90 % of the points clear in every Lloyd decision,
    on the restatement alone."""
    pairs, w, ub, res = scale_case(name)
    n = len(res["image_ids"])
    assert components(pairs) == 1
    assert (n, res["k"]) == {"10000_k100": (10000, 100), "16593_cap64": (16593, 4), "1601_one_row_tile": (1601, 4),
                             "257_short_chunk": (257, 4)}[name]
    draws, share = clear_share(res)
    assert draws and share >= 0.9, (draws, share)
    if name != "10000_k100":
        assert ref.min_margin(res) >= 1e-6 and res["num_lost_edges"] == 8  # the weak links, and nothing else
    # the Gram grid these sizes are for (csrc/view_graph_clustering.hip: CL_MAX_CHUNKS 64, 256 rows, CL_TILE 16)
    n_chunks = min(64, -(-n // 256))
    chunk_rows = -(-(-(-n // n_chunks)) // 16) * 16
    grid = -(-n // chunk_rows)
    last = n - (grid - 1) * chunk_rows
    assert (n_chunks, grid, last) == {"10000_k100": (40, 40, 16), "16593_cap64": (64, 62, 1), "1601_one_row_tile": (7, 7, 161),
                                      "257_short_chunk": (2, 2, 113)}[name]


def test_degenerate_fixtures_have_the_components_they_claim():
    for sizes, half, seed, k in (([100, 100, 100], 5, 81, 3), ([200, 200], 5, 82, 4), ([60] * 5, 4, 83, 3)):
        for unit in (False, True):
            pairs, w, truth = planted_sparse(sizes, half, seed, n_weak=0, unit_weights=unit)
            assert components(pairs) == len(sizes) and len(truth) == sum(sizes)
            lam = np.linalg.eigvalsh(ref.laplacian(len(truth), ref.prepare(pairs, w)[1]))
            if unit:  # the true Laplacian: eigenvalue 0 once per component, nothing below
                assert np.abs(lam[:len(sizes)]).max() < 1e-12 and lam[len(sizes)] > 1e-3
    res = ref.cluster(*planted_sparse([100, 100, 100], 5, 81, n_weak=0)[:2], num_images_ub=100)
    assert res["num_lost_edges"] == 0 and ref.min_margin(res) >= 1e-6
    pairs, w = twin_blocks(150, 5, 85)
    assert components(pairs) == 2
    lam = np.linalg.eigvalsh(ref.laplacian(300, ref.prepare(pairs, w)[1]))
    assert np.abs(lam[0:6:2] - lam[1:6:2]).max() <= 1e-9 and lam[4] - lam[3] > 1.0  # pairs; k = 3 cuts the second


def test_kmeans_cap_fixtures():
    """The uncapped Lloyd counts the device tests rely on, every margin clear; a cap ends the iteration where it says."""
    from tests.test_view_graph_clustering_gpu import random_graph, sequence_graph
    for (pairs, w), ub, natural in ((sequence_graph(600, 3, 51), 50, 14), (random_graph(1000, 8, 61), 100, 17)):
        res = ref.cluster(pairs, w, num_images_ub=ub)
        assert res["kmeans_iterations"] == natural and ref.min_margin(res) >= 1e-6 and res["empty_centres"] == []
        for cap in (1, 7, 8, 9, 16):
            capped = ref.cluster(pairs, w, num_images_ub=ub, max_kmeans_iterations=cap)
            assert capped["kmeans_iterations"] == min(cap, natural)
            assert np.array_equal(capped["lloyd_margins"], res["lloyd_margins"][:len(capped["lloyd_margins"])])


def test_kmeans_records_an_empty_centre():
    """Rows given by hand (no graph): three centres over two distinct rows.  The centre drawn on a duplicate of an earlier
    one never wins a point (strict <), has no member and turns NaN; the restatement records it.  No graph was found whose
    spectral rows do this with clear margins (tens of thousands of seeded small graphs were tried), so the device side of
    this path is still covered only through labels_in."""
    X = np.array([[0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [5.0, 0.0]])
    with np.errstate(invalid="ignore"):  # the last draw's weights are all 0
        assign, it, _, _, empty = ref.kmeans(X, 3)
    assert len(set(assign.tolist())) == 2 and it == 2
    assert empty == [(0, 2), (1, 2)]
