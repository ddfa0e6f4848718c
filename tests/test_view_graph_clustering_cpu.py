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
