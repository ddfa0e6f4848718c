"""Cluster alignment's restatement (tests/cluster_alignment_ref.py; SfMAligner) on the CPU: the draws against
g++'s std::mt19937 + uniform_int_distribution<int>, PROSAC's index range, recovery of planted Sim3s, and one small case
per ruling."""
import math
import shutil
import subprocess

import numpy as np
import pytest

from tests import cluster_alignment_ref as ref

CPP = r'''
#include <cstdio>
#include <random>
int main() {
  std::mt19937 g(12345u);
  for (int i = 0; i < 2000; ++i) std::printf("%u\n", (unsigned)g());
  const int his[] = {0, 1, 2, 3, 5, 6, 99, 1000, 65535, 199999, 2147483646};
  for (unsigned seed : {0u, 7u, 4294967295u}) {
    std::mt19937 h(seed);
    for (int hi : his) {
      std::uniform_int_distribution<int> d(0, hi);
      for (int i = 0; i < 40; ++i) std::printf("%d\n", d(h));
    }
  }
  return 0;
}
'''


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ (libstdc++) to compile the std:: side")
def test_mt19937_draws_match_std(tmp_path):
    src = tmp_path / "draws.cpp"
    src.write_text(CPP)
    exe = tmp_path / "draws"
    subprocess.check_call(["g++", "-O1", "-std=c++17", str(src), "-o", str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    g = ref.MT19937(12345)
    assert [g() for _ in range(2000)] == out[:2000]
    pos = 2000
    for seed in (0, 7, 4294967295):
        h = ref.MT19937(seed)
        for hi in (0, 1, 2, 3, 5, 6, 99, 1000, 65535, 199999, 2147483646):
            assert [ref.rand_int(h, hi) for _ in range(40)] == out[pos:pos + 40], (seed, hi)
            pos += 40
    assert pos == len(out)


def test_prosac_index_stays_below_n():
    for N in range(6, 2001):
        ns, br = ref.prosac_table(N, 5000)
        assert ns.max() <= N - 1, N
        assert ns.min() >= 4


def test_prosac_schedule_starts_like_the_sampler():
    ns, br = ref.prosac_table(244, 10)
    assert list(ns[:3]) == [4, 5, 6] and not br[0]
    mt = ref.max_iter_table(100, ref.default_options())
    assert mt[100] == 100 and mt[4] == 5000 and mt[90] == 100
    assert mt[50] == max(100, int(math.log(0.01) / (math.log(1 - 0.5 ** 4) - np.finfo(float).eps)))


def check_recovery(res, planted, tol_R, tol_rel_t):
    a = res["anchor"]
    for c in np.flatnonzero(res["in_component"]):
        s, R, t = ref.planted_relative(planted, int(c), a)
        assert abs(res["s"][c] - s) <= 1e-2 * s
        assert np.abs(res["R"][c] - R).max() <= tol_R
        assert np.abs(res["t"][c] - t).max() <= tol_rel_t * (1 + np.abs(t).max())


@pytest.mark.parametrize("seed,k", [(1, 4), (7, 6)])
def test_restatement_recovers_planted_sim3(seed, k):
    clusters, planted = ref.scene(n_images=15 * k, n_clusters=k, seed=seed)
    res = ref.align(clusters)
    assert res["in_component"].all()
    assert res["num_edges"] >= k - 1
    check_recovery(res, planted, 5e-3, 5e-3)
    for p in res["pairs"]:
        for d, (a, b) in enumerate(((p["i"], p["j"]), (p["j"], p["i"]))):
            s, R, t = ref.planted_relative(planted, a, b)
            assert abs(p["s"][d] - s) <= 1e-2 * s and np.abs(p["R"][d] - R).max() < 5e-3


def test_fast_join_equals_find_common_3d_points():
    clusters, _ = ref.scene(n_images=50, n_clusters=5, overlap=12, seed=3)
    corr = ref.join(clusters)
    assert len(corr) >= 4
    for (i, j), (a, b) in corr.items():
        la, lb = ref.join_literal(clusters, i, j)
        assert (la == a).all() and (lb == b).all()


# ---------------------------------------------------------------- rulings, one small case each
def cluster(images, pts, obs, ids=None):
    pts = np.asarray(pts, np.float64).reshape(-1, 3)
    return dict(image_ids=np.asarray(images, np.uint32), point_ids=np.asarray(ids if ids is not None else np.arange(len(pts)), np.uint64),
                xyz=pts, obs=np.asarray(obs, np.uint32).reshape(-1, 3))


def pair_of(n_pts, n_images=2, noise=0.0, seed=0, sim=(2.0, None, (1.0, -2.0, 0.5)), outliers=()):
    """two clusters over n_images common images; point q is seen in image q % n_images with point2D_idx q"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-2, 2, (n_pts, 3))
    s, R, t = sim
    R = ref.random_rotation(rng) if R is None else R
    Y = s * X @ R.T + np.asarray(t) + rng.normal(0, noise, X.shape)
    for q in outliers:
        Y[q] += rng.uniform(-5.0, 5.0, 3)
    obs = [(q % n_images, q, q) for q in range(n_pts)]
    imgs = list(range(n_images))
    return [cluster(imgs, X, obs), cluster(imgs, Y, obs)], (s, R, np.asarray(t))


@pytest.mark.parametrize("n", [0, 1, 2])
def test_n_at_most_two_is_no_edge(n):
    clusters, _ = pair_of(n)
    res = ref.align(clusters)
    (p,) = res["pairs"]
    assert p["num_correspondences"] == n and not p["edge"]
    assert res["anchor"] == 0 and list(res["in_component"]) == [True, False]
    assert list(res["separators"]) == [0, 1]


@pytest.mark.parametrize("n", [3, 4, 5])
def test_n_three_to_five_fits_all(n):
    clusters, (s, R, t) = pair_of(n)
    (p,) = ref.align(clusters)["pairs"]
    assert p["edge"] and p["iterations"] == [0, 0]
    assert abs(p["s"][0] - s) < 1e-9 and np.abs(p["R"][0] - R).max() < 1e-9 and np.abs(p["t"][0] - t).max() < 1e-9
    assert p["msd"][0] < 1e-9 and p["msd"][1] < 1e-9


def test_one_common_image_is_no_pair():
    clusters, _ = pair_of(10, n_images=1)
    res = ref.align(clusters)
    assert res["pairs"] == [] and list(res["separators"]) == [0]


def test_fewer_than_four_inliers_is_no_edge():
    # 8 correspondences drawn independently at random on both sides: no 4 of them share a transform, PROSAC keeps < 4 inliers
    rng = np.random.default_rng(2)
    X = rng.uniform(-2, 2, (8, 3))
    Y = rng.uniform(-50, 50, (8, 3))
    obs = [(q % 2, q, q) for q in range(8)]
    res = ref.align([cluster([0, 1], X, obs), cluster([0, 1], Y, obs)])
    (p,) = res["pairs"]
    assert min(p["inliers"]) < 4 and not p["edge"]
    assert ref.DBL_MAX in p["msd"]


def test_four_or_five_inliers_refit_on_all():
    clusters, (s, R, t) = pair_of(9, outliers=(0, 2, 4, 6))  # 5 of 9 agree
    (p,) = ref.align(clusters, ref.default_options(max_reprojection_error=10.0))["pairs"]
    assert all(4 <= c <= 5 for c in p["inliers"])
    # the refit on all 9 (outliers included) is not the planted transform; msd is the mean over all
    a = np.asarray(clusters[0]["xyz"])
    b = np.asarray(clusters[1]["xyz"])
    s2, R2, t2 = ref.fit_all(a, b, 1.0, np.eye(3), np.zeros(3))
    assert abs(p["s"][0] - s2) < 1e-12 and np.abs(p["R"][0] - R2).max() < 1e-12


def test_nan_prone_pair_is_no_edge():
    # every point of cluster 0 at one place: src_var = 0, Umeyama's c = 0/0, NaN model and msd -> no edge (the reference: NaN edge)
    X = np.ones((4, 3))
    Y = np.random.default_rng(0).uniform(-1, 1, (4, 3))
    obs = [(q % 2, q, q) for q in range(4)]
    res = ref.align([cluster([0, 1], X, obs), cluster([0, 1], Y, obs)])
    (p,) = res["pairs"]
    assert math.isnan(p["msd"][0]) and not p["edge"] and res["num_edges"] == 0


def test_kruskal_float_ties_by_index():
    e = [(np.float32(0.5), 1, 2), (np.float32(0.5), 0, 2), (np.float32(0.5), 0, 1)]
    sims = {(a, b): (1.0, np.eye(3), np.zeros(3)) for a in range(3) for b in range(3)}
    g = ref.graph(3, e, sims)
    assert g["mst"] == [(0, 1), (0, 2)]
    assert g["anchor"] == 0 and list(g["mst_parent"]) == [-1, 0, 0]
    # weights equal as float32 though not as double
    w1, w2 = 0.30000001, 0.30000002
    assert np.float32(w1) == np.float32(w2)
    g = ref.graph(3, [(np.float32(w2), 0, 1), (np.float32(w1), 1, 2), (np.float32(0.4), 0, 2)], sims)
    assert g["mst"] == [(0, 1), (1, 2)]


def test_two_node_anchor_is_the_larger_index():
    sims = {(0, 1): (2.0, np.eye(3), np.array([1.0, 0, 0])), (1, 0): (0.5, np.eye(3), np.array([-0.5, 0, 0]))}
    g = ref.graph(3, [(np.float32(0.1), 0, 1)], sims)
    assert g["anchor"] == 1 and list(g["mst_parent"]) == [1, -1, -1]
    assert g["s"][0] == 2.0 and list(g["t"][0]) == [1.0, 0, 0]
    assert list(g["in_component"]) == [True, True, False]


def test_disconnected_cluster_and_component_ties():
    sims = {(a, b): (1.0, np.eye(3), np.zeros(3)) for a in range(5) for b in range(5)}
    g = ref.graph(5, [(np.float32(0.1), 3, 4), (np.float32(0.1), 1, 2)], sims)  # two components of 2: the one holding 1 wins
    assert list(g["in_component"]) == [False, True, True, False, False] and g["anchor"] == 2
    g = ref.graph(4, [(np.float32(0.2), 0, 1), (np.float32(0.3), 1, 2)], sims)  # a path: the middle is the anchor
    assert g["anchor"] == 1 and list(g["mst_parent"]) == [1, -1, 1, -1] and not g["in_component"][3]


def test_single_cluster_is_identity_at_zero():
    clusters, _ = pair_of(10)
    res = ref.align(clusters[:1])
    assert res["anchor"] == 0 and res["pairs"] == [] and res["in_component"].all()
    assert res["s"][0] == 1.0 and (res["R"][0] == np.eye(3)).all() and (res["t"][0] == 0).all()


def test_path_composition():
    r = ref.random_rotation(np.random.default_rng(5))
    sims = {(0, 1): (2.0, r, np.array([1.0, 2.0, 3.0])), (1, 2): (0.5, r.T, np.array([0.0, 1.0, 0.0])),
            (2, 1): (2.0, r, np.zeros(3)), (1, 0): (0.5, r.T, np.zeros(3))}
    g = ref.graph(3, [(np.float32(0.1), 0, 1), (np.float32(0.2), 1, 2)], sims)
    assert g["anchor"] == 1
    x = np.array([0.3, -0.2, 0.9])
    y = 2.0 * r @ x + np.array([1.0, 2.0, 3.0])
    assert np.allclose(g["s"][0] * g["R"][0] @ x + g["t"][0], y, atol=1e-14)
