"""Cluster alignment on the device (dsm_align_clusters; SfMAligner) against the numpy restatement
(tests/cluster_alignment_ref.py): separators, correspondence counts, edges, MST, anchor, inlier and iteration counts
identical wherever the restatement's margins are >= 1e-9 relative; Sim3s and msd to 1e-12.  Also the planted Sim3s,
byte-identical repeats and shuffles, the large cases and the argument errors."""
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import cluster_alignment_ref as ref
from tests.test_cluster_alignment_cpu import check_recovery, cluster, pair_of

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
RTOL = 1e-12


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def dev_align(ctx, clusters, o=None, seeds=None):
    opts = capi.default_align_options(**(o or {}))
    return ctx.align_clusters(clusters, opts, seeds)


def close(x, y, rtol=RTOL):
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    return bool((np.abs(x - y) <= rtol * np.maximum(np.abs(y), 1.0)).all())


def compare_pair(dp, ep):
    assert (int(dp["i"]), int(dp["j"])) == (ep["i"], ep["j"])
    assert int(dp["num_common_images"]) == ep["num_common_images"]
    assert int(dp["num_correspondences"]) == ep["num_correspondences"]
    if ep["margin"] < MARGIN:
        return False
    assert list(dp["num_inliers"]) == ep["inliers"], (ep["i"], ep["j"])
    assert list(dp["iterations"]) == ep["iterations"], (ep["i"], ep["j"])
    assert bool(dp["edge"]) == ep["edge"]
    for d in (0, 1):
        if ep["num_correspondences"] < 3:
            continue
        if ep["num_correspondences"] > 5:  # PROSAC's own best, before the refit: the replay of the draws itself
            assert close(dp["prosac_cost"][d], ep["prosac_cost"][d]), (ep["i"], ep["j"], d)
            assert close(dp["prosac_s"][d], ep["prosac_s"][d]) and close(dp["prosac_R"][d], np.ravel(ep["prosac_R"][d]))
            assert close(dp["prosac_t"][d], ep["prosac_t"][d])
        assert close(dp["s"][d], ep["s"][d]) and close(dp["R"][d], np.ravel(ep["R"][d])) and close(dp["t"][d], ep["t"][d])
        if ep["msd"][d] == ref.DBL_MAX:
            assert dp["msd"][d] == ref.DBL_MAX
        else:
            assert close(dp["msd"][d], ep["msd"][d])
    return True


def compare(dev, exp, min_clear=1.0):
    assert list(dev["separators"]) == list(exp["separators"])
    assert len(dev["pairs"]) == len(exp["pairs"])
    clear = [compare_pair(dp, ep) for dp, ep in zip(dev["pairs"], exp["pairs"])]
    assert np.mean(clear) >= min_clear, clear
    # the host graph on the device's own weights, as the restatement rules it
    K = len(dev["in_component"])
    edges = [(np.float32(p["weight"]), int(p["i"]), int(p["j"])) for p in dev["pairs"] if p["edge"]]
    sims = {}
    for p in dev["pairs"]:
        if p["edge"]:
            sims[(int(p["i"]), int(p["j"]))] = (float(p["s"][0]), p["R"][0].reshape(3, 3), p["t"][0])
            sims[(int(p["j"]), int(p["i"]))] = (float(p["s"][1]), p["R"][1].reshape(3, 3), p["t"][1])
    g = ref.graph(K, edges, sims)
    assert dev["anchor"] == g["anchor"] and (dev["in_component"] == g["in_component"]).all()
    assert (dev["mst_parent"] == g["mst_parent"]).all()
    assert close(dev["s"], g["s"], 1e-15) and close(dev["R"], g["R"], 1e-15) and close(dev["t"], g["t"], 1e-15)
    if all(clear):
        assert dev["anchor"] == exp["anchor"] and (dev["mst_parent"] == exp["mst_parent"]).all()
        assert (dev["in_component"] == exp["in_component"]).all()
        assert close(dev["s"], exp["s"]) and close(dev["R"], exp["R"], 1e-11) and close(dev["t"], exp["t"], 1e-11)
    rep = dev["report"]
    assert rep.num_pairs == len(exp["pairs"]) and rep.num_edges == exp["num_edges"] or not all(clear)
    assert rep.num_separators == len(exp["separators"])
    return clear


@pytest.mark.parametrize("seed,k", [(1, 4), (2, 4), (7, 6), (11, 8)])
def test_device_matches_restatement_and_planted(ctx, seed, k):
    clusters, planted = ref.scene(n_images=15 * k, n_clusters=k, seed=seed)
    dev = dev_align(ctx, clusters)
    exp = ref.align(clusters)
    compare(dev, exp, min_clear=0.5)
    assert dev["in_component"].all()
    check_recovery(dev, planted, 5e-3, 5e-3)
    assert dev["report"].device_ms > 0 and dev["report"].prosac_iterations == sum(sum(p["iterations"]) for p in exp["pairs"]) \
        or not all(p["margin"] >= MARGIN for p in exp["pairs"])


def test_explicit_seeds_and_user_seed(ctx):
    clusters, _ = ref.scene(n_images=60, n_clusters=4, seed=3)
    K = len(clusters)
    seeds = np.arange(K * K, dtype=np.uint32).reshape(K, K) * 7919 + 3
    compare(dev_align(ctx, clusters, seeds=seeds), ref.align(clusters, seeds=seeds), min_clear=0.5)
    o = ref.default_options(random_seed=99)
    compare(dev_align(ctx, clusters, dict(random_seed=99)), ref.align(clusters, o), min_clear=0.5)
    assert capi.align_seed(1, 2, 1, 99) == ref.align_seed(1, 2, 1, 99)


def scattered_pair(fx):
    """300 correspondences, half of them outliers at scattered indices, noise 0.04 against the 0.1 threshold: which
    inliers PROSAC keeps, how many iterations it runs and its best cost all depend on the draws"""
    out = sorted(np.random.default_rng(fx).choice(300, 150, replace=False))
    return pair_of(300, n_images=4, noise=0.04, seed=fx, outliers=out)[0]


@pytest.mark.parametrize("fx", [3, 4, 5])
def test_prosac_outcome_follows_the_draws(ctx, fx):
    clusters = scattered_pair(fx)
    seen = set()
    for us in (0, 1, 2):
        dev = dev_align(ctx, clusters, dict(random_seed=us))
        exp = ref.align(clusters, ref.default_options(random_seed=us))
        assert compare(dev, exp) == [True]  # margins clear: counts identical, PROSAC's cost and model to 1e-12
        (p,) = dev["pairs"]
        seen.add((int(p["iterations"][0]), int(p["num_inliers"][0]), float(p["prosac_cost"][0])))
        # another stream gives another answer: the device follows this one
        other = ref.align(clusters, ref.default_options(random_seed=us + 100))["pairs"][0]
        assert not close(p["prosac_cost"][0], other["prosac_cost"][0])
    assert len(seen) == 3
    K = 2
    seeds = np.array([[0, 0x9E3779B9], [12345, 0]], np.uint32).reshape(K, K)
    assert compare(dev_align(ctx, clusters, seeds=seeds), ref.align(clusters, seeds=seeds)) == [True]


@pytest.mark.parametrize("iters", [1, 2, 3, 7, 300])
def test_short_prosac_runs_pick_the_same_sample(ctx, iters):
    # with a fixed number of trials the best model is one of the first draws: the first samples take the sampler's
    # "3 of the top n - 1, then n" branch, later ones 4 of the top n
    clusters = scattered_pair(4)
    o = dict(min_iterations=iters, max_iterations=iters)
    dev = dev_align(ctx, clusters, o)
    exp = ref.align(clusters, ref.default_options(**o))
    assert compare(dev, exp) == [True]
    assert list(dev["pairs"][0]["iterations"]) == [iters, iters]


def blob(res):
    return (res["pairs"].tobytes(), res["anchor"], res["in_component"].tobytes(), res["mst_parent"].tobytes(), res["s"].tobytes(),
            res["R"].tobytes(), res["t"].tobytes(), res["separators"].tobytes())


def test_repeat_and_shuffle_are_byte_identical(ctx):
    clusters, _ = ref.scene(n_images=120, n_clusters=8, seed=5)
    a = blob(dev_align(ctx, clusters))
    assert blob(dev_align(ctx, clusters)) == a
    rng = np.random.default_rng(0)
    shuffled = []
    for c in clusters:
        perm = rng.permutation(len(c["point_ids"]))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        ob = c["obs"][rng.permutation(len(c["obs"]))].copy()
        ob[:, 2] = inv[ob[:, 2]]
        shuffled.append(dict(image_ids=c["image_ids"][rng.permutation(len(c["image_ids"]))], point_ids=c["point_ids"][perm],
                             xyz=c["xyz"][perm], obs=ob))
    assert blob(dev_align(ctx, shuffled)) == a


def test_large_pair_200k_correspondences(ctx):
    rng = np.random.default_rng(9)
    n = 100000
    X = rng.uniform(-3, 3, (n, 3))
    R = ref.random_rotation(rng)
    Y = 1.7 * X @ R.T + np.array([0.5, -1.0, 2.0]) + rng.normal(0, 0.002, X.shape)
    bad = rng.random(n) < 0.1
    Y[bad] += rng.uniform(-5, 5, (int(bad.sum()), 3))
    obs = np.concatenate([np.stack([np.full(n, im), np.arange(n), np.arange(n)], 1) for im in (0, 1)])
    clusters = [cluster([0, 1, 2], X, obs), cluster([0, 1, 3], Y, obs)]
    dev = dev_align(ctx, clusters)
    (p,) = dev["pairs"]
    assert p["num_correspondences"] == 2 * n
    exp = ref.align(clusters)
    compare(dev, exp, min_clear=0.0)
    assert p["edge"] and abs(p["s"][0] - 1.7) < 1e-3 and np.abs(p["R"][0].reshape(3, 3) - R).max() < 1e-3


def test_thousand_pairs_in_one_call(ctx):
    # 50 clusters over the same 8 images: every pair shares them, 1 225 pairs
    rng = np.random.default_rng(4)
    n_pts = 40
    X = rng.uniform(-2, 2, (n_pts, 3))
    obs = np.array([(q % 8, q, q) for q in range(n_pts)] + [((q + 3) % 8, 1000 + q, q) for q in range(n_pts)])
    clusters, planted = [], []
    for c in range(50):
        s, R, t = float(rng.uniform(0.5, 2)), ref.random_rotation(rng), rng.uniform(-5, 5, 3)
        planted.append((s, R, t))
        keep = rng.random(len(obs)) >= 0.1
        clusters.append(cluster(range(8), s * X @ R.T + t + rng.normal(0, 0.002, X.shape), obs[keep],
                                ids=rng.choice(1 << 30, n_pts, replace=False)))
    dev = dev_align(ctx, clusters)
    assert len(dev["pairs"]) == 1225 and dev["report"].num_pairs == 1225
    assert dev["in_component"].all()
    check_recovery(dev, planted, 5e-3, 5e-3)
    # the restatement on every 25th pair
    corr = ref.join(clusters)
    for p in dev["pairs"][::25]:
        i, j = int(p["i"]), int(p["j"])
        ii, jj = corr[(i, j)]
        a, b = clusters[i]["xyz"][ii], clusters[j]["xyz"][jj]
        assert p["num_correspondences"] == len(a)
        o = ref.default_options()
        for d, (x, y) in enumerate(((a, b), (b, a))):
            e = ref.find_similarity(x, y, ref.align_seed(i, j, d), o)
            if min(e["residual_margin"], e["cost_margin"]) < MARGIN:
                continue
            assert p["num_inliers"][d] == e["inliers"] and p["iterations"][d] == e["iterations"]
            assert close(p["s"][d], e["s"]) and close(p["R"][d], np.ravel(e["R"])) and close(p["msd"][d], e["msd"])


def test_low_inlier_pair_runs_all_iterations(ctx):
    clusters, _ = pair_of(200, n_images=4, noise=0.001, seed=3, outliers=range(20, 200))  # 10 % inliers
    dev = dev_align(ctx, clusters, dict(max_reprojection_error=100.0))
    (p,) = dev["pairs"]
    assert list(p["iterations"]) == [5000, 5000]
    compare(dev, ref.align(clusters, ref.default_options(max_reprojection_error=100.0)), min_clear=0.0)


@pytest.mark.parametrize("n", [5, 6, 7])
def test_n_five_six_seven(ctx, n):
    clusters, (s, R, t) = pair_of(n, noise=0.001, seed=n)
    dev = dev_align(ctx, clusters)
    exp = ref.align(clusters)
    compare(dev, exp, min_clear=0.0)  # near-ties between all-inlier samples may leave PROSAC's choice unclear ...
    (p,) = dev["pairs"]
    (e,) = exp["pairs"]
    assert (p["iterations"][0] > 0) == (n > 5)
    # ... but every correspondence is an inlier, so the refit on them all does not depend on it
    assert list(p["num_inliers"]) == ([n, n] if n > 5 else [0, 0]) == e["inliers"]
    for d in (0, 1):
        assert close(p["s"][d], e["s"][d]) and close(p["R"][d], np.ravel(e["R"][d])) and close(p["msd"][d], e["msd"][d])
    assert abs(p["s"][0] - s) < 1e-2


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4])
def test_small_n(ctx, n):
    clusters, _ = pair_of(n)
    dev = dev_align(ctx, clusters)
    (p,) = dev["pairs"]
    assert p["num_correspondences"] == n and bool(p["edge"]) == (n >= 3)
    compare(dev, ref.align(clusters))


def test_single_cluster(ctx):
    clusters, _ = pair_of(10)
    dev = dev_align(ctx, clusters[:1])
    assert dev["anchor"] == 0 and len(dev["pairs"]) == 0 and dev["in_component"].all()
    assert dev["s"][0] == 1.0 and (dev["R"][0] == np.eye(3)).all() and (dev["t"][0] == 0).all()


def test_invalid_arguments(ctx):
    clusters, _ = pair_of(10)

    def bad(cl, **o):
        with pytest.raises(capi.DsmError):
            dev_align(ctx, cl, o)

    unreg = [dict(c) for c in clusters]
    unreg[1] = dict(unreg[1], obs=np.concatenate([unreg[1]["obs"], [[7, 99, 0]]]).astype(np.uint32))
    bad(unreg)
    rng_bad = [dict(c) for c in clusters]
    rng_bad[0] = dict(rng_bad[0], obs=np.concatenate([rng_bad[0]["obs"], [[0, 99, 10]]]).astype(np.uint32))
    bad(rng_bad)
    dup = [dict(c) for c in clusters]
    dup[0] = dict(dup[0], obs=np.concatenate([dup[0]["obs"], [[0, 0, 3]]]).astype(np.uint32))
    bad(dup)
    dupid = [dict(c) for c in clusters]
    dupid[1] = dict(dupid[1], point_ids=np.zeros(10, np.uint64))
    bad(dupid)
    bad(clusters, threshold=0.0)
    bad(clusters, threshold=-1.0)
    bad(clusters, max_iterations=5001)
    bad(clusters, max_iterations=50, min_iterations=100)
    bad(clusters, failure_probability=1.0)
    with pytest.raises(capi.DsmError):
        ctx.align_clusters([])
    # the context stays usable
    assert len(dev_align(ctx, clusters)["pairs"]) == 1
