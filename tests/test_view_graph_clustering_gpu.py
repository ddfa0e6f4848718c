"""View-graph clustering on the device (dsm_view_graph_cluster; ClusteringScenes) against the numpy
restatement (tests/view_graph_clustering_ref.py): the Ritz values and the subspace by tolerance (eigh there, a
Chebyshev-filtered subspace iteration here), the labels, edge clusters and cluster image lists identical wherever the
restatement's k-means decisions are clear of rounding; byte-identical repeats and shuffles, labels_in, the argument errors."""
import math

import numpy as np
import pytest

from tests import view_graph_clustering_ref as ref
from tests.test_view_graph_clustering_cpu import planted, same_partition

MARGIN = 1e-6
EV_RTOL = 1e-10


def random_graph(n, deg, seed):
    rng = np.random.default_rng(seed)
    s = set()
    for i in range(n):
        for j in rng.choice(n, deg, replace=False):
            if i != j:
                s.add((min(i, int(j)), max(i, int(j))))
    p = np.array(sorted(s), np.uint32)
    p = p[rng.permutation(len(p))]
    return p, rng.integers(15, 500, len(p)).astype(np.int32)


def sequence_graph(n, half, seed):
    rng = np.random.default_rng(seed)
    p = np.array([(i, i + d) for i in range(n) for d in range(1, half + 1) if i + d < n], np.uint32)
    return p, rng.integers(15, 500, len(p)).astype(np.int32)


def check_spectrum(dev, exp, opts_tol=1e-10):
    """Ritz values, residuals and the Davis-Kahan bound on the subspace: sin(angle) <= ||R||_2 / gap with
    ||R||_2 <= sqrt(k) * the worst column residual (2 x for k <= 4)."""
    r = dev["report"]
    k = exp["k"]
    ev = exp["eigenvalues"]
    assert r.max_eigen_residual_ratio <= opts_tol
    assert np.all(np.abs(dev["eigenvalues"][:k] - ev[:k]) <= EV_RTOL * np.maximum(np.abs(ev[:k]), 1.0)), \
        np.abs(dev["eigenvalues"][:k] - ev[:k]).max()
    gap = ev[k] - ev[k - 1]
    assert gap > 0
    sine = ref.principal_sine(dev["eigenvectors"], exp["subspace"])
    bound = max(2.0, math.sqrt(k)) * r.max_eigen_residual / gap
    eigh_err = 100 * np.finfo(np.float64).eps * np.abs(ev).max() / gap  # eigh's own backward error, seen through the gap
    assert sine <= bound + eigh_err, (sine, bound, eigh_err)
    # the (k+1)-th Ritz value is not iterated to the tolerance; by interlacing it lies above lambda_(k+1)
    assert r.ncv == k or r.eigen_gap >= gap - 1e-8 * max(1.0, abs(gap))
    return sine, bound


def check_same(dev, exp):
    assert np.array_equal(dev["image_ids"], exp["image_ids"])
    assert dev["labels"].tolist() == exp["labels"].tolist()
    assert dev["edge_cluster"].tolist() == exp["edge_cluster"].tolist()
    assert [c.tolist() for c in dev["clusters"]] == [c.tolist() for c in exp["clusters"]]
    r = dev["report"]
    assert (r.num_images, r.num_edges, r.num_clusters) == (len(exp["image_ids"]), exp["num_edges"], len(exp["clusters"]))
    assert (r.num_lost_edges, r.num_readded_edges) == (exp["num_lost_edges"], exp["num_readded_edges"])
    assert (r.clustered_images_num, r.clustered_edges_num) == (exp["clustered_images_num"], exp["clustered_edges_num"])


def check_same_where_clear(dev, exp):
    """Everything identical when every recorded decision margin is >= MARGIN; otherwise the labels of the points whose every
    Lloyd decision was clear (the k-means++ draws must all be clear).  Returns True for the full comparison."""
    if ref.min_margin(exp) >= MARGIN:
        check_same(dev, exp)
        assert dev["report"].kmeans_iterations == exp["kmeans_iterations"]
        return True
    n = len(exp["labels"])
    assert (exp["draw_margins"] >= MARGIN).all()
    clear = (exp["lloyd_margins"].reshape(-1, n) >= MARGIN).all(axis=0)
    assert clear.mean() > 0.9
    assert np.array_equal(dev["labels"][clear], exp["labels"][clear])
    return False


def compare(dsm, pairs, w, ub, use=None, full=True, **kw):
    opts = _opts(num_images_ub=ub, **kw)
    dev = dsm.cluster_view_graph(pairs, w, use=use, options=opts)
    exp = ref.cluster(pairs, w, use=use, num_images_ub=ub, **kw)
    check_spectrum(dev, exp)
    assert check_same_where_clear(dev, exp) or not full, "fixture on a knife edge"
    return dev, exp


def _opts(**kw):
    from dagsfm_amd import capi
    return capi.default_clustering_options(**kw)


@pytest.mark.gpu
@pytest.mark.parametrize("n_blocks,size,seed", [(6, 100, 1), (20, 100, 4)])
def test_planted_partitions(dsm, n_blocks, size, seed):
    pairs, w, truth = planted(n_blocks, size, seed)
    dev, _ = compare(dsm, pairs, w, size)
    assert same_partition(dev["labels"], dev["image_ids"], truth)
    assert dev["report"].eigen_iterations > 0 and dev["report"].ncv == 2 * n_blocks


@pytest.mark.gpu
def test_random_1000_k10(dsm):
    pairs, w = random_graph(1000, 8, 21)
    compare(dsm, pairs, w, 100, full=False)  # Lloyd margins down to 1e-8 here: the labels of the clear points


@pytest.mark.gpu
def test_sequence_400_k4_small_gaps(dsm):
    pairs, w = sequence_graph(400, 4, 22)
    opts = _opts(num_images_ub=100)
    dev = dsm.cluster_view_graph(pairs, w, options=opts)
    exp = ref.cluster(pairs, w, num_images_ub=100)
    check_spectrum(dev, exp)
    check_same_where_clear(dev, exp)


@pytest.mark.gpu
def test_chained_through_cycle_filter_and_rotation_averaging(dsm):
    from tests.test_rotation_averaging import CASES
    p, q, _, _ = CASES["300x30_noise"]()
    keep, _ = dsm.view_graph_filter_cycles(p, q, 5.0)
    ra = dsm.rotation_averaging(p, q, use=keep)
    fin = set(ra["image_ids"][ra["in_final_cc"]].tolist())
    use = (ra["edge_state"] == 3) & np.array([a in fin and b in fin for a, b in p.tolist()])
    w = np.random.default_rng(23).integers(15, 400, len(p)).astype(np.int32)
    dev, exp = compare(dsm, p, w, 100, use=use.astype(np.uint8))
    assert dev["report"].num_clusters == len(fin) // 100 >= 2
    assert (dev["edge_cluster"][~use] == -1).all()


@pytest.mark.gpu
def test_repeats_are_byte_identical_and_shuffles_do_not_matter(dsm):
    pairs, _ = random_graph(1000, 8, 21)
    w = (np.random.default_rng(5).permutation(len(pairs)) + 15).astype(np.int32)  # distinct weights: no tie in Expand
    opts = _opts(num_images_ub=100)
    a = dsm.cluster_view_graph(pairs, w, options=opts)
    b = dsm.cluster_view_graph(pairs, w, options=opts)
    for key in ("image_ids", "labels", "edge_cluster", "offsets", "eigenvalues", "eigenvectors"):
        assert a[key].tobytes() == b[key].tobytes(), key
    o = np.random.default_rng(6).permutation(len(pairs))
    sw = o.copy()
    sw_pairs = pairs[o].copy()
    flip = np.random.default_rng(7).random(len(o)) < 0.5
    sw_pairs[flip] = sw_pairs[flip][:, ::-1]
    c = dsm.cluster_view_graph(sw_pairs, w[sw], options=opts)
    inv = np.argsort(o)
    for key in ("image_ids", "labels", "offsets", "eigenvalues", "eigenvectors"):
        assert a[key].tobytes() == c[key].tobytes(), key
    assert c["edge_cluster"][inv].tobytes() == a["edge_cluster"].tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a["clusters"], c["clusters"]))


@pytest.mark.gpu
def test_k_one_runs_no_solver(dsm):
    pairs, w = random_graph(150, 6, 8)
    for ub in (100, 1000):
        dev = dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=ub))
        r = dev["report"]
        assert r.eigen_iterations == 0 and r.operator_applications == 0 and r.kmeans_iterations == 0
        assert (dev["labels"] == 0).all() and r.num_clusters == 1 and r.num_lost_edges == 0
        assert dev["clusters"][0].tolist() == dev["image_ids"].tolist()
        assert dev["eigenvalues"] is None


@pytest.mark.gpu
@pytest.mark.parametrize("expand", [1, 0])
def test_labels_in_matches_restatement(dsm, expand):
    pairs, w = random_graph(600, 6, 9)
    ids, _ = ref.prepare(pairs, w)
    lab = np.random.default_rng(10).integers(0, 6, len(ids)).astype(np.uint32)
    dev = dsm.cluster_view_graph(pairs, w, labels_in=lab, options=_opts(num_images_ub=100, expand=expand))
    exp = ref.cluster(pairs, w, labels_in=lab, num_images_ub=100, expand=bool(expand))
    check_same(dev, exp)
    assert dev["report"].eigen_iterations == 0
    if expand:
        assert dev["report"].num_readded_edges > 0


@pytest.mark.gpu
def test_invalid_arguments(dsm):
    from dagsfm_amd import capi
    pairs, w = random_graph(300, 6, 11)
    for kw in ({"num_images_ub": 0}, {"image_overlap": 2}, {"image_overlap": 0}, {"completeness_ratio": 1.5},
               {"num_images_ub": 1}):  # the last: k = N >= N
        with pytest.raises(capi.DsmError) as e:
            dsm.cluster_view_graph(pairs, w, options=_opts(**kw))
        assert "error 1" in str(e.value) or "INVALID" in str(e.value) or "(1)" in str(e.value), str(e.value)
    bad = w.copy()
    bad[3] = -1
    with pytest.raises(capi.DsmError):
        dsm.cluster_view_graph(pairs, bad)


@pytest.mark.gpu
def test_eigen_iteration_cap_is_not_converged(dsm):
    from dagsfm_amd import capi
    pairs, w = random_graph(1000, 8, 21)
    with pytest.raises(capi.DsmError) as e:
        dsm.cluster_view_graph(pairs, w, options=_opts(num_images_ub=100, max_eigen_iterations=1))
    assert "residual" in str(e.value)
