"""Cluster alignment on the device (dsm_align_clusters) at its rulings and block edges: every entry of
tests/cluster_alignment_scenes.py against the restatement under the rule the CPU file (test_cluster_alignment_edges_cpu.py)
has established for it -- "clear": compare(...) all True, no pair skipped, and the device's own margins >= 1e-9; "graph":
counts, inliers, edge flags, the graph and the refitted Sim3s, whatever PROSAC's margins.  Then the raw C call: a
pairs_capacity below the pair count, the argument errors with their messages and the refusal of non-finite input."""
import ctypes
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import cluster_alignment_ref as ref
from tests import cluster_alignment_scenes as scenes
from tests.test_cluster_alignment_edges_cpu import named, restated
from tests.test_cluster_alignment_gpu import MARGIN, RTOL, close, compare, compare_pair, dev_align

pytestmark = pytest.mark.gpu
COMPARISONS = scenes.comparisons()
# entries whose expected values hold NaN: compare()'s close() has no NaN, they are compared field by field below
NAN_ENTRIES = ("source_at_one_place", "destination_at_one_place", "degenerate_head_one_iteration")
CLEAR = [c[0] for c in COMPARISONS if c[4] == "clear" and c[0] not in NAN_ENTRIES]
GRAPH = [c[0] for c in COMPARISONS if c[4] == "graph"]


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def device(ctx, name):
    _, clusters, opt, seeds, _ = named(name)
    return dev_align(ctx, clusters, opt, seeds)


def same(x, y, rtol=RTOL):
    """close(), with NaN where and only where the expected value has it"""
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    nan = np.isnan(y)
    return bool((np.isnan(x) == nan).all()) and close(x[~nan], y[~nan], rtol)


def check_counts(dev, exp):
    assert list(dev["separators"]) == list(exp["separators"])
    assert [(int(p["i"]), int(p["j"])) for p in dev["pairs"]] == [(p["i"], p["j"]) for p in exp["pairs"]]
    for dp, ep in zip(dev["pairs"], exp["pairs"]):
        assert int(dp["num_common_images"]) == ep["num_common_images"] and int(dp["num_correspondences"]) == ep["num_correspondences"]
        assert list(dp["num_inliers"]) == ep["inliers"] and bool(dp["edge"]) == ep["edge"], (ep["i"], ep["j"])
    rep = dev["report"]
    assert rep.num_pairs == len(exp["pairs"]) and rep.num_edges == exp["num_edges"] and rep.num_separators == len(exp["separators"])


def check_graph(dev, exp):
    assert dev["anchor"] == exp["anchor"] and list(dev["in_component"]) == list(exp["in_component"])
    assert list(dev["mst_parent"]) == list(exp["mst_parent"])
    assert dev["report"].num_in_component == int(exp["in_component"].sum())
    assert close(dev["s"], exp["s"]) and close(dev["R"], exp["R"], 1e-11) and close(dev["t"], exp["t"], 1e-11)  # as compare()


# ---------------------------------------------------------------- rule "clear"
@pytest.mark.parametrize("name", CLEAR)
def test_clear_entry_equals_the_restatement(ctx, name):
    dev = device(ctx, name)
    exp = restated(name)
    assert len(exp["pairs"]) >= 1
    assert compare(dev, exp) == [True] * len(exp["pairs"])
    rep = dev["report"]
    print("%s: device margins residual %.3e cost %.3e weight %.3e" % (name, rep.min_residual_margin, rep.min_cost_margin,
                                                                      rep.min_weight_margin))
    assert rep.min_residual_margin >= MARGIN and rep.min_cost_margin >= MARGIN
    assert rep.prosac_iterations == sum(sum(p["iterations"]) for p in exp["pairs"])
    check_graph(dev, exp)


@pytest.fixture(scope="module")
def chunk_edges(ctx):
    return device(ctx, "chunk_edges")


@pytest.mark.parametrize("k", range(len(scenes.CHUNK_NS)), ids=["n_%d" % n for n in scenes.CHUNK_NS])
def test_chunk_edge_pair_by_pair(chunk_edges, k):
    """The pairs of the one call one by one, so that a failure names its N."""
    dp, ep = chunk_edges["pairs"][k], restated("chunk_edges")["pairs"][k]
    assert ep["num_correspondences"] == scenes.CHUNK_NS[k]
    assert compare_pair(dp, ep) is True


def test_chunk_edges_cover_every_tail(ctx):
    dev = device(ctx, "chunk_edges")
    assert [int(p["num_correspondences"]) for p in dev["pairs"]] == list(scenes.CHUNK_NS)
    assert [int(p["num_correspondences"]) % 256 for p in dev["pairs"]] == [255, 0, 1, 255, 0, 1, 1]
    assert all(p["edge"] for p in dev["pairs"]) and dev["report"].num_prosac_problems == 2 * len(scenes.CHUNK_NS)


def test_runs_end_at_the_trial_asked_for(ctx):
    for it in scenes.BATCH_ENDS:
        (p,) = device(ctx, "batch_end_%d" % it)["pairs"]
        assert list(p["iterations"]) == [it, it]
    for name in ("min_iterations_0", "one_iteration"):
        (p,) = device(ctx, name)["pairs"]
        assert list(p["iterations"]) == [1, 1] and p["edge"]
    (p,) = device(ctx, "four_or_five_inliers")["pairs"]
    assert list(p["iterations"]) == [2227, 2234] and list(p["num_inliers"]) == [5, 5]
    cl = scenes.five_of_nine()
    for d, (x, y) in enumerate(((cl[0]["xyz"], cl[1]["xyz"]), (cl[1]["xyz"], cl[0]["xyz"]))):  # refitted on all 9
        s, R, t = ref.fit_all(x, y, 1.0, np.eye(3), np.zeros(3))
        assert close(p["s"][d], s) and close(p["R"][d], np.ravel(R)) and close(p["t"][d], t)
        assert not close(p["s"][d], p["prosac_s"][d], 1e-3)


def test_rulings_on_the_device(ctx):
    dev = device(ctx, "one_common_image")
    assert [(int(p["i"]), int(p["j"])) for p in dev["pairs"]] == [(1, 2)] and list(dev["separators"]) == [0, 10, 11]
    assert dev["report"].num_correspondences == 10 + 40  # the shared keys of (0, 1) are joined, but (0, 1) is no pair
    assert list(dev["in_component"]) == [False, True, True]
    (p,) = device(ctx, "fewer_than_four_inliers")["pairs"]
    assert list(p["iterations"]) == [5000, 5000] and list(p["msd"]) == [ref.DBL_MAX] * 2 and not p["edge"]
    dev = device(ctx, "weight_above_limit")
    (p,) = dev["pairs"]
    assert list(p["num_inliers"]) == [10, 10] and not p["edge"] and p["weight"] > 1.8 and dev["report"].num_edges == 0
    assert list(dev["in_component"]) == [True, False] and dev["anchor"] == 0


# ---------------------------------------------------------------- expected values with NaN
def check_nan_entry(dev, exp):
    check_counts(dev, exp)
    check_graph(dev, exp)
    for dp, ep in zip(dev["pairs"], exp["pairs"]):
        assert ep["margin"] >= MARGIN
        assert list(dp["iterations"]) == ep["iterations"]
        for d in (0, 1):
            for key in ("s", "R", "t", "prosac_cost", "prosac_s", "prosac_R", "prosac_t"):
                assert same(dp[key][d], ep[key][d]), (key, d)
            assert dp["msd"][d] == ref.DBL_MAX if ep["msd"][d] == ref.DBL_MAX else same(dp["msd"][d], ep["msd"][d]), d


def test_source_at_one_place_is_no_edge(ctx):
    dev = device(ctx, "source_at_one_place")
    check_nan_entry(dev, restated("source_at_one_place"))
    (p,) = dev["pairs"]
    assert p["num_correspondences"] == 4 and math.isnan(p["msd"][0]) and not p["edge"] and dev["report"].num_edges == 0


def test_destination_at_one_place_keeps_the_small_scale_path(ctx):
    dev = device(ctx, "destination_at_one_place")
    exp = restated("destination_at_one_place")
    check_nan_entry(dev, exp)
    (p,) = dev["pairs"]
    (e,) = exp["pairs"]
    # FindRTS returns after setting s and before dividing R or writing t: exactly s = 0, R = cR = 0, t = Sim3()'s 0
    assert p["s"][0] == 0.0 == e["s"][0] and (p["R"][0] == 0.0).all() and (p["t"][0] == 0.0).all()
    assert close(p["msd"][0], scenes.DESTINATION_MSD)
    assert math.isnan(p["msd"][1]) and not p["edge"] and dev["report"].num_edges == 0


def test_degenerate_first_sample_alone(ctx):
    dev = device(ctx, "degenerate_head_one_iteration")
    check_nan_entry(dev, restated("degenerate_head_one_iteration"))
    (p,) = dev["pairs"]
    assert p["num_correspondences"] == 44 and list(p["iterations"]) == [1, 1] and list(p["num_inliers"]) == [0, 0]
    assert all(math.isnan(s) for s in p["prosac_s"]) and list(p["prosac_cost"]) == [44 * scenes.THRESHOLD] * 2
    assert list(p["msd"]) == [ref.DBL_MAX] * 2 and not p["edge"]


# ---------------------------------------------------------------- rule "graph"
@pytest.mark.parametrize("name", GRAPH)
def test_graph_entry_equals_the_restatement(ctx, name):
    dev = device(ctx, name)
    exp = restated(name)
    check_counts(dev, exp)
    check_graph(dev, exp)
    for dp, ep in zip(dev["pairs"], exp["pairs"]):
        for d in (0, 1):
            assert close(dp["s"][d], ep["s"][d]) and close(dp["R"][d], np.ravel(ep["R"][d])) and close(dp["t"][d], ep["t"][d])
            assert close(dp["msd"][d], ep["msd"][d])


def test_five_clusters_on_the_device(ctx):
    dev = device(ctx, "graph_five_clusters")
    assert [(int(p["i"]), int(p["j"]), int(p["num_correspondences"])) for p in dev["pairs"]] == [(1, 2, 30), (2, 3, 30), (3, 4, 30)]
    assert [bool(p["edge"]) for p in dev["pairs"]] == [True, False, True]
    assert pair_of_dev(dev, 2, 3)["weight"] > 1.8  # dropped by the limit alone: 10 inliers, a finite weight
    assert list(dev["in_component"]) == [False, True, True, False, False]  # two components of two: the smaller index wins
    assert dev["anchor"] == 2 and list(dev["mst_parent"]) == [-1, 2, -1, -1, -1]
    for c in (0, 3, 4):
        assert dev["s"][c] == 1.0 and (dev["R"][c] == np.eye(3)).all() and (dev["t"][c] == 0.0).all()
    p12 = pair_of_dev(dev, 1, 2)
    assert dev["s"][1] == p12["s"][0] and (dev["R"][1].ravel() == p12["R"][0]).all() and (dev["t"][1] == p12["t"][0]).all()
    assert dev["report"].num_correspondences == 120 and dev["report"].num_in_component == 2


def pair_of_dev(dev, i, j):
    return next(p for p in dev["pairs"] if (int(p["i"]), int(p["j"])) == (i, j))


def test_tied_path_on_the_device(ctx):
    dev = device(ctx, "graph_tied_path")
    e, f = scenes.TIED_EDGES
    we, wf = pair_of_dev(dev, *e)["weight"], pair_of_dev(dev, *f)["weight"]
    assert we == wf  # the same correspondences in the same order: Kruskal's comparator falls through to (i, j)
    assert dev["in_component"].all() and dev["anchor"] == 2 and list(dev["mst_parent"]) == [1, 2, -1, 2, 1]
    assert dev["s"][0] == dev["s"][4] and (dev["R"][0] == dev["R"][4]).all() and (dev["t"][0] == dev["t"][4]).all()


# ---------------------------------------------------------------- the join
def test_same_keys_three_pairs(ctx):
    dev = device(ctx, "same_keys")
    assert [(int(p["i"]), int(p["j"]), int(p["num_correspondences"])) for p in dev["pairs"]] == [(0, 1, 90), (0, 2, 90), (1, 2, 90)]
    assert dev["report"].num_correspondences == 270 and dev["report"].num_observations == 270


@pytest.mark.parametrize("kind", ["nothing", "images_only"])
def test_empty_cluster_leaves_the_other_pairs_alone(ctx, kind):
    base = device(ctx, "empty_base")
    fields = [f for f in capi.ALIGN_PAIR_DTYPE.names if f not in ("i", "j")]
    for where in ("first", "middle", "last"):
        dev = device(ctx, "empty_%s_%s" % (kind, where))
        pos = scenes.with_empty(kind, where)[2]
        for p in base["pairs"]:
            q = pair_of_dev(dev, int(p["i"]) + (p["i"] >= pos), int(p["j"]) + (p["j"] >= pos))
            assert all(p[f].tobytes() == q[f].tobytes() for f in fields)
        extra = [p for p in dev["pairs"] if pos in (int(p["i"]), int(p["j"]))]
        assert len(extra) == (2 if kind == "images_only" else 0)
        for p in extra:
            assert p["num_correspondences"] == 0 and not p["edge"] and p["num_common_images"] == 4
            assert np.isnan(p["msd"]).all() and math.isnan(p["weight"]) and list(p["iterations"]) == [0, 0]
        assert not dev["in_component"][pos] and dev["in_component"].sum() == 3
        assert dev["s"][pos] == 1.0 and (dev["R"][pos] == np.eye(3)).all() and (dev["t"][pos] == 0.0).all()
        keep = [c for c in range(len(dev["s"])) if c != pos]
        assert dev["s"][keep].tobytes() == base["s"].tobytes() and dev["t"][keep].tobytes() == base["t"].tobytes()


# ---------------------------------------------------------------- the raw C call
def raw_align(ctx, flat, K=None, options=None, capacity=None, **replace):
    """dsm_align_clusters on the arrays of scenes.flatten(); replace: argument name -> None (a NULL) or another array.
    Returns (rc, message, outputs)."""
    K = flat["K"] if K is None else K
    n = max(flat["K"], 1)
    cap = n * (n - 1) // 2 + 1 if capacity is None else capacity
    out = dict(pairs=np.zeros(max(cap, 1), capi.ALIGN_PAIR_DTYPE), n_pairs=np.zeros(1, np.uint32),
               anchor=np.zeros(1, np.int32), in_component=np.zeros(n, np.uint8), mst_parent=np.zeros(n, np.int32),
               sim3=np.zeros((n, 13)), separators=np.zeros(max(len(flat["image_ids"]), 1), np.uint32), n_separators=np.zeros(1, np.uint32))
    arrays = dict(flat, **out)
    arrays.update(replace)
    ptr = lambda key: None if arrays[key] is None else arrays[key].ctypes.data
    opt = None if options is None else ctypes.byref(options)
    rc = ctx._L.dsm_align_clusters(ctx._h, K, ptr("image_offsets"), ptr("image_ids"), ptr("point_offsets"), ptr("point_ids"), ptr("xyz"),
                                   ptr("obs_offsets"), ptr("obs"), opt, None, ptr("pairs"), cap, ptr("n_pairs"), ptr("anchor"),
                                   ptr("in_component"), ptr("mst_parent"), ptr("sim3"), ptr("separators"), ptr("n_separators"), None)
    return rc, ctx._L.dsm_last_error(ctx._h).decode(), out


INVALID = 1  # DSM_ERR_INVALID_ARGUMENT


def test_pairs_capacity_below_the_pair_count(ctx):
    _, clusters, opt, seeds, _ = named("same_keys")
    full = device(ctx, "same_keys")
    assert len(full["pairs"]) == 3
    buf = np.zeros(3, capi.ALIGN_PAIR_DTYPE)
    buf.view(np.uint8)[:] = 0xAB
    rc, msg, out = raw_align(ctx, scenes.flatten(clusters), capacity=1, pairs=buf)
    assert rc == 0, msg
    assert out["n_pairs"][0] == 3
    assert buf[0].tobytes() == full["pairs"][0].tobytes()
    assert (buf[1:].view(np.uint8) == 0xAB).all()
    assert out["anchor"][0] == full["anchor"] and list(out["mst_parent"]) == list(full["mst_parent"])
    rc, msg, out = raw_align(ctx, scenes.flatten(clusters), capacity=0, pairs=None)
    assert rc == 0 and out["n_pairs"][0] == 3  # no capacity, no buffer: the count alone


def test_argument_errors_say_what_is_wrong(ctx):
    clusters = scenes.chunk_pair(255)
    flat = scenes.flatten(clusters)

    def refused(text, **kw):
        rc, msg, _ = raw_align(ctx, flat, **kw)
        assert rc == INVALID and text in msg, (rc, msg)

    refused("num_clusters must be in [1, 65536]", K=0)
    refused("num_clusters must be in [1, 65536]", K=65537)
    for key in ("image_offsets", "point_offsets", "obs_offsets"):
        up = flat[key].copy()
        up[0] = 1
        refused("offsets must start at 0", **{key: up})
        down = flat[key].copy()
        down[1], down[2] = down[2], down[1]
        refused("offsets must be non-decreasing", **{key: down})
        refused("NULL argument", **{key: None})
    for key in ("image_ids", "point_ids", "xyz", "obs", "separators", "n_pairs", "anchor", "in_component", "mst_parent", "sim3",
                "n_separators", "pairs"):
        refused("NULL argument", **{key: None})

    def flagged(text, cl, **o):
        with pytest.raises(capi.DsmError, match=text):
            dev_align(ctx, cl, o)

    a, b = clusters
    more = lambda c, row: dict(c, obs=np.concatenate([c["obs"], [row]]).astype(np.uint32))
    flagged("an observation on an image its cluster has not registered", [a, more(b, [7, 999, 0])])
    flagged("a point index out of range", [more(a, [0, 999, 255]), b])
    flagged(r"a repeated \(image_id, point2D_idx\) inside one cluster", [more(a, [0, 0, 3]), b])
    flagged("a repeated point id inside one cluster", [a, dict(b, point_ids=np.r_[b["point_ids"][:-1], b["point_ids"][0]])])
    # observations, but no point to index
    flagged("a point index out of range", [a, dict(b, xyz=np.zeros((0, 3)), point_ids=np.zeros(0, np.uint64))])
    for o in (dict(threshold=0.0), dict(threshold=-1.0), dict(max_iterations=5001), dict(max_iterations=0),
              dict(max_iterations=50, min_iterations=100), dict(min_iterations=-1), dict(failure_probability=1.0),
              dict(failure_probability=0.0), dict(max_reprojection_error=-1.0), dict(max_reprojection_error=math.nan)):
        flagged("option out of range", clusters, **o)
    # the context still works
    assert compare(device(ctx, "chunk_edges"), restated("chunk_edges")) == [True] * len(scenes.CHUNK_NS)


def test_non_finite_input_is_refused(ctx):
    clusters = scenes.chunk_pair(255)
    for c, q, d, bad in ((0, 0, 0, math.nan), (1, 254, 2, math.inf), (0, 100, 1, -math.inf)):
        xyz = np.array(clusters[c]["xyz"], np.float64)
        xyz[q, d] = bad
        cl = list(clusters)
        cl[c] = dict(clusters[c], xyz=xyz)
        with pytest.raises(capi.DsmError, match="non-finite point_xyz"):
            dev_align(ctx, cl)
    for thr in (math.nan, math.inf, -math.inf):
        with pytest.raises(capi.DsmError, match="non-finite threshold"):
            dev_align(ctx, clusters, dict(threshold=thr))
    (p,) = dev_align(ctx, clusters)["pairs"]
    assert p["edge"] and p["num_correspondences"] == 255
