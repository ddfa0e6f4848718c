"""CPU-only: the restatement's verdict (tests/cluster_alignment_ref.py) on every entry of tests/cluster_alignment_scenes.py, so
that tests/test_cluster_alignment_edges_gpu.py can hold the device to the strict rule on all of them.  A "clear" entry has no
pair with a margin below 1e-9; a "graph" entry meets the conditions under which its graph does not depend on PROSAC's choice.
Also the shape every scene promises by its name, and the restatement's own order of wide ids."""
import functools
import math

import numpy as np
import pytest

from tests import cluster_alignment_ref as ref
from tests import cluster_alignment_scenes as scenes

MARGIN = 1e-9  # tests/test_cluster_alignment_gpu.py's
COMPARISONS = scenes.comparisons()
NAMES = [c[0] for c in COMPARISONS]
CLEAR = [c[0] for c in COMPARISONS if c[4] == "clear"]
GRAPH = [c[0] for c in COMPARISONS if c[4] == "graph"]


def named(name):
    return next(c for c in COMPARISONS if c[0] == name)


@functools.lru_cache(maxsize=None)
def restated(name, user_seed=None):
    _, clusters, opt, seeds, _ = named(name)
    o = ref.default_options(**opt)
    if user_seed is not None:
        o["random_seed"] = user_seed
        seeds = None
    with np.errstate(all="ignore"):
        return ref.align(clusters, o, seeds)


def pair(res, i, j):
    return next(p for p in res["pairs"] if (p["i"], p["j"]) == (i, j))


def test_names_are_unique_and_every_rule_is_known():
    assert len(set(NAMES)) == len(NAMES)
    assert set(c[4] for c in COMPARISONS) == {"clear", "graph"}
    assert sum(len(scenes.of_kind(kind)) for kind, _ in scenes.KINDS) == len(COMPARISONS)


@pytest.mark.parametrize("name", CLEAR)
def test_every_pair_of_a_clear_entry_is_clear(name):
    """The cap: no clear-rule entry holds an unclear pair, so compare() on the device may not skip any."""
    res = restated(name)
    for p in res["pairs"]:
        print("%s (%d, %d): N %d, margin %.3e (residual %.3e %.3e, cost %.3e %.3e, weight %.3e, float %.3e), inliers %s, "
              "iterations %s, edge %d" % (name, p["i"], p["j"], p["num_correspondences"], p["margin"], *p["residual_margin"],
                                          *p["cost_margin"], p["weight_margin"], p["float_margin"], p["inliers"], p["iterations"],
                                          p["edge"]))
        assert p["margin"] >= MARGIN, (name, p["i"], p["j"])


def cycle_free(K, edges):
    uf = list(range(K))

    def find(x):
        while uf[x] != x:
            x = uf[x]
        return x

    for _, i, j in edges:
        a, b = find(i), find(j)
        if a == b:
            return False
        uf[a] = b
    return True


@pytest.mark.parametrize("name", GRAPH)
def test_graph_entries_do_not_depend_on_prosac(name):
    """What makes the "graph" rule sound: no weight near the limit, inlier counts that no stream of draws changes (so the
    refit sees the same correspondences whatever PROSAC's best sample was), and no equal float32 weights on a cycle, where
    Kruskal's order would decide the tree."""
    _, clusters, opt, _, _ = named(name)
    o = ref.default_options(**opt)
    res = restated(name)
    others = [restated(name, us) for us in (1, 2, 3)]
    edges = []
    for k, p in enumerate(res["pairs"]):
        print("%s (%d, %d): N %d, inliers %s, weight %r, weight margin %.3e, float margin %.3e, edge %d"
              % (name, p["i"], p["j"], p["num_correspondences"], p["inliers"], p["weight"], p["weight_margin"], p["float_margin"],
                 p["edge"]))
        assert p["weight_margin"] >= 0.1
        assert p["float_margin"] >= MARGIN
        N = p["num_correspondences"]
        for d in (0, 1):
            assert p["inliers"][d] == N or all(r["pairs"][k]["inliers"][d] == p["inliers"][d] for r in others)
        for r in others:
            assert r["pairs"][k]["edge"] == p["edge"]
            if p["msd"][0] != ref.DBL_MAX:
                assert abs(r["pairs"][k]["weight"] - p["weight"]) <= 1e-12 * p["weight"]
        if p["edge"] and res["in_component"][p["i"]]:
            edges.append((np.float32(p["weight"]), p["i"], p["j"]))
    w = [e[0] for e in edges]
    assert cycle_free(len(clusters), edges) or len(set(w)) == len(w)


# ---------------------------------------------------------------- the shapes the names promise
def test_chunk_edges_sizes_and_results():
    res = restated("chunk_edges")
    assert [p["num_correspondences"] for p in res["pairs"]] == list(scenes.CHUNK_NS)
    assert [(p["i"], p["j"]) for p in res["pairs"]] == [(2 * k, 2 * k + 1) for k in range(len(scenes.CHUNK_NS))]
    for p, n in zip(res["pairs"], scenes.CHUNK_NS):
        assert p["edge"] and p["iterations"] == [100, 100]
        assert all(0.6 * n <= c <= 0.72 * n for c in p["inliers"])  # the 70 % without a moved point, less the noisy ones
        # the explicit seeds restate the pair as the two-cluster scene it came from
        (q,) = ref.align(scenes.chunk_pair(n))["pairs"]
        assert q["msd"] == p["msd"] and q["inliers"] == p["inliers"]


@pytest.mark.parametrize("it", scenes.BATCH_ENDS)
def test_batch_ends_run_exactly_that_many_trials(it):
    (p,) = restated("batch_end_%d" % it)["pairs"]
    assert p["iterations"] == [it, it] and p["num_correspondences"] == 300


def test_short_runs():
    for name in ("min_iterations_0", "one_iteration"):
        (p,) = restated(name)["pairs"]
        assert p["iterations"] == [1, 1] and p["edge"] and p["inliers"] == [50, 50]


def test_four_or_five_inliers_end_inside_the_ninth_batch():
    (p,) = restated("four_or_five_inliers")["pairs"]
    assert p["inliers"] == [5, 5] and p["iterations"] == [2227, 2234]
    assert all(8 * ref.BATCH < it < 9 * ref.BATCH for it in p["iterations"])
    cl = scenes.five_of_nine()
    a, b = cl[0]["xyz"], cl[1]["xyz"]
    for d, (x, y) in enumerate(((a, b), (b, a))):  # refitted on all 9, not on the 5
        s, R, t = ref.fit_all(x, y, 1.0, np.eye(3), np.zeros(3))
        assert p["s"][d] == s and (p["R"][d] == R).all() and (p["t"][d] == t).all()
        assert not np.allclose(p["s"][d], p["prosac_s"][d], rtol=1e-3)
    assert p["edge"] and 1.8 < p["weight"] < 10.0


def test_rulings_rule_as_stated():
    res = restated("one_common_image")
    assert [(p["i"], p["j"]) for p in res["pairs"]] == [(1, 2)]
    assert list(res["separators"]) == [0, 10, 11]  # one common image is a separator (the reference inserts it), not a pair
    assert len(ref.join(named("one_common_image")[1])[(0, 1)][0]) == 10  # correspondences, but no pair
    (p,) = restated("fewer_than_four_inliers")["pairs"]
    assert p["iterations"] == [5000, 5000] and min(p["inliers"]) < 4 and p["msd"] == [ref.DBL_MAX, ref.DBL_MAX] and not p["edge"]
    (p,) = restated("weight_above_limit")["pairs"]
    assert p["inliers"] == [10, 10] and p["iterations"] == [370, 370] and not p["edge"]
    assert abs(p["weight"] - 3.38) < 0.01 and p["weight"] != ref.DBL_MAX
    res = restated("source_at_one_place")
    (p,) = res["pairs"]
    assert p["num_correspondences"] == 4 and math.isnan(p["msd"][0]) and not p["edge"] and res["num_edges"] == 0


def test_destination_at_one_place_takes_the_small_scale_path():
    res = restated("destination_at_one_place")
    (p,) = res["pairs"]
    assert p["s"][0] == 0.0 and (p["R"][0] == 0.0).all() and (p["t"][0] == 0.0).all()
    assert abs(p["msd"][0] - scenes.DESTINATION_MSD) <= 1e-15
    assert math.isnan(p["msd"][1]) and math.isnan(p["s"][1]) and not p["edge"] and res["num_edges"] == 0


def test_degenerate_head():
    cl = named("degenerate_head_seed_0")[1]
    ii, jj = ref.join(cl)[(0, 1)]
    assert len(ii) == 44 and list(ii[:5]) == [0] * 5 and list(jj[:5]) == [0] * 5
    for us in (0, 1):
        (p,) = restated("degenerate_head_seed_%d" % us)["pairs"]
        assert p["edge"] and p["inliers"] == [44, 44]
    res = restated("degenerate_head_one_iteration")
    (p,) = res["pairs"]
    assert p["iterations"] == [1, 1] and p["inliers"] == [0, 0] and p["msd"] == [ref.DBL_MAX, ref.DBL_MAX] and not p["edge"]
    assert all(math.isnan(s) for s in p["prosac_s"]) and p["prosac_cost"] == [44 * scenes.THRESHOLD] * 2


def test_same_keys_yield_three_pairs_in_rank_order():
    _, cl, _, _, _ = named("same_keys")
    res = restated("same_keys")
    assert [(p["i"], p["j"], p["num_correspondences"]) for p in res["pairs"]] == [(0, 1, 90), (0, 2, 90), (1, 2, 90)]
    corr = ref.join(cl)
    for (i, j), (a, b) in corr.items():
        assert list(b) != sorted(b) and list(np.asarray(cl[j]["point_ids"])[b]) == sorted(cl[j]["point_ids"])
        la, lb = ref.join_literal(cl, i, j)
        assert (la == a).all() and (lb == b).all()
    assert all(p["edge"] for p in res["pairs"]) and res["in_component"].all()


def moved_pairs(base, res, pos):
    """the pairs of res that are the base's with the clusters at and after pos moved up by one"""
    out = []
    for p in base["pairs"]:
        out.append((p, pair(res, p["i"] + (p["i"] >= pos), p["j"] + (p["j"] >= pos))))
    return out


@pytest.mark.parametrize("kind", ["nothing", "images_only"])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_an_empty_cluster_changes_no_other_pair(kind, where):
    base = restated("empty_base")
    res = restated("empty_%s_%s" % (kind, where))
    pos = scenes.with_empty(kind, where)[2]
    for p, q in moved_pairs(base, res, pos):
        for key in ("num_correspondences", "inliers", "iterations", "msd", "weight", "edge"):
            assert p[key] == q[key]
    extra = [p for p in res["pairs"] if pos in (p["i"], p["j"])]
    assert len(extra) == (2 if kind == "images_only" else 0)
    assert all(p["num_correspondences"] == 0 and not p["edge"] for p in extra)
    assert not res["in_component"][pos] and res["in_component"].sum() == 3


def test_wide_ids_are_ordered_as_uint64():
    _, cl, _, _, _ = named("wide_ids")
    ids = [int(x) for x in cl[1]["point_ids"]]
    assert len(set(ids)) == 64 and len(set(x & 0xFFFFFFFF for x in ids)) == 1 and sum(x >= 1 << 63 for x in ids) == 32
    assert int(cl[0]["image_ids"].max()) == scenes.WIDE_IMAGE and int(cl[0]["obs"][:, 1].max()) == scenes.WIDE_IMAGE
    ii, jj = ref.join(cl)[(0, 1)]
    assert [ids[q] for q in jj] == sorted(ids)  # Python's unbounded integers: the unsigned order
    as_int64 = sorted(ids, key=lambda x: x - (1 << 64) if x >= 1 << 63 else x)
    assert as_int64 != sorted(ids)
    la, lb = ref.join_literal(cl, 0, 1)
    assert (la == ii).all() and (lb == jj).all()
    (p,) = restated("wide_ids")["pairs"]
    assert p["num_correspondences"] == 64 and p["edge"]


def test_five_clusters_graph():
    res = restated("graph_five_clusters")
    assert [(p["i"], p["j"], p["num_correspondences"]) for p in res["pairs"]] == [(1, 2, 30), (2, 3, 30), (3, 4, 30)]
    assert [p["edge"] for p in res["pairs"]] == [True, False, True]
    assert pair(res, 2, 3)["num_common_images"] == 2 and pair(res, 2, 3)["inliers"] == [10, 10]
    assert list(res["in_component"]) == [False, True, True, False, False]
    assert res["anchor"] == 2 and list(res["mst_parent"]) == [-1, 2, -1, -1, -1]
    for c in (0, 3, 4):
        assert res["s"][c] == 1.0 and (res["R"][c] == np.eye(3)).all() and (res["t"][c] == 0.0).all()
    assert res["s"][1] != 1.0
    assert sum(len(v[0]) for v in ref.join(named("graph_five_clusters")[1]).values()) == 120  # the 30 of (0, 1) among them


def test_tied_path_graph():
    res = restated("graph_tied_path")
    assert [(p["i"], p["j"]) for p in res["pairs"]] == [(0, 1), (1, 2), (1, 4), (2, 3)] and all(p["edge"] for p in res["pairs"])
    w = {(p["i"], p["j"]): np.float32(p["weight"]) for p in res["pairs"]}
    (e, f) = scenes.TIED_EDGES
    assert w[e] == w[f] and pair(res, *e)["weight"] == pair(res, *f)["weight"]  # the same data: the same bits
    assert res["in_component"].all() and res["anchor"] == 2 and list(res["mst_parent"]) == [1, 2, -1, 2, 1]
    assert res["mst"].index(e) < res["mst"].index(f)  # Kruskal took them in (i, j) order
