"""CPU-only: pins tests/vocabulary_build_ref.py to the reference at the edges tests/test_vocabulary_build_cpu.py leaves out
(vocabulary_build_scenes.EDGE_CASES: small, odd and large branchings, 0 / 2 / "until convergence" iterations, emptied clusters,
roots around 2 * branching - 1) -- to its own binary where oracle/_ref/libflann_ref.so exists and to the answers recorded from it
in tests/golden/vocab_quantize_v2.npz everywhere -- and asserts that every case still reaches the path it is there for
(the statistics hook of vocabulary_build_ref.cluster_node).  DRAW_CASES inject draws the binary cannot be fed: for them only the
reach is asserted here, the device is compared with the restatement in tests/test_vocabulary_build_edges_gpu.py."""
import functools
import hashlib
import os

import numpy as np
import pytest

from tests import flann_ref
from tests import vocabulary_build_ref as R
from tests import vocabulary_build_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_quantize_v2.npz")
VB_CHUNK = 256  # threads of a block of csrc/vocabulary_build.hip: a branching above it takes the second trip of its loops


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(words, centres, nodes, statistics) of the restatement after srand(seed), once per case."""
    d, nw, b, it, seed = S.EDGE_CASES[name]
    R.srand(seed)
    stats = []
    words, centres, nodes, _ = R.quantize(d, nw, b, it, stats=stats)
    return words, centres, nodes, stats


@functools.lru_cache(maxsize=None)
def restated_draws(name):
    d, nw, b, it, values = S.DRAW_CASES[name]
    stats = []
    words, centres, nodes, _ = R.quantize(d, nw, b, it, rand=S.cycled_draws(values), stats=stats)
    return words, centres, nodes, stats


def nan_nodes(nodes):
    return sum(bool(np.isnan(nd.pivot).any()) for nd in nodes)


def test_golden_holds_data_only_and_is_small(golden):
    assert os.path.getsize(GOLDEN) < 400 * 1000
    assert all(golden[k].dtype.kind in "iub" for k in golden.files)  # np.load refuses pickled objects by default as well
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(S.EDGE_CASES)
    for name, case in S.EDGE_CASES.items():
        assert (name + "/input" in golden.files) == (len(case[0]) <= 300), name


def test_rand_stream_is_the_recorded_one(golden):
    for name, (_, _, _, _, seed) in S.EDGE_CASES.items():
        R.srand(seed)
        assert [R.libc_rand() for _ in range(8)] == list(golden[name + "/rand8"]), name


@pytest.mark.parametrize("name", sorted(S.EDGE_CASES))
def test_restatement_equals_recorded_reference(golden, name):
    d, nw, b, it, seed = S.EDGE_CASES[name]
    assert [int(v) for v in golden[name + "/options"]] == [len(d), nw, b, it, seed]
    assert hashlib.sha256(d.tobytes()).digest() == golden[name + "/input_sha256"].tobytes()
    if name + "/input" in golden.files:
        assert (golden[name + "/input"] == d).all()
    words, centres, _, _ = restated(name)
    # The reference casts std::round(centre) to uint8_t, undefined for the NaN centre of an emptied cluster.  No such centre is
    # returned: a NaN variance loses every comparison of getMinVarianceClusters, so a node with such a child is never split.
    assert np.isfinite(centres).all()
    assert len(words) == int(golden[name + "/count"]) and (words == golden[name + "/words"]).all()
    assert len(words) == S.EDGE_EXPECTED_COUNT.get(name, nw)


@pytest.mark.parametrize("name", sorted(S.EDGE_CASES))
def test_restatement_equals_reference_binary(name):
    lib = flann_ref.load()
    if lib is None:
        pytest.skip("oracle/_ref/libflann_ref.so was not built (no reference on this machine)")
    d, nw, b, it, seed = S.EDGE_CASES[name]
    out = np.zeros((nw, 128), np.uint8)
    lib.flann_ref_seed(seed)
    count = lib.flann_ref_quantize(d.ctypes.data, len(d), nw, b, it, out.ctypes.data)
    words = restated(name)[0]
    assert count == len(words) and (out[:count] == words).all()


def test_statistics_hook_changes_nothing():
    d, nw, b, it, seed = S.EDGE_CASES["emptied_clusters"]
    R.srand(seed)
    rec = R.Recorder()
    words, centres, nodes, indices = R.quantize(d, nw, b, it, rand=rec)
    ref_words, ref_centres, ref_nodes, _ = restated("emptied_clusters")
    assert (words == ref_words).all() and R.same_floats(centres.view(np.uint32), ref_centres.view(np.uint32))
    assert all(R.same_floats(a, b_) if a.dtype == np.uint32 else (a == b_).all()
               for a, b_ in zip(R.tree_arrays(nodes), R.tree_arrays(ref_nodes)))
    assert len(rec.draws) == b * len(restated("emptied_clusters")[3])  # a clustered node draws branching values


# ------------------------------------------------------------------ every case reaches what it is there for
def schedule_forms(stats, b):
    """Clustered nodes by the form the default switch gives them: (whole chip, batched workgroups, single workgroups)."""
    wg_max = max(2 * b - 2, VB_CHUNK)
    chip = sum(s["size"] > wg_max for s in stats)
    batched = sum(s["size"] <= wg_max and s["size"] < 2 * b - 1 for s in stats)
    return chip, batched, len(stats) - chip - batched


@pytest.mark.parametrize("name", ["branching_17", "branching_31"])
def test_tile_remainder_cases_run_in_every_form(name):
    b = S.EDGE_CASES[name][2]
    assert b > 16 and b % 16 in (1, 15)
    chip, batched, single = schedule_forms(restated(name)[3], b)
    assert chip == 1 and batched > 0 and single > 0


def test_small_branchings_cluster_many_nodes():
    for name, b in (("branching_2", 2), ("branching_3", 3)):
        stats = restated(name)[3]
        assert S.EDGE_CASES[name][2] == b and len(stats) > 50
        _, batched, single = schedule_forms(stats, b)
        assert batched > 0 and single > 0


def test_large_branching_repairs_in_both_forms():
    """Three clustered nodes: the root, the identical rows in the whole-chip form, what the repair leaves of them batched; the
    repair runs where the branching exceeds the 256 threads of a block."""
    d, nw, b, it, _ = S.EDGE_CASES["branching_300"]
    _, _, nodes, stats = restated("branching_300")
    assert b > VB_CHUNK and len(nodes) == 901 and [s["node"] for s in stats][0] == 0 and len(stats) == 3
    wg_max = max(2 * b - 2, VB_CHUNK)
    chip = [s for s in stats[1:] if s["size"] > wg_max]
    batched = [s for s in stats[1:] if s["size"] < 2 * b - 1]
    assert len(chip) == 1 and len(batched) == 1 and chip[0]["size"] >= b and batched[0]["size"] >= b
    assert chip[0]["repairs"] > 0 and batched[0]["repairs"] > 0
    assert nan_nodes(nodes) == 0


def test_no_iteration_case_has_no_repair_and_ends():
    _, _, nodes, stats = restated("no_iteration")
    assert len(stats) == 76 and all(s["iterations"] == 0 and s["repairs"] == 0 for s in stats)
    assert any(s["size"] >= 2 * 8 - 1 for s in stats[1:]) and any(s["size"] < 2 * 8 - 1 for s in stats)


def test_until_convergence_runs_longer_and_converges():
    stats = restated("until_convergence")[3]
    assert max(s["iterations"] for s in stats) > 2 and all(s["converged"] for s in stats)
    two = restated("two_iterations")[3]
    assert max(s["iterations"] for s in two) == 2 and not all(s["converged"] for s in two)
    assert any(s["converged"] and s["iterations"] < 2 for s in two)  # ... and a node that stops before its limit


def test_emptied_clusters_case_reaches_nan_nodes():
    words, centres, nodes, stats = restated("emptied_clusters")
    assert len(nodes) == 753 and nan_nodes(nodes) == 498 == sum(s["nan_centres"] for s in stats)
    assert sum(bool(np.isnan(nd.variance)) for nd in nodes) == 498
    assert sum(s["repairs"] for s in stats) > 0 and len(words) == 40 and np.isfinite(centres).all()
    for name in S.EDGE_CASES:
        assert (nan_nodes(restated(name)[2]) > 0) == (name in S.EDGE_NAN_CASES), name


def test_root_sizes_straddle_the_batching_bound():
    b = 8
    sizes = sorted(len(S.EDGE_CASES[k][0]) for k in S.EDGE_CASES if k.startswith("root_"))
    assert sizes == [b, b + 1, 2 * b - 2, 2 * b - 1, 2 * b]
    for n in sizes:
        _, _, nodes, stats = restated("root_%d" % n)
        assert S.EDGE_CASES["root_%d" % n][2] == b and len(stats) == 1 and len(nodes) == b + 1


@pytest.mark.parametrize("name", sorted(S.DRAW_CASES))
def test_draw_cases_reach_their_paths(name):
    d, nw, b, it, values = S.DRAW_CASES[name]
    words, centres, nodes, stats = restated_draws(name)
    assert len(words) == S.DRAW_EXPECTED_COUNT.get(name, nw) and np.isfinite(centres).all()
    if values == (0,):
        # every seed is point 0, everything belongs to cluster 0: the first iteration repairs the other b - 1 one by one
        assert stats[0]["repairs"] == b - 1
    if name == "zero_one_iteration":
        assert nan_nodes(nodes) == 693
    else:
        assert nan_nodes(nodes) == 0
    if values == (S.RAND_MAX,):
        assert stats[0]["repairs"] == 0


def test_extreme_draws_select_the_ends():
    """Draw 0 takes index 0 every time; draw RAND_MAX the last point that still weighs something, at most n - 1."""
    closest = np.array([5, 0, 9, 4, 0, 0])
    assert R.select_prefix(R.rand_double(18.0, lambda: 0), closest) == R.select_walk(R.rand_double(18.0, lambda: 0), closest) == 0
    rv = R.rand_double(18.0, lambda: R.RAND_MAX)
    assert rv < 18.0 and R.select_prefix(rv, closest) == R.select_walk(rv, closest) == 3
    assert R.rand_int(700, lambda: R.RAND_MAX) == 699 and R.rand_int(700, lambda: 0) == 0


def test_same_floats():
    f = np.array([1.5, np.nan, -0.0, np.inf], np.float32)
    g = f.copy()
    g.view(np.uint32)[1] ^= 0x80000001  # another sign and payload: still a NaN
    assert R.same_floats(f.view(np.uint32), g.view(np.uint32))
    assert not R.same_floats(f.view(np.uint32), np.array([1.5, np.nan, 0.0, np.inf], np.float32).view(np.uint32))  # -0 is not 0
    assert not R.same_floats(f.view(np.uint32), np.array([1.5, 2.0, -0.0, np.inf], np.float32).view(np.uint32))
    assert not R.same_floats(f.view(np.uint32), f[:3].view(np.uint32))
