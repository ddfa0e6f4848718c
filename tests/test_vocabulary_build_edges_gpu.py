"""GPU: dsm_retrieval_quantize / dsm_retrieval_train_embedding at the edges tests/test_vocabulary_build_gpu.py leaves out,
against the numpy restatement (tests/vocabulary_build_ref.py; pinned to the reference's binary at these very cases by
tests/test_vocabulary_build_edges_cpu.py) and the recorded reference (tests/golden/vocab_quantize_v2.npz).

Everything is compared with == or as float bits.  The one relaxation is R.same_floats: a NaN equals a NaN.  The centre of a
cluster the last iteration emptied is 0 * inf; the sign and payload of that NaN are the processor's (x86 gives the negative
default NaN, the device the positive one), not the algorithm's, and no NaN can reach the words
(test_vocabulary_build_edges_cpu.py asserts that the returned centres are finite)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import vocabulary_build_ref as R
from tests import vocabulary_build_scenes as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_quantize_v2.npz")
OK, INVALID_ARGUMENT, OUT_OF_RANGE, NOT_READY = 0, 1, 4, 5
# workgroup_node_max: every clustered node by the whole chip / everything in workgroups / the default / between branching and
# 2 * branching - 2, where a node too large for a workgroup breaks a batch in the middle of the walk
SCHEDULES = ("chip", "default", "mid", "workgroup")


def workgroup_node_max(schedule, b):
    return {"chip": 1, "workgroup": 2 ** 31 - 1, "default": 0, "mid": b + b // 2}[schedule]


def case_of(name):
    if name in S.EDGE_CASES:
        d, nw, b, it, seed = S.EDGE_CASES[name]
        R.srand(seed)
        return d, nw, b, it, R.libc_rand
    d, nw, b, it, values = S.DRAW_CASES[name]
    return d, nw, b, it, S.cycled_draws(values)


@functools.lru_cache(maxsize=None)
def restated(name):
    """(words, centres, tree arrays, indices, the draws it took) of the restatement: computed once per case."""
    d, nw, b, it, rand = case_of(name)
    rec = R.Recorder(rand)
    words, centres, nodes, indices = R.quantize(d, nw, b, it, rand=rec)
    return words, centres, R.tree_arrays(nodes), indices.astype(np.int32), tuple(rec.draws)


def _params():
    out = []
    for name in sorted(S.EDGE_CASES) + sorted(S.DRAW_CASES):
        b = (S.EDGE_CASES.get(name) or S.DRAW_CASES[name])[2]
        out += [(name, s) for s in SCHEDULES if s != "mid" or b in (8, 17)]
    return out


@pytest.mark.parametrize("name,schedule", _params())
def test_quantize_equals_restatement(dsm, name, schedule):
    from dagsfm_amd import capi
    ref_words, ref_centres, ref_tree, ref_indices, draws = restated(name)
    d, nw, b, it, _ = case_of(name)
    if schedule == "mid":
        assert b < workgroup_node_max(schedule, b) <= 2 * b - 2
    o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it,
                                              workgroup_node_max=workgroup_node_max(schedule, b))
    replay = R.Replay(draws)
    words, centres = dsm.retrieval_quantize(d, o, rand=replay, with_centers=True)
    assert replay.pos == len(draws), "the device took %d draws, the reference %d" % (replay.pos, len(draws))
    parent, first, size, variance, radius, pivots, indices = dsm.vocabulary_tree()
    assert len(parent) == len(ref_tree[0])
    for got, ref, what in zip((parent, first, size), ref_tree[:3], ("parent", "first child", "size")):
        assert got.shape == ref.shape and (got == ref).all(), what
    for got, ref, what in zip((variance, radius, pivots), ref_tree[3:], ("variance bits", "radius bits", "pivot bits")):
        assert R.same_floats(got, ref), what
    assert (indices == ref_indices).all()
    assert words.shape == ref_words.shape and (words == ref_words).all()
    assert np.isfinite(centres).all() and (centres.view(np.uint32) == ref_centres.view(np.uint32)).all()
    assert (R.round_half_away(centres) == words).all()
    if name in S.EDGE_CASES:
        golden = np.load(GOLDEN)
        assert int(golden[name + "/count"]) == len(words) and (golden[name + "/words"] == words).all()


# ---------------------------------------------------------------------------------------------------- embedding
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def edge_scene():
    desc, words, projection, ids = S.embedding_edge_scene()
    return desc, words, projection, ids, R.train_embedding(desc, words, projection)


def test_embedding_ties_across_word_tiles(dsm):
    desc, words, projection, ids, (ref_thr, ref_has) = edge_scene()
    assert len(words) == 130 and len(desc) == 345
    assert (words[64] == words[63]).all() and (words[129] == words[2]).all()
    assert sorted(set(np.bincount(ids, minlength=130))) == [0, 4, 5, 6, 8, 300]
    assert {63, 65, 127, 128} <= set(ids) and 64 not in ids and 129 not in ids
    tied = desc[ids == 127].astype(np.int64)
    assert (((tied - words[127]) ** 2).sum(axis=1) == ((tied - words[128]) ** 2).sum(axis=1)).all()
    assert (R.nearest_words(desc, words) == ids).all()
    assert list(np.nonzero(ref_has)[0]) == sorted(w for w, s in S.EDGE_MEMBERS.items() if s >= 5)
    for given in (None, ids):
        thr, has = dsm.retrieval_train_embedding(desc, words, projection, given)
        assert (has == ref_has).all()
        assert (bits(thr) == bits(ref_thr)).all()
    assert not ref_thr[ref_has == 0].any() and ref_thr[ref_has == 1].any(axis=1).all()


def test_embedding_ids_are_the_index_ids(dsm):
    """Training and indexing assign the same word: the ids of dsm_retrieval_index for the scene as one image are the
    restatement's, and training with them gives the bits training with none gives."""
    desc, words, projection, ids, (ref_thr, _) = edge_scene()
    thr, _ = dsm.retrieval_train_embedding(desc, words, projection)
    dsm.set_images([desc])
    dsm.retrieval_set_vocabulary(words, projection, thr)
    index_ids = dsm.retrieval_debug_word_ids(0, len(desc), 1)[:, 0]
    assert (index_ids == R.nearest_words(desc, words)).all()
    thr2, _ = dsm.retrieval_train_embedding(desc, words, projection, index_ids)
    assert (bits(thr2) == bits(thr)).all() and (bits(thr) == bits(ref_thr)).all()


@pytest.mark.parametrize("num_words", [1, 3, 5])
def test_embedding_few_words(dsm, num_words):
    desc = S.uniform(41, 53)
    words = desc[:num_words].copy()
    projection = S.embedding_scene()[2]
    ref_thr, ref_has = R.train_embedding(desc, words, projection)
    assert ref_has.any()
    thr, has = dsm.retrieval_train_embedding(desc, words, projection)
    assert (has == ref_has).all() and (bits(thr) == bits(ref_thr)).all()


def test_embedding_more_rows_than_one_pass_of_the_projection(dsm):
    """4 * 4096 + 300 descriptors: the projection's grid of 4096 blocks of 4 rows wraps; thousands of members per word."""
    n = 4 * 4096 + 300
    desc = S.uniform(n, 54)
    words = S.uniform(5, 55)
    projection = S.embedding_scene()[2]
    ref_thr, ref_has = R.train_embedding(desc, words, projection)
    assert np.bincount(R.nearest_words(desc, words), minlength=5).min() > 1000
    thr, has = dsm.retrieval_train_embedding(desc, words, projection)
    assert (has == ref_has).all() and list(has) == [1] * 5 and (bits(thr) == bits(ref_thr)).all()


@pytest.mark.parametrize("members", [64, 63])
def test_embedding_median_overflows_as_the_reference(dsm, members):
    """(m1 + m2) is a float sum in the reference: past FLT_MAX it is inf for an even count, an odd count takes one element."""
    desc, words, projection = S.overflow_scene(members)
    ref_thr, ref_has = R.train_embedding(desc, words, projection)
    assert np.isinf(ref_thr[0, 0]) == (members % 2 == 0) and np.isfinite(ref_thr[0, 1:]).all() and ref_thr[0, 0] > 1e38
    thr, has = dsm.retrieval_train_embedding(desc, words, projection)
    assert list(has) == [1] == list(ref_has) and (bits(thr) == bits(ref_thr)).all()


# ---------------------------------------------------------------------------------------------------- host paths
@pytest.fixture()
def fresh():
    from dagsfm_amd import capi
    ctx = capi.Context(0, check=False)
    yield ctx
    ctx.close()


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_refused_options(dsm):
    from dagsfm_amd import capi
    d = S.CASES["smallest_64_16_4"][0]
    with pytest.raises(capi.DsmError, match="dsm error 1: dsm_retrieval_quantize: branching above 4096"):
        dsm.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=5000, branching=4097))
    with pytest.raises(capi.DsmError, match="dsm error 1: dsm_retrieval_quantize: fewer descriptors than num_visual_words"):
        dsm.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=65, branching=4))
    projection = np.zeros((64, 128), np.float32)
    ids = np.zeros(64, np.int32)
    ids[63] = -1
    with pytest.raises(capi.DsmError, match="dsm error 1: dsm_retrieval_train_embedding: a word id out of range"):
        dsm.retrieval_train_embedding(d, d[:4], projection, ids)


def test_not_ready_and_empty_input(fresh):
    from dagsfm_amd import capi
    with pytest.raises(capi.DsmError, match="dsm error 5: dsm_get_vocabulary_tree"):
        fresh.vocabulary_tree()
    with pytest.raises(capi.DsmError, match="dsm error 5: dsm_get_vocabulary_build_time"):
        fresh.vocabulary_build_time()
    L, h = fresh._L, fresh._h
    d = S.CASES["smallest_64_16_4"][0]
    projection = np.zeros((64, 128), np.float32)
    thr, has = np.full((4, 64), 7.0, np.float32), np.full(4, 7, np.uint8)
    # no word: refused, the outputs untouched
    assert L.dsm_retrieval_train_embedding(h, p(d), 64, p(d), 0, p(projection), None, p(thr), p(has)) == INVALID_ARGUMENT
    assert b"num_words out of range" in L.dsm_last_error(h) and (thr == 7.0).all() and (has == 7).all()
    with pytest.raises(capi.DsmError):
        fresh.vocabulary_build_time()
    # no descriptor: zeros, and a finished vocabulary call
    assert L.dsm_retrieval_train_embedding(h, None, 0, p(d), 4, p(projection), None, p(thr), p(has)) == OK
    assert not thr.any() and not has.any()
    times = fresh.vocabulary_build_time()
    assert times["embedding"] == 0.0
    with pytest.raises(capi.DsmError, match="dsm error 5"):
        fresh.vocabulary_tree()


def test_tree_hook_capacities_and_a_refused_call(fresh):
    from dagsfm_amd import capi
    L, h = fresh._L, fresh._h
    d, nw, b, it, _ = case_of("root_16")
    fresh.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it),
                             rand=R.Replay(restated("root_16")[4]))
    tree = fresh.vocabulary_tree()
    k, n = len(tree[0]), len(tree[6])
    assert (k, n) == (9, 16)
    nodes = (capi.VocabularyTreeNode * k)()
    pivots = np.zeros((k, 128), np.float32)
    indices = np.full(n, -1, np.int32)
    assert L.dsm_get_vocabulary_tree(h, None, ctypes.addressof(nodes), None, k - 1, None, 0) == OUT_OF_RANGE
    assert b"node capacity too small" in L.dsm_last_error(h)
    assert L.dsm_get_vocabulary_tree(h, None, None, p(pivots), k - 1, None, 0) == OUT_OF_RANGE
    assert L.dsm_get_vocabulary_tree(h, None, None, None, 0, p(indices), n - 1) == OUT_OF_RANGE
    assert b"indices capacity too small" in L.dsm_last_error(h)
    assert not pivots.any() and (indices == -1).all()
    assert L.dsm_get_vocabulary_tree(h, None, ctypes.addressof(nodes), p(pivots), k, p(indices), n) == OK
    assert (indices == tree[6]).all() and R.same_floats(pivots.view(np.uint32), tree[5])
    # a call refused before it starts leaves the last tree; one refused on the way ("does not end") leaves none
    with pytest.raises(capi.DsmError, match="dsm error 1"):
        fresh.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=17, branching=8))
    assert len(fresh.vocabulary_tree()[0]) == k
    same = np.repeat(d[:1], 8, axis=0)
    with pytest.raises(capi.DsmError, match="does not end"):
        fresh.retrieval_quantize(same, capi.default_vocabulary_build_options(num_visual_words=2, branching=2, num_iterations=0))
    with pytest.raises(capi.DsmError, match="dsm error 5: dsm_get_vocabulary_tree"):
        fresh.vocabulary_tree()


def test_memory_budget_refusals(fresh):
    from dagsfm_amd import capi
    name = "branching_17"
    ref_words, _, _, _, draws = restated(name)
    d, nw, b, it, _ = case_of(name)
    o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it)
    desc, words, projection, ids, (ref_thr, ref_has) = edge_scene()
    fresh.set_memory_budget(4096)  # below the descriptors alone
    replay = R.Replay(draws)
    with pytest.raises(capi.DsmError, match="dsm error 4: dsm_retrieval_quantize: .* exceed the memory budget"):
        fresh.retrieval_quantize(d, o, rand=replay)
    assert replay.pos == 0  # refused before a draw
    with pytest.raises(capi.DsmError, match="dsm error 4: dsm_retrieval_train_embedding: .* exceed the memory budget"):
        fresh.retrieval_train_embedding(desc, words, projection)
    fresh.set_memory_budget(0)
    got = fresh.retrieval_quantize(d, o, rand=replay)
    assert replay.pos == len(draws) and got.shape == ref_words.shape and (got == ref_words).all()
    thr, has = fresh.retrieval_train_embedding(desc, words, projection)
    assert (has == ref_has).all() and (bits(thr) == bits(ref_thr)).all()
