"""GPU: dsm_retrieval_quantize / dsm_retrieval_train_embedding against the numpy restatement of the reference
(tests/vocabulary_build_ref.py, pinned to the reference's own binary by tests/test_vocabulary_build_cpu.py) with == on
everything the test hook returns, and against the recorded answers of the reference (tests/golden/vocab_quantize_v1.npz)."""
import functools
import os

import numpy as np
import pytest

from tests import vocabulary_build_ref as R
from tests import vocabulary_build_scenes as S

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_quantize_v1.npz")
# workgroup_node_max: every clustered node by the whole chip / everything in workgroups / the default
SCHEDULES = {"chip": 1, "workgroup": 2 ** 31 - 1, "default": 0}


@functools.lru_cache(maxsize=None)
def restated(name):
    """(words, tree arrays, indices, the draws it took) of the restatement after srand(seed): computed once per case."""
    d, nw, b, it, seed = S.CASES[name]
    R.srand(seed)
    rec = R.Recorder()
    words, _, nodes, indices = R.quantize(d, nw, b, it, rand=rec)
    return words, R.tree_arrays(nodes), indices.astype(np.int32), tuple(rec.draws)


def seed_process_rand(dsm, seed):
    """srand(seed) for a call that draws from the process's rand() (rand_fn NULL).  Anything else in the process that calls
    rand() between the seeding and the draws shifts the stream -- a process's first HIP calls can --, so one small call in
    each form runs first."""
    from dagsfm_amd import capi
    d = S.CASES["smallest_64_16_4"][0]
    for wg in SCHEDULES.values():
        dsm.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=16, branching=4, workgroup_node_max=wg))
    R.srand(seed)


def device(dsm, name, schedule, rand):
    from dagsfm_amd import capi
    d, nw, b, it, _ = S.CASES[name]
    o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it, workgroup_node_max=SCHEDULES[schedule])
    words, centers = dsm.retrieval_quantize(d, o, rand=rand, with_centers=True)
    return words, centers, dsm.vocabulary_tree()


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
@pytest.mark.parametrize("name", sorted(S.CASES))
def test_quantize_equals_restatement(dsm, name, schedule):
    ref_words, ref_tree, ref_indices, draws = restated(name)
    replay = R.Replay(draws)
    words, centers, tree = device(dsm, name, schedule, replay)
    assert replay.pos == len(draws), "the device took %d draws, the reference %d" % (replay.pos, len(draws))
    parent, first, size, variance, radius, pivots, indices = tree
    assert len(parent) == len(ref_tree[0])
    for got, ref, what in zip((parent, first, size, variance, radius, pivots), ref_tree,
                              ("parent", "first child", "size", "variance bits", "radius bits", "pivot bits")):
        assert got.shape == ref.shape and (got == ref).all(), what
    assert (indices == ref_indices).all()
    assert words.shape == ref_words.shape and (words == ref_words).all()
    assert (R.round_half_away(centers) == words).all()
    golden = np.load(GOLDEN)
    assert int(golden[name + "/count"]) == len(words) and (golden[name + "/words"] == words).all()


@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_large_root_equals_recorded_reference(dsm, schedule):
    """More chunks than the threads that scan them (vocabulary_build_scenes.large_case): the reference's recorded words."""
    import hashlib
    from dagsfm_amd import capi
    golden = np.load(GOLDEN)
    d, nw, b, it, seed = S.large_case()
    assert hashlib.sha256(d.tobytes()).digest() == golden[S.LARGE + "/input_sha256"].tobytes()
    seed_process_rand(dsm, seed)
    o = capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it, workgroup_node_max=SCHEDULES[schedule])
    words = dsm.retrieval_quantize(d, o)
    assert len(words) == int(golden[S.LARGE + "/count"]) and (words == golden[S.LARGE + "/words"]).all()
    _, _, size, _, _, _, indices = dsm.vocabulary_tree()
    assert size[0] == len(d) and (np.sort(indices) == np.arange(len(d))).all()


def test_null_rand_is_the_process_rand(dsm):
    name = "batch_edges_1000_300_8"
    ref_words = restated(name)[0]
    seed_process_rand(dsm, S.CASES[name][4])
    words, _, _ = device(dsm, name, "default", None)
    assert words.shape == ref_words.shape and (words == ref_words).all()


def test_seeds(dsm):
    name = "modes_3000_64_4"
    out = []
    for seed in (2, 2, 3):
        seed_process_rand(dsm, seed)
        out.append(device(dsm, name, "default", None)[0])
    assert out[0].shape == out[1].shape and (out[0] == out[1]).all()
    assert out[0].shape != out[2].shape or (out[0] != out[2]).any()


def test_refusals(dsm):
    from dagsfm_amd import capi
    d = S.CASES["smallest_64_16_4"][0]
    for kw, n in (({"num_visual_words": 3, "branching": 4}, 64), ({"num_visual_words": 65, "branching": 4}, 64),
                  ({"num_visual_words": 16, "branching": 1}, 64), ({"num_visual_words": 16, "branching": 4, "workgroup_node_max": -1}, 64)):
        with pytest.raises(capi.DsmError, match="dsm error 1: dsm_retrieval_quantize"):
            dsm.retrieval_quantize(d[:n], capi.default_vocabulary_build_options(**kw))
    # identical points without an iteration: no repair splits them, the reference recurses without end
    same = np.repeat(d[:1], 8, axis=0)
    for wg in SCHEDULES.values():
        with pytest.raises(capi.DsmError, match="does not end"):
            dsm.retrieval_quantize(same, capi.default_vocabulary_build_options(num_visual_words=2, branching=2, num_iterations=0,
                                                                               workgroup_node_max=wg))
    with pytest.raises(ValueError, match="does not end"):
        R.quantize(same, 2, 2, 0, rand=lambda: 5)
    with pytest.raises(capi.DsmError, match="word id out of range"):
        dsm.retrieval_train_embedding(d, d[:4], np.zeros((64, 128), np.float32), np.full(64, 4, np.int32))


# ---------------------------------------------------------------------------------------------------- embedding
def test_embedding_equals_restatement(dsm):
    desc, words, projection, ids = S.embedding_scene()
    assert sorted(np.bincount(ids, minlength=len(words)))[:6] == [0, 1, 4, 5, 6, 7]
    ref_thr, ref_has = R.train_embedding(desc, words, projection)
    assert (R.nearest_words(desc, words) == ids).all()
    thr, has = dsm.retrieval_train_embedding(desc, words, projection)
    assert (has == ref_has).all() and list(has) == [0, 0, 0, 1, 1, 1, 1, 1]
    assert (thr.view(np.uint32) == ref_thr.view(np.uint32)).all()
    assert not thr[:3].any() and thr[3:].any(axis=1).all()
    # the caller's ids: the same ids give the same answer, other ids another
    thr2, has2 = dsm.retrieval_train_embedding(desc, words, projection, ids)
    assert (thr2.view(np.uint32) == thr.view(np.uint32)).all() and (has2 == has).all()
    other = (ids % 2).astype(np.int32)
    thr3, has3 = dsm.retrieval_train_embedding(desc, words, projection, other)
    ref3 = R.train_embedding(desc, words, projection, other)
    assert (thr3.view(np.uint32) == ref3[0].view(np.uint32)).all() and (has3 == ref3[1]).all() and list(has3[:3]) == [1, 1, 0]


def test_embedding_tied_column(dsm):
    desc, words, projection, ids = S.embedding_scene()
    projection = projection.copy()
    projection[7] = 0.0            # a column of equal values (all zero) ...
    projection[9] = 0.0
    projection[9, 0] = 1.0         # ... and one that takes few distinct values (the first byte)
    ref_thr, ref_has = R.train_embedding(desc, words, projection, ids)
    thr, has = dsm.retrieval_train_embedding(desc, words, projection, ids)
    assert (thr.view(np.uint32) == ref_thr.view(np.uint32)).all() and (has == ref_has).all()
    assert not thr[:, 7].any()


def test_build_vocabulary_round_trip(dsm):
    """build_vocabulary -> set_vocabulary -> index -> query on a 12-image scene: every image retrieves itself first."""
    from dagsfm_amd import capi, synthetic
    scene = synthetic.Scene(12, 256, seed=3)
    descs = [scene.image(i)[0] for i in range(12)]
    train = np.concatenate(descs)
    projection = np.linalg.qr(np.random.default_rng(5).normal(size=(128, 128)))[0][:64].astype(np.float32)
    R.srand(1)
    o = capi.default_vocabulary_build_options(num_visual_words=64, branching=8, num_iterations=11)
    words, proj, thr = dsm.build_vocabulary(train, projection, o)
    assert words.shape == (64, 128) and thr.shape == (64, 64)
    dsm.set_images(descs)
    dsm.retrieval_set_vocabulary(words, proj, thr)
    dsm.retrieval_index()
    res = dsm.retrieval_query(12, num_neighbors=5, max_num_images=12)
    for q, (idx, scores) in enumerate(res):
        assert idx[0] == q, (q, idx[:3], scores[:3])
    times = dsm.vocabulary_build_time()
    assert set(times) == set(capi.VOCABULARY_BUILD_STAGES) and all(v >= 0.0 for v in times.values())
