"""Device retrieval (dagsfm_amd/csrc/retrieval.hip) on the inputs of tests/retrieval_edge_cases.py: word search ties across
half-waves, tiles and steps, vocabulary and row shapes around the tile sizes, inverted files of hundreds of entries whose
runs cross and end on the 64-entry chunks, the Hamming cut, a second query batch, degenerate image sets and the error
returns.  References: exact int64 distances in numpy and RetrievalOracle.find_word_ids for the word ids, RetrievalOracle for
lists and scores, tests/retrieval_emulation.py for match tuples and IDF.  Every comparison is exact (ids, tuples, float bit
patterns); that each input reaches the path it is meant for is asserted by tests/test_retrieval_edges.py without a device.
With DSM_LIBRARY=check in the environment the whole module runs on the check build."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import oracle_lib, retrieval_emulation
from tests import retrieval_edge_cases as ec

pytestmark = pytest.mark.gpu

OK, INVALID_ARGUMENT, OUT_OF_RANGE, NOT_READY = 0, 1, 4, 5


def _use(kernel, monkeypatch):
    if kernel == "valu":  # the check build's form of the word search (the `dsm` fixture then hands out the check build)
        monkeypatch.setenv("DSM_VOCAB_ASSIGN_VALU", "1")


def _oracle(voc, descs):
    orc = oracle_lib.RetrievalOracle(*voc)
    for i, d in enumerate(descs):
        orc.add(i, d)
    orc.prepare()
    return orc


def _index(dsm, voc, descs):
    dsm.set_images(descs)
    dsm.retrieval_set_vocabulary(*voc)
    dsm.retrieval_index()


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _assert_lists(res, orc, descs, k, max_images, queries=None):
    """Image lists identical, scores bit-identical, for the given queries (all by default)."""
    assert len(res) == len(descs)
    for q in (range(len(descs)) if queries is None else queries):
        ids, sc = orc.query(descs[q], k, max_images, capacity=max(len(descs), 1) + 1)
        assert list(res[q][0]) == list(ids), (q, k, max_images, list(res[q][0])[:8], list(ids)[:8])
        assert (_bits(res[q][1]) == _bits(sc)).all(), (q, k, max_images)


def _assert_word_ids(dsm, words, descs):
    orc = oracle_lib.RetrievalOracle(*ec.vocabulary_of(words))
    for i, d in enumerate(descs):
        ref, _ = ec.exact_word_ids(d, words, 8)
        for k in range(1, 9):
            got = dsm.retrieval_debug_word_ids(i, len(d), k)
            assert got.shape == (len(d), k)
            assert (got == ref[:, :k]).all(), (i, k, np.argwhere(got != ref[:, :k])[:4])
            if len(words) <= 129 or k in (1, 8):
                assert (got == orc.find_word_ids(d, k)).all(), (i, k)


# ------------------------------------------------------------------------------------------------ word assignment
@pytest.mark.parametrize("kernel", ["mfma", "valu"])
@pytest.mark.parametrize("n_words", ec.VOCABULARY_SIZES)
def test_word_ids_on_vocabulary_and_row_shapes(dsm, n_words, kernel, monkeypatch):
    """Vocabularies of 1 .. 4097 words around the 32-word tile and the 64-word step (INVALID tails below 8 words, the padding
    of the last tile), arbitrary bytes with all-0 and all-255 rows on both sides, on all five image sets: padded totals of
    256 .. 1280 rows, so that the last workgroup is full and half empty, images of 0, 1, 255, 256 and 257 features.
    k = 1 .. 8 against numpy's exact distances and the oracle."""
    _use(kernel, monkeypatch)
    rng = np.random.default_rng(1000 + n_words)
    words = ec.byte_vocabulary(rng, n_words)
    dsm.set_images([np.zeros((1, 128), np.uint8)])
    dsm.retrieval_set_vocabulary(*ec.vocabulary_of(words))
    for total, counts in ec.IMAGE_SETS.items():
        descs = [ec.byte_descriptors(rng, n, words) for n in counts]
        assert ec.padded_rows(counts) == total
        dsm.set_images(descs)
        _assert_word_ids(dsm, words, descs)


@pytest.mark.parametrize("kernel", ["mfma", "valu"])
def test_word_ids_with_ties_across_halves_tiles_and_steps(dsm, kernel, monkeypatch):
    """Equal words in both half-waves of a tile, in both tiles of a step, in different steps, 9 / 12 / 20 copies of one word
    over all of these, and descriptors exactly between two different words: always ascending id."""
    _use(kernel, monkeypatch)
    words, desc, owner = ec.tie_case()
    dsm.set_images([desc])
    dsm.retrieval_set_vocabulary(*ec.vocabulary_of(words))
    _assert_word_ids(dsm, words, [desc])
    got = dsm.retrieval_debug_word_ids(0, len(desc), 8)
    for row, name in enumerate(owner):  # the planted lists themselves, spelled out
        if name.startswith("between_"):
            assert list(got[row, :2]) == list(ec.EQUIDISTANT_PAIRS[name[len("between_"):]])
        else:
            ids = sorted(ec.TIE_GROUPS[name][0])[:8]
            assert list(got[row, :len(ids)]) == ids, name
    # the same rows behind an empty image and a 255-feature image: other lanes, other workgroup
    descs = [desc[:0], desc[:255], desc]
    dsm.set_images(descs)
    _assert_word_ids(dsm, words, descs)


# ------------------------------------------------------------------------------------------------ long inverted files
def _planted_hamming_pairs(descs, masks, wordof, res, q):
    """For query image q: (feature, image, database feature, h) for its zero-signature features against every entry of the
    same word in a retrieved image whose signature has popcount 0, 23, 24, 25 or 64."""
    out = []
    for i in np.nonzero(masks[q] == 0)[0]:
        for img in res[q][0]:
            img = int(img)
            for f in np.nonzero(wordof[img] == wordof[q][i])[0]:
                h = int(ec.popcount64(masks[img][f]))
                if h in ec.POPCOUNTS:
                    out.append((int(i), img, int(f), h))
    return out


@pytest.mark.parametrize("n_words", [1, 2, 3])
def test_scores_and_matches_on_long_inverted_files(dsm, n_words):
    """Inverted files of 384 .. 580 entries with runs of up to 300: runs open over one and over two chunk boundaries, runs
    ending exactly at entry 64 / 128 / on a later boundary and followed by another image, a run ending with the file on a
    boundary, a carried run without votes before a run with votes; entries at Hamming distance 0, 23, 24, 25 and 64 from
    the query.  num_neighbors 1, 5, 8 and max_num_images 1, the image count and above it, for query and matches."""
    voc, descs, masks, wordof = ec.long_case(n_words)
    n = len(descs)
    orc = _oracle(voc, descs)
    _index(dsm, voc, descs)
    tuples = {k: retrieval_emulation.emulate(voc[0], voc[1], voc[2], descs, k, orc) for k in (1, 5, 8)}
    assert (_bits(dsm.retrieval_idf(n_words)) == _bits(tuples[1][1])).all()
    assert ((tuples[1][1] == 0).all()) == (n_words == 1)
    for k, max_images in [(1, n), (5, 1), (5, n), (5, n + 7), (8, n), (8, 1), (1, n + 7)]:
        res = dsm.retrieval_query(n, num_neighbors=k, max_num_images=max_images)
        _assert_lists(res, orc, descs, k, max_images)
        assert all(len(r[0]) == min(max_images, len(orc.query(descs[q], k, -1)[0])) for q, r in enumerate(res))
        offs, tup = dsm.retrieval_matches(res, num_neighbors=k, max_num_images=max_images)
        assert len(tup) == 0 or int((tup[:, 3] & 255).max()) <= ec.MAX_HAMMING
        for q in range(n):
            if (k, max_images) == (5, n) or q in (0, n - 1):  # (the emulation walks the files in Python: every query once)
                exp = tuples[k][0](q, res[q][0])
                got = tup[int(offs[q]):int(offs[q + 1])]
                assert got.shape == exp.shape and (got == exp).all(), (k, max_images, q)
        if max_images >= n:
            seen_h = set()
            for q in range(n):
                got = set((int(t[0]), int(t[1]), int(t[2]), int(t[3]) & 255) for t in tup[int(offs[q]):int(offs[q + 1])])
                for (i, img, f, h) in _planted_hamming_pairs(descs, masks, wordof, res, q):
                    assert ((i, img, f, h) in got) == (h <= ec.MAX_HAMMING), (q, i, img, f, h)
                    seen_h.add(h)
            assert seen_h == set(ec.POPCOUNTS)
    # the same bytes again
    res1 = dsm.retrieval_query(n, num_neighbors=5, max_num_images=n)
    res2 = dsm.retrieval_query(n, num_neighbors=5, max_num_images=n)
    for a, b in zip(res1, res2):
        assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all()


# ------------------------------------------------------------------------------------------------ query batches
def test_second_query_batch_equals_oracle(dsm):
    """6 700 images: dsm_retrieval_query scores 6 677 queries, then 23.  Lists and scores of every query against the oracle."""
    voc, descs = ec.batch_case()
    n = len(descs)
    batch = ec.query_batch(n)
    assert n == ec.BATCH_IMAGES and 0 < n - batch < 64
    _index(dsm, voc, descs)
    res = dsm.retrieval_query(n, num_neighbors=5, max_num_images=12)
    orc = _oracle(voc, descs)
    _assert_lists(res, orc, descs, 5, 12, queries=list(range(batch, n)) + list(range(0, batch)))
    assert sum(int(r[0][0]) == q for q, r in enumerate(res)) > 0.9 * n  # a discriminating set: images retrieve themselves
    dsm.set_images([descs[0]])  # release the large buffers' contents for the tests that follow


# ------------------------------------------------------------------------------------------------ degenerate sets
def _small_case(seed, n_words, counts):
    return ec.clustered_case(np.random.default_rng(seed), n_words, counts)


def _full_check(dsm, voc, descs, k=5, max_images=None):
    """index + query + matches + idf against the references; returns the raw results for byte comparisons."""
    n = len(descs)
    max_images = n if max_images is None else max_images
    orc = _oracle(voc, descs)
    _index(dsm, voc, descs)
    res = dsm.retrieval_query(n, num_neighbors=k, max_num_images=max_images)
    _assert_lists(res, orc, descs, k, max_images)
    offs, tup = dsm.retrieval_matches(res, num_neighbors=k, max_num_images=max_images)
    tuples, idf = retrieval_emulation.emulate(voc[0], voc[1], voc[2], descs, k, orc)
    got_idf = dsm.retrieval_idf(len(voc[0]))
    assert (_bits(got_idf) == _bits(idf)).all()
    for q in range(n):
        exp = tuples(q, res[q][0])
        got = tup[int(offs[q]):int(offs[q + 1])]
        assert got.shape == exp.shape and (got == exp).all(), q
    return res, offs, tup, got_idf


@pytest.mark.parametrize("where", ["front", "middle", "end", "several"])
def test_empty_images_inside_the_set(dsm, where):
    """An image without features takes no rows, is no database image (the IDF's image total counts the others only) and
    retrieves nothing."""
    counts = {"front": [0, 40, 33, 50], "middle": [40, 0, 33, 50], "end": [40, 33, 50, 0], "several": [0, 0, 40, 0, 33, 50, 0]}[where]
    voc, descs = _small_case(3, 24, counts)
    res, offs, tup, idf = _full_check(dsm, voc, descs)
    for q, c in enumerate(counts):
        assert (len(res[q][0]) == 0) == (c == 0)
        assert all(counts[int(d)] > 0 for d in res[q][0])
        if c == 0:
            assert offs[q] == offs[q + 1]


def test_all_images_empty(dsm):
    voc, descs = _small_case(4, 24, [0, 0, 0])
    _index(dsm, voc, descs)
    res = dsm.retrieval_query(3, num_neighbors=5, max_num_images=3)
    assert all(len(r[0]) == 0 for r in res)
    offs, tup = dsm.retrieval_matches(res, num_neighbors=5, max_num_images=3)
    assert list(offs) == [0, 0, 0, 0] and len(tup) == 0
    assert (dsm.retrieval_idf(24) == 0).all()


def test_word_in_every_image_scores_zero(dsm):
    """Word 0 occurs in every image (IDF exactly 0), words 1 and 2 discriminate.  An image that shares only word 0 with the
    query is listed with a score of exactly 0, behind the others."""
    rng = np.random.default_rng(8)
    cw = ec.centres(3)
    plan = [[20, 30, 0], [25, 30, 0], [30, 0, 35], [35, 0, 30], [70, 0, 0]]  # counts[image][word]
    descs = [np.array([ec.feature(w, ec.random_mask(rng, int(rng.integers(0, 12))), cw, rng) for w in range(3) for _ in range(row[w])], np.uint8)
             for row in plan]
    voc = ec.vocabulary_of(cw)
    for k in (1, 5, 8):
        res, offs, tup, idf = _full_check(dsm, voc, descs, k=k)
        assert idf[0] == 0 and idf[1] > 0 and idf[2] > 0
        assert all(4 in r[0] and r[1][list(r[0]).index(4)] == 0 for r in res)  # image 4 holds word 0 only: its constant is 0
        if k == 1:  # a feature meets its own word only
            assert len(res[0][0]) == 5 and set(int(d) for d in res[0][0][:2]) == {0, 1} and (res[0][1][2:] == 0).all()
            assert (res[4][1] == 0).all() and list(res[4][0]) == [0, 1, 2, 3, 4]  # equal scores from one item: ascending image


def test_one_word_vocabulary(dsm):
    """Every IDF is 0: all scores are exactly 0 and every query lists the images in the order its first feature meets them,
    which is the order of the single inverted file."""
    voc, descs = _small_case(5, 1, [30, 0, 70, 20, 90])
    for k in (1, 8):
        res, offs, tup, idf = _full_check(dsm, voc, descs, k=k)
        assert idf[0] == 0
        for q, r in enumerate(res):
            assert (_bits(r[1]) == 0).all() and (len(r[0]) > 0) == (len(descs[q]) > 0)
    res, _, _, _ = _full_check(dsm, voc, descs, k=5, max_images=2)
    assert all(len(r[0]) in (0, 2) for r in res)


@pytest.mark.parametrize("copies", [2, 3])
def test_identical_images(dsm, copies):
    """Byte-identical images score equal for every query (each of them is itself such a query): equal scores are listed in
    the order of their first contribution, and inside one item by ascending image."""
    voc, descs = _small_case(6, 40, [60, 45, 80, 52])
    same = [1, 3, 5][:copies]
    descs = [descs[0], descs[1], descs[2], descs[1], descs[3], descs[1]][:2 * copies]
    for k, max_images in [(5, None), (1, None), (8, 2)]:
        res, offs, tup, idf = _full_check(dsm, voc, descs, k=k, max_images=max_images)
        if max_images is None:
            for q, r in enumerate(res):
                pos = [list(r[0]).index(s) for s in same if s in r[0]]
                assert len(pos) in (0, copies)
                if pos:
                    assert pos == list(range(pos[0], pos[0] + copies))  # adjacent and in ascending image order
                    assert len(set(_bits(r[1])[pos])) == 1
            for s in same:
                assert list(res[s][0][:copies]) == same


def test_index_append_index_equals_one_upload(dsm):
    """dsm_retrieval_index, dsm_append_images, dsm_retrieval_index again: the same bytes as one upload of the whole set; a
    query between the append and the second index is refused."""
    voc, descs = _small_case(7, 64, [300, 0, 129, 256, 1, 257, 80])
    whole = _full_check(dsm, voc, descs)
    _index(dsm, voc, descs[:3])
    first = dsm.retrieval_query(3, 5, 3)
    _assert_lists(first, _oracle(voc, descs[:3]), descs[:3], 5, 3)
    dsm.append_images(descs[3:])
    with pytest.raises(capi.DsmError, match="dsm error %d" % NOT_READY):
        dsm.retrieval_query(len(descs), 5, len(descs))
    dsm.retrieval_index()
    n = len(descs)
    res = dsm.retrieval_query(n, 5, n)
    offs, tup = dsm.retrieval_matches(res, 5, n)
    for a, b in zip(res, whole[0]):
        assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all()
    assert (offs == whole[1]).all() and (tup == whole[2]).all()
    assert (_bits(dsm.retrieval_idf(64)) == _bits(whole[3])).all()
    # and all of it once more: repeated calls give the same bytes
    dsm.retrieval_index()
    res2 = dsm.retrieval_query(n, 5, n)
    offs2, tup2 = dsm.retrieval_matches(res2, 5, n)
    for a, b in zip(res, res2):
        assert (a[0] == b[0]).all() and (_bits(a[1]) == _bits(b[1])).all()
    assert (offs == offs2).all() and (tup == tup2).all()


# ------------------------------------------------------------------------------------------------ error returns
def test_error_returns_of_the_retrieval_entry_points():
    """Every retrieval entry point of include/dagsfm_mi355x.h with each documented precondition: the status code, and that the
    context still answers a correct query afterwards."""
    ctx = capi.Context(0)
    L, vp, u32, u64 = ctx._L, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
    L.dsm_retrieval_set_word_ids.argtypes = [vp, vp, u32, vp]
    L.dsm_retrieval_set_flann_index.argtypes = [vp, vp]
    L.dsm_retrieval_flann_search.argtypes = [vp, vp, u32, u32, vp, vp, vp]
    L.dsm_retrieval_matches.argtypes = [vp, u32, u32, vp, vp, vp]
    L.dsm_get_retrieval_matches.argtypes = [vp, vp, u64]
    L.dsm_get_retrieval_idf.argtypes = [vp, vp, u32]
    voc, descs = _small_case(9, 32, [40, 25, 0, 60])
    n, n_feat = len(descs), sum(len(d) for d in descs)
    orc = _oracle(voc, descs)
    cnt, idx, sc = np.zeros(n, np.uint32), np.zeros((n, n), np.uint32), np.zeros((n, n), np.float32)
    offs, wid, idf = np.zeros(n + 1, np.uint64), np.zeros((64, 8), np.int32), np.zeros(32, np.float32)
    h = lambda: ctx._h
    p = lambda a: a.ctypes.data

    def query(k=5, m=n):
        return L.dsm_retrieval_query(h(), k, m, p(cnt), p(idx), p(sc))

    def matches(k=5, m=n):
        return L.dsm_retrieval_matches(h(), k, m, p(cnt), p(idx), p(offs))

    def healthy():
        ctx.retrieval_set_word_ids(None, None)
        ctx.set_images(descs)
        ctx.retrieval_set_vocabulary(*voc)
        ctx.retrieval_index()
        _assert_lists(ctx.retrieval_query(n, 5, n), orc, descs, 5, n)

    try:
        ctx.set_images(descs)
        # before dsm_retrieval_set_vocabulary
        one = np.zeros(n_feat, np.int32)
        assert L.dsm_retrieval_index(h()) == NOT_READY
        assert L.dsm_retrieval_set_word_ids(h(), p(one), 1, p(one)) == NOT_READY
        assert L.dsm_retrieval_set_flann_index(h(), None) == NOT_READY
        assert L.dsm_retrieval_flann_search(h(), p(descs[0]), 1, 1, p(wid), None, None) == NOT_READY
        assert L.dsm_retrieval_debug_word_ids(h(), 0, 5, p(wid)) == NOT_READY
        assert query() == NOT_READY and matches() == NOT_READY
        bad = capi.Vocabulary(num_words=0, reserved=0, words=p(voc[0]), projection=p(voc[1]), thresholds=p(voc[2]))
        assert L.dsm_retrieval_set_vocabulary(h(), ctypes.byref(bad)) == INVALID_ARGUMENT
        bad = capi.Vocabulary(num_words=32, reserved=0, words=None, projection=p(voc[1]), thresholds=p(voc[2]))
        assert L.dsm_retrieval_set_vocabulary(h(), ctypes.byref(bad)) == INVALID_ARGUMENT
        assert L.dsm_retrieval_set_vocabulary(h(), None) == INVALID_ARGUMENT
        # with a vocabulary, before dsm_retrieval_index
        ctx.retrieval_set_vocabulary(*voc)
        assert query() == NOT_READY and matches() == NOT_READY
        assert L.dsm_get_retrieval_idf(h(), p(idf), 32) == NOT_READY
        assert L.dsm_retrieval_flann_search(h(), p(descs[0]), 1, 1, p(wid), None, None) == NOT_READY  # no FLANN index set
        assert L.dsm_retrieval_debug_word_ids(h(), n, 5, p(wid)) == OUT_OF_RANGE
        assert L.dsm_retrieval_debug_word_ids(h(), 0, 0, p(wid)) == OUT_OF_RANGE
        assert L.dsm_retrieval_debug_word_ids(h(), 0, 9, p(wid)) == OUT_OF_RANGE
        assert L.dsm_retrieval_debug_word_ids(h(), 0, 5, None) == INVALID_ARGUMENT
        healthy()
        # argument ranges of query and matches
        for k, m in [(0, n), (9, n), (5, 0)]:
            assert query(k, m) == INVALID_ARGUMENT and matches(k, m) == INVALID_ARGUMENT
        assert L.dsm_retrieval_query(h(), 5, n, None, p(idx), p(sc)) == INVALID_ARGUMENT
        assert L.dsm_retrieval_matches(h(), 5, n, p(cnt), p(idx), None) == INVALID_ARGUMENT
        healthy()
        # the two getters: capacity below the total
        assert query() == OK and matches() == OK and offs[n] > 1
        tup = np.zeros((int(offs[n]), 5), np.uint32)
        assert L.dsm_get_retrieval_matches(h(), p(tup), int(offs[n]) - 1) == OUT_OF_RANGE
        assert L.dsm_get_retrieval_idf(h(), p(idf), 31) == OUT_OF_RANGE
        assert L.dsm_get_retrieval_idf(h(), None, 32) == INVALID_ARGUMENT
        assert L.dsm_get_retrieval_matches(h(), p(tup), int(offs[n])) == OK and L.dsm_get_retrieval_idf(h(), p(idf), 32) == OK
        healthy()
        # the caller's word ids
        ids1 = np.concatenate([orc.find_word_ids(d, 1)[:, 0] for d in descs]).astype(np.int32)
        ids3 = np.concatenate([orc.find_word_ids(d, 3) for d in descs]).astype(np.int32)
        assert L.dsm_retrieval_set_word_ids(h(), p(ids1), 0, p(ids3)) == INVALID_ARGUMENT
        assert L.dsm_retrieval_set_word_ids(h(), p(ids1), 9, p(ids3)) == INVALID_ARGUMENT
        assert L.dsm_retrieval_set_word_ids(h(), p(ids1), 3, None) == INVALID_ARGUMENT
        assert L.dsm_retrieval_set_word_ids(h(), None, 3, p(ids3)) == INVALID_ARGUMENT
        for wrong in (32, -1):
            b1, b3 = ids1.copy(), ids3.copy()
            b1[7] = wrong
            assert L.dsm_retrieval_set_word_ids(h(), p(b1), 3, p(ids3)) == OUT_OF_RANGE
            b3[7, 2] = wrong
            assert L.dsm_retrieval_set_word_ids(h(), p(ids1), 3, p(b3)) == OUT_OF_RANGE
        healthy()
        assert L.dsm_retrieval_set_word_ids(h(), p(ids1), 3, p(ids3)) == OK
        assert query() == NOT_READY  # setting ids drops the index
        assert L.dsm_retrieval_index(h()) == OK
        assert query(5) == INVALID_ARGUMENT and matches(5) == INVALID_ARGUMENT  # k differs from the ids' k
        assert query(3) == OK
        _assert_lists([(idx[q, :cnt[q]], sc[q, :cnt[q]]) for q in range(n)], orc, descs, 3, n)  # exact ids in, exact lists out
        assert matches(3) == OK
        ctx.set_images(descs[::-1])  # other images, the same number of features: the ids are stale
        assert L.dsm_retrieval_index(h()) == NOT_READY
        assert query(3) == NOT_READY
        healthy()
    finally:
        ctx.close()
