"""CPU side of the retrieval edge-case suite: every input of tests/test_retrieval_edges_gpu.py that claims to reach a path of
dagsfm_amd/csrc/retrieval.hip (a tie across half-waves / tiles / steps, a half-empty last workgroup, a run open at a chunk
boundary, a run ending exactly on one, Hamming distances on both sides of the cut, a second query batch) is shown here to
have that property -- from numpy, the oracle's word ids and the padding rule, without a device."""
import numpy as np
import pytest

from tests import oracle_lib, retrieval_emulation
from tests import retrieval_edge_cases as ec


def test_column_map_of_the_word_search():
    """Register r of half-wave `half` holds column 8*(r>>2) + 4*half + (r&3) of a 32-word tile: the 32 columns are covered
    once, and ec.word_half() is that map's inverse."""
    seen = {}
    for half in range(2):
        for r in range(16):
            seen[8 * (r >> 2) + 4 * half + (r & 3)] = half
    assert sorted(seen) == list(range(32))
    for step in range(4):
        for tile in range(2):
            for c in range(32):
                i = 64 * step + 32 * tile + c
                assert (ec.word_step(i), ec.word_tile(i), ec.word_half(i)) == (step, tile, seen[c])
    assert ec.word_half(5) != ec.word_half(5 ^ 4) and ec.word_tile(5) == ec.word_tile(5 ^ 4)
    # the tie the older test plants (words 4m+2 == 4m+3) never leaves a half-wave
    assert all(ec.word_half(4 * m + 2) == ec.word_half(4 * m + 3) for m in range(64))


def test_planted_ties_straddle_what_they_claim():
    used = []
    for name, (ids, spans) in ec.TIE_GROUPS.items():
        assert ec.group_spans(ids) >= spans and spans, name
        assert max(ids) < ec.TIE_WORDS
        used += ids
    for name, (a, b) in ec.EQUIDISTANT_PAIRS.items():
        used += [a, b]
    assert len(used) == len(set(used))  # no group overwrites another
    assert ec.group_spans(ec.TIE_GROUPS["halves"][0]) == {"half"}
    assert ec.group_spans(ec.TIE_GROUPS["tiles"][0]) == {"tile"}
    assert ec.group_spans(ec.TIE_GROUPS["steps"][0]) == {"step"}
    assert [len(ec.TIE_GROUPS[n][0]) for n in ("nine", "twelve", "twenty")] == [9, 12, 20]
    assert ec.group_spans(list(ec.EQUIDISTANT_PAIRS["halves"])) == {"half"}
    assert ec.group_spans(list(ec.EQUIDISTANT_PAIRS["tiles"])) == {"tile"}
    assert ec.group_spans(list(ec.EQUIDISTANT_PAIRS["steps"])) == {"step"}
    assert ec.TIE_WORDS % 64 != 0  # the last tile carries padding words


def test_tie_case_has_the_ties_and_both_references_agree():
    """In the tie case the k nearest words of the planted descriptors ARE the group, in ascending id (lists that overflow
    keep the 8 lowest ids), the numpy reference and the oracle's search give the same lists, and the rows end in a
    half-empty workgroup."""
    words, desc, owner = ec.tie_case()
    assert ec.last_workgroup_half_empty([len(desc)]) and ec.padded_rows([len(desc)]) == 768
    ref, dist = ec.exact_word_ids(desc, words, 8)
    orc = oracle_lib.RetrievalOracle(*ec.vocabulary_of(words))
    for k in range(1, 9):
        assert (orc.find_word_ids(desc, k) == ref[:, :k]).all(), k
    for row, name in enumerate(owner):
        if name.startswith("between_"):
            a, b = ec.EQUIDISTANT_PAIRS[name[len("between_"):]]
            assert dist[row, a] == dist[row, b] == 1 and list(ref[row, :2]) == [a, b]
        else:
            ids = ec.TIE_GROUPS[name][0]
            assert len(set(dist[row, ids])) == 1 and dist[row, ids[0]] == dist[row].min()
            assert list(ref[row, :min(8, len(ids))]) == sorted(ids)[:8]


def test_image_sets_cover_the_row_shapes():
    sizes = set()
    for total, counts in ec.IMAGE_SETS.items():
        assert ec.padded_rows(counts) == total
        assert ec.last_workgroup_half_empty(counts) == (total in (256, 768, 1280))
        sizes |= set(counts)
    assert sizes >= {0, 1, 255, 256, 257}
    assert sorted(ec.IMAGE_SETS) == [256, 512, 768, 1024, 1280]


@pytest.mark.parametrize("n_words", ec.VOCABULARY_SIZES)
def test_byte_vocabularies_numpy_equals_oracle(n_words):
    """The two word-id references agree on arbitrary bytes (all-0 / all-255 rows on both sides), with INVALID tails when the
    vocabulary has fewer than k words."""
    rng = np.random.default_rng(n_words)
    words = ec.byte_vocabulary(rng, n_words)
    desc = ec.byte_descriptors(rng, 40, words)
    assert (desc[0] == 0).all() and (desc[1] == 255).all()
    if n_words >= 3:
        assert (words == 0).all(1).any() and (words == 255).all(1).any()
    orc = oracle_lib.RetrievalOracle(*ec.vocabulary_of(words))
    ref, _ = ec.exact_word_ids(desc, words, 8)
    for k in (1, 8):
        assert (orc.find_word_ids(desc, k) == ref[:, :k]).all()
    assert ((ref == ec.INVALID).sum(1) == max(0, 8 - n_words)).all()


@pytest.mark.parametrize("n_words", [1, 2, 3])
def test_long_case_signatures_words_and_runs(n_words):
    """The construction of the long-file cases does what it is meant to: the oracle assigns every feature its intended word,
    retrieval_emulation.signatures gives exactly the planted bit masks, and the inverted files contain the chunk cases."""
    voc, descs, masks, wordof = ec.long_case(n_words)
    orc = oracle_lib.RetrievalOracle(*voc)
    ids = []
    for d, m, w in zip(descs, masks, wordof):
        assert 100 <= len(d) <= 700
        got = orc.find_word_ids(d, 1)[:, 0]
        assert (got == w).all()
        assert (retrieval_emulation.signatures(voc[1], voc[2][got], d) == m).all()
        near = orc.find_word_ids(d, 8)
        assert (np.sort(near[:, :n_words], axis=1) == np.arange(n_words)).all() and (near[:, n_words:] == ec.INVALID).all()
        ids.append(got)
    assert 4 <= len(descs) <= 8
    runs, entries = ec.inverted_files(ids, n_words)
    assert [sum(e - s for _, s, e in r) for r in runs] == [sum(row[w] for row in ec.LONG_CASES[n_words]["counts"]) for w in range(n_words)]
    assert max(e - s for r in runs for _, s, e in r) >= 128 and min(r[-1][2] for r in runs) >= 300
    props = ec.run_properties(runs)
    want = {3: {"open_over_one", "open_over_two", "ends_at_64_followed", "ends_at_128_followed", "mid_start_ends_on_boundary_followed",
                "ends_with_file_on_boundary", "whole_chunk_from_boundary"},
            2: {"open_over_one", "open_over_two", "mid_start_ends_on_boundary_followed", "ends_with_file_on_boundary",
                "whole_chunk_from_boundary", "ends_at_64_followed"},
            1: {"open_over_one", "open_over_two", "mid_start_ends_on_boundary_followed", "ends_with_file_on_boundary"}}[n_words]
    assert props >= want, want - props
    # a query feature of signature 0 exists in every file's word, and meets a carried run without a vote
    assert carried(runs, entries, masks)
    # Hamming distances 0, 23, 24, 25 and 64 from such a query feature occur in every file, in another image than the query's
    for w, (imgs, feats) in enumerate(entries):
        esig = np.array([masks[int(i)][int(f)] for i, f in zip(imgs, feats)], np.uint64)
        zero_images = set(int(i) for i, s in zip(imgs, esig) if s == 0)
        assert zero_images
        q = min(zero_images)
        h = ec.popcount64(esig[imgs != q])
        assert set(ec.POPCOUNTS) <= set(int(x) for x in h)
    if n_words > 1:  # IDF weights that are not zero: no word occurs in every image
        for w in range(n_words):
            assert len(set(int(i) for i in entries[w][0])) < len(descs)


def carried(runs, entries, masks):
    return ec.carried_run_without_votes(runs, entries, masks, 0)


def test_batch_case_needs_two_batches():
    assert ec.query_batch(6688) == 6688 and ec.query_batch(6689) < 6689
    b = ec.query_batch(ec.BATCH_IMAGES)
    assert b < ec.BATCH_IMAGES and 0 < ec.BATCH_IMAGES - b < 64  # two batches, the second short
    assert ec.BATCH_IMAGES * 256 * 128 < 256 << 20  # padded descriptors on the device
    assert b * ec.BATCH_IMAGES * 32 + 2 * b * ec.BATCH_IMAGES * 12 < 4 << 30  # accumulators, sort keys / values and their copies


def test_hamming_cut_is_24():
    assert ec.MAX_HAMMING == 24
    L = oracle_lib.load().lib
    import ctypes
    L.oracle_retrieval_hamming_weight.restype = ctypes.c_float
    L.oracle_retrieval_hamming_weight.argtypes = [ctypes.c_uint32]
    assert L.oracle_retrieval_hamming_weight(24) > 0 and L.oracle_retrieval_hamming_weight(25) == 0
