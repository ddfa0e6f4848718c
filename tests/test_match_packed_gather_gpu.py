"""The packed gathered pass (csrc/match_kernels.hip, k1_best_rows<GATHER, FUSED>; csrc/capi.hip): pass 2 of the cross-check no
longer runs one workgroup per pair and 512 entries but packs the entries of a RUN -- consecutive pairs of the list with the same
column image -- into 512-entry blocks, whatever pairs the entries belong to.  What can go wrong is the bookkeeping: a pair
boundary inside a 32-row fragment, a wave or a block, the image base of an entry's row, runs of length one, empty pairs and
empty runs, a run that a chunk boundary cuts, an image that comes back in a later run.  Every case is held pair by pair to the CPU
oracle's match list, index for index; the last test also to the two-kernel form of the check build, which keeps the per-pair grid.

The entry count of a pair (its one-way matches) is planted: unrelated SIFT-like descriptors never pass the ratio test, a near
copy of a row of the column image does.  Some planted rows have a twin in the column image, so that pass 2 rejects their two
entries: the cross-check is not the identity."""
import numpy as np
import pytest

from dagsfm_amd import capi

pytestmark = pytest.mark.gpu

CASE1_COUNTS = (5, 27, 33, 1, 0, 129, 62, 300, 0)
CASE1_SIZES = (256, 300, 513, 257, 400, 640, 1024, 700, 256)
N_TWINS = 30  # rows 2t, 2t + 1 of a column image are near copies of each other, t < N_TWINS


def rand_sift(rng, n, scale=512.0):
    x = rng.random((n, 128), dtype=np.float32) ** 2
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.clip(np.rint(scale * x), 0, 255).astype(np.uint8)


def near(rng, x, k):
    """k bytes nudged by one: a neighbour at a small distance that grows with k."""
    y = x.astype(np.int32).copy()
    idx = rng.choice(128, k, replace=False)
    y[idx] += np.where(y[idx] < 200, 1, -1)
    return np.clip(y, 0, 255).astype(np.uint8)


def column_image(rng, n):
    a = rand_sift(rng, n)
    for t in range(N_TWINS):
        a[2 * t + 1] = near(rng, a[2 * t], 2)
    return a


def second_image(rng, a, n, count, cols=None):
    """n features, `count` one-way matches from the rows of `a`: near copies of `count` of its rows in distinct columns (`cols`:
    use these columns, in order).  A quarter of the count, while the twins last, comes from twin rows: one column, two entries,
    and pass 2 sees two almost equally near rows."""
    b = rand_sift(rng, n)
    n_twin = min(count // 4, N_TWINS)
    twins = rng.permutation(N_TWINS)[:n_twin]
    singles = 2 * N_TWINS + rng.permutation(len(a) - 2 * N_TWINS)[:count - 2 * n_twin]
    rows = [2 * int(t) for t in twins] + [int(r) for r in singles]
    if cols is None:
        cols = rng.permutation(n)
    assert len(rows) <= len(cols)
    for r, c in zip(rows, cols):
        b[int(c)] = near(rng, a[r], 6)
    return b


class Case:
    """Images, a pair list, and the oracle's match lists (computed once per distinct pair and kept)."""

    def __init__(self, descs, pairs):
        self.descs = descs
        self.pairs = np.array(pairs, dtype=np.uint32).reshape(-1, 2)
        self._ref = {}

    def ref(self, oracle, i, j, cross):
        key = (int(i), int(j), bool(cross))
        if key not in self._ref:
            self._ref[key] = oracle.match_sift_features_cpu(self.descs[key[0]], self.descs[key[1]], 0.8, 0.7, bool(cross))
        return self._ref[key]

    def run(self, dsm, pairs=None, cross=1):
        pairs = self.pairs if pairs is None else np.array(pairs, dtype=np.uint32).reshape(-1, 2)
        dsm.set_images(self.descs)
        dsm.match_pairs(pairs, capi.default_match_options(cross_check=cross))
        offs, m = dsm.matches()
        return offs.copy(), m.copy()

    def check(self, oracle, offs, m, pairs=None, cross=1):
        pairs = self.pairs if pairs is None else pairs
        assert len(offs) == len(pairs) + 1
        for k, (i, j) in enumerate(pairs):
            got = m[int(offs[k]):int(offs[k + 1])]
            ref = self.ref(oracle, i, j, cross)
            assert got.shape == ref.shape, (k, i, j, got.shape, ref.shape)
            assert (got == ref).all(), (k, i, j)


@pytest.fixture(scope="module")
def case1():
    """One column image (768 features) against nine second images: ONE run whose pair boundaries fall at entries 5, 32, 65, 66,
    66, 195, 257, 557 -- three pairs inside the first fragment, a boundary on the 32-row edge, one inside the second wave
    (195), and the 512-entry block edge in the middle of the pair that holds entries 257 .. 556."""
    rng = np.random.default_rng(20261019)
    a = column_image(rng, 768)
    descs = [a] + [second_image(rng, a, n, c) for n, c in zip(CASE1_SIZES, CASE1_COUNTS)]
    return Case(descs, [(0, k) for k in range(1, 10)])


@pytest.fixture(scope="module")
def case2():
    """Two neighbouring pairs of a run whose 40 entries carry the same i2 (the same 30 columns: ten hold a twin's two entries)
    while the two second images hold different descriptors there: near copies of different rows of the column image."""
    rng = np.random.default_rng(77)
    a = column_image(rng, 512)
    cols = rng.permutation(300)[:60]
    b1 = second_image(rng, a, 300, 40, cols)
    b2 = second_image(rng, a, 420, 40, cols)
    return Case([a, b1, b2], [(0, 1), (0, 2)])


@pytest.fixture(scope="module")
def case3():
    """Three column images (0 - 2), nine planted second images (3 - 11: 3 - 6 for image 0, 7 for image 1, 8 - 11 for image 2)
    and three second images without a match (12 - 14)."""
    rng = np.random.default_rng(303)
    cols = [column_image(rng, n) for n in (256, 700, 385)]
    owner = (0, 0, 0, 0, 1, 2, 2, 2, 2)
    counts = (40, 3, 200, 64, 31, 1, 130, 97, 256)
    sizes = (256, 300, 513, 1024, 257, 640, 300, 256, 700)
    descs = cols + [second_image(rng, cols[o], n, c) for o, n, c in zip(owner, sizes, counts)]
    descs += [rand_sift(rng, n) for n in (256, 333, 512)]
    return Case(descs, [])


CASE3_LISTS = {
    # the column image changes every pair
    "runs_of_one": [(0, 3), (1, 7), (2, 8), (0, 4), (2, 9), (1, 7), (0, 5)],
    # a run of one pair between two long runs
    "one_between_long": [(0, 3), (0, 4), (0, 5), (0, 6), (1, 7), (2, 8), (2, 9), (2, 10), (2, 11)],
    # the same pair twice in a row
    "same_pair_twice": [(0, 5), (0, 5), (2, 11), (2, 11)],
    # a pair with zero entries first in its run, last in its run, and alone in its run
    "zero_entry_pairs": [(0, 12), (0, 3), (0, 5), (1, 13), (2, 10), (2, 14)],
    # every pair has zero entries: no block, no launch
    "no_entries_at_all": [(0, 12), (0, 13), (1, 14), (2, 12)],
    # unsorted: a column image returns after another one, two separate runs
    "image_returns": [(0, 3), (0, 4), (2, 8), (2, 9), (0, 5), (0, 6)],
}


def test_case1_entry_counts(case1, oracle, dsm):
    """The construction, through the one-way result: the planted counts are the pairs' entry counts, on the oracle and on the
    device, so the boundaries of the docstring above are where the test says they are."""
    want = list(CASE1_COUNTS)
    assert [len(case1.ref(oracle, 0, k, False)) for k in range(1, 10)] == want
    assert np.cumsum(want)[:-1].tolist() == [5, 32, 65, 66, 66, 195, 257, 557]
    offs, m = case1.run(dsm, cross=0)
    assert np.diff(offs.astype(np.int64)).tolist() == want
    case1.check(oracle, offs, m, cross=0)


def test_run_boundaries_inside_fragment_wave_and_block(case1, oracle, dsm):
    offs, m = case1.run(dsm)
    case1.check(oracle, offs, m)
    n = np.diff(offs.astype(np.int64))
    assert 0 < n[7] < 300 and n[4] == 0 and n[8] == 0  # the twins: pass 2 rejects entries, the cross-check is not the identity


def test_same_row_index_different_image(case2, oracle, dsm):
    one = [case2.ref(oracle, 0, k, False) for k in (1, 2)]
    assert len(one[0]) == len(one[1]) == 40 and sorted(one[0][:, 1]) == sorted(one[1][:, 1])  # the same columns i2 ...
    assert set(one[0][:, 0]) != set(one[1][:, 0])                                            # ... from different rows
    offs, m = case2.run(dsm)
    case2.check(oracle, offs, m)
    assert int(offs[1]) > 20 and int(offs[2] - offs[1]) > 20


@pytest.mark.parametrize("name", sorted(CASE3_LISTS))
def test_list_shapes(case3, oracle, dsm, name):
    pairs = np.array(CASE3_LISTS[name], dtype=np.uint32)
    offs, m = case3.run(dsm, pairs)
    case3.check(oracle, offs, m, pairs)
    if name == "no_entries_at_all":
        assert int(offs[-1]) == 0
        assert all(len(case3.ref(oracle, i, j, False)) == 0 for i, j in pairs)
    else:
        assert int(offs[-1]) > 0


@pytest.mark.parametrize("chunk_pairs", [5, 3])
def test_chunk_boundary_inside_a_run(case1, oracle, dsm, monkeypatch, chunk_pairs):
    """A pair of case 1 costs the chunk planner 768 rows: 5 pairs per chunk cut the run in two (5 + 4), 3 in three."""
    offs0, m0 = case1.run(dsm)
    monkeypatch.setenv("DSM_MATCH_CHUNK_ROWS", str(768 * chunk_pairs))
    offs1, m1 = case1.run(dsm)
    assert (offs0 == offs1).all() and (m0 == m1).all() and len(m0) > 300
    case1.check(oracle, offs1, m1)


def test_packed_pass_equals_two_kernel_form(case1, case2, case3, oracle, dsm, monkeypatch):
    """DSM_K1_RESOLVE_KERNEL=1 (check build): the unfused pass 2 on the (pair, row block) grid + k1_resolve_index gives the
    same offsets and matches as the product's packed pass."""
    jobs = [(case1, case1.pairs), (case2, case2.pairs)] + [(case3, np.array(CASE3_LISTS[n], dtype=np.uint32)) for n in sorted(CASE3_LISTS)]
    product = [c.run(dsm, p) for c, p in jobs]
    monkeypatch.setenv("DSM_K1_RESOLVE_KERNEL", "1")  # a check-build schedule: from here on `dsm` is the check library's context
    for (c, p), (offs0, m0) in zip(jobs, product):
        offs1, m1 = c.run(dsm, p)
        assert (offs0 == offs1).all() and (m0 == m1).all()
        c.check(oracle, offs1, m1, p)
