"""The resolve of the flagged rows in the tail of k1_best_rows (csrc/match_kernels.hip): the wave that owns a 32-row fragment
stages it in its quarter of the B-tile LDS, ballots the rows that passed the pre-test and resolves them four per trip.  The
shapes are the smallest at which that tail can go wrong -- every row flagged, none, flag counts around the trip size, the
`both sets` code, the runner-up inside the winning set through the gathered pass, a ragged pair list in one launch -- and every
case is held to exact equality with the CPU oracle; the last one to the two-kernel form of the check build as well."""
import numpy as np
import pytest

from dagsfm_amd import capi

pytestmark = pytest.mark.gpu


def check_equal(m_gpu, m_cpu):
    assert m_gpu.shape == m_cpu.shape, (m_gpu.shape, m_cpu.shape)
    assert (m_gpu == m_cpu).all()


def rand_sift(rng, n, scale=512.0):
    """SIFT-like descriptors: 128 x U(0,1)^2, L2-normalised, x scale, rounded, saturated to u8.  scale = 500 keeps a
    descriptor's dot product with its own copy below 2^18, so that an exact copy is at a distance > 0 (acos does not
    saturate) and max_ratio = 2.0 accepts a row whose best column has a duplicate."""
    x = rng.random((n, 128), dtype=np.float32) ** 2
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return np.clip(np.rint(scale * x), 0, 255).astype(np.uint8)


def near(rng, x, k):
    """k bytes nudged by one: a neighbour at a small distance that grows with k."""
    y = x.astype(np.int32).copy()
    idx = rng.choice(128, k, replace=False)
    y[idx] += np.where(y[idx] < 200, 1, -1)
    return np.clip(y, 0, 255).astype(np.uint8)


@pytest.mark.parametrize("n1,n2", [(130, 96), (513, 70), (33, 300)])
@pytest.mark.parametrize("cross", [0, 1])
def test_every_row_flagged(dsm, oracle, n1, n2, cross):
    """max_ratio 2.0 / max_distance 3.0 reject nothing: all 32 rows of every fragment are flagged (eight trips) and every
    fragment is staged.  (130, 96): two ragged fragments of wave 1, waves 2 - 3 without rows; (513, 70): a second row block
    that holds one row; (33, 300): a fragment with a single row."""
    rng = np.random.default_rng(100 * n1 + n2)
    d1 = rand_sift(rng, n1)
    d2 = rand_sift(rng, n2)
    o = capi.default_match_options(max_ratio=2.0, max_distance=3.0, cross_check=cross)
    ref = oracle.match_sift_features_cpu(d1, d2, 2.0, 3.0, bool(cross))
    if not cross:
        assert len(ref) == n1  # the construction: every row of image 1 is matched, so every row was flagged
    check_equal(dsm.match_sift_features(d1, d2, o), ref)


def test_no_row_flagged(dsm, oracle):
    """All-zero rows have dot 0 with everything (best_i2 stays -1, sift.cc:136): the ballots are empty, nothing is staged or
    resolved, the result is empty."""
    rng = np.random.default_rng(5)
    d1 = np.zeros((130, 128), np.uint8)
    d2 = rand_sift(rng, 96)
    for cross in (0, 1):
        o = capi.default_match_options(max_distance=0.01, cross_check=cross)
        m = dsm.match_sift_features(d1, d2, o)
        assert len(m) == 0
        check_equal(m, oracle.match_sift_features_cpu(d1, d2, 0.8, 0.01, bool(cross)))


@pytest.mark.parametrize("k", [0, 1, 3, 4, 5, 31, 32])
def test_flag_counts_around_the_trip_size(dsm, oracle, k):
    """Exactly k rows of ONE 32-row fragment are flagged: they have a single copy among the columns.  Every other row has two
    identical copies in different tiles, so its second best equals its best and the pre-test rejects it (sift.cc:151-155).
    With max_ratio 2.0 the duplicates pass, and resolve to the lower column."""
    rng = np.random.default_rng(700 + k)
    n1, n2 = 128, 320
    d1 = rand_sift(rng, n1, 500.0)
    d2 = rand_sift(rng, n2, 500.0)
    single = set((64 + rng.permutation(32)[:k]).tolist())  # rows of the fragment 64 .. 95
    for i in range(n1):
        d2[i] = d1[i]                  # tiles 0 - 3
        if i not in single:
            d2[160 + i] = d1[i]        # tiles 5 - 8
    ref = oracle.match_sift_features_cpu(d1, d2, 0.8, 0.7, False)
    assert ref[:, 0].tolist() == sorted(single) and (ref[:, 0] == ref[:, 1]).all()  # the construction does what it says
    for cross in (0, 1):
        check_equal(dsm.match_sift_features(d1, d2, capi.default_match_options(cross_check=cross)),
                    oracle.match_sift_features_cpu(d1, d2, 0.8, 0.7, bool(cross)))
        ref2 = oracle.match_sift_features_cpu(d1, d2, 2.0, 0.7, bool(cross))
        assert len(ref2) == n1 and (ref2[:, 0] == ref2[:, 1]).all()  # every row, at the lower of its columns
        check_equal(dsm.match_sift_features(d1, d2, capi.default_match_options(max_ratio=2.0, cross_check=cross)), ref2)


@pytest.mark.parametrize("n2", [65, 257])
def test_best_value_in_both_column_sets(dsm, oracle, n2):
    """The best column duplicated at c and c ^ 4 -- the two half-waves' sets of one tile reach the same best value in the same
    tile (set code 2, 32 columns to resolve) -- in tile 0 and in the last tile that can hold both columns of an image padded
    to 256 / 512 columns; one more row has its best in the image's very last column, alone in a tile of padding."""
    rng = np.random.default_rng(n2)
    n1 = 40
    d1 = rand_sift(rng, n1, 500.0)
    d2 = rand_sift(rng, n2, 500.0)
    hi = max(c for c in range(n2) if c & 4)
    d2[3] = d2[7] = d1[5]
    d2[hi ^ 4] = d2[hi] = d1[17]
    d2[n2 - 1] = d1[33]
    for cross in (0, 1):
        ref = oracle.match_sift_features_cpu(d1, d2, 2.0, 0.7, bool(cross))
        got = {int(a): int(b) for a, b in ref}
        assert got[5] == 3 and got[17] == (hi ^ 4) and got[33] == n2 - 1  # the lower column wins
        check_equal(dsm.match_sift_features(d1, d2, capi.default_match_options(max_ratio=2.0, cross_check=cross)), ref)
        ref = oracle.match_sift_features_cpu(d1, d2, 0.8, 0.7, bool(cross))
        assert 5 not in ref[:, 0] and 17 not in ref[:, 0] and 33 in ref[:, 0]  # a duplicate of the best is the second best
        check_equal(dsm.match_sift_features(d1, d2, capi.default_match_options(cross_check=cross)), ref)


def test_runner_up_inside_the_winning_set_through_pass_2(dsm, oracle):
    """The three placements of test_second_best_in_the_same_column_set_as_the_best (runner-up in the set of the best column,
    in the other half-wave's set of the same tile, in another tile), planted among the COLUMNS of the gathered pass: image a
    holds a near copy (6 nudged bytes) and a runner-up (9) of a row of image b, so pass 1 yields two entries for that row and
    pass 2 must reject it at the default ratio with the true second best only.  n2 < n1 and 5, 33 and 129 entries: the
    gathered fragments are ragged."""
    rng = np.random.default_rng(2024)
    n1, n2 = 300, 200
    same_set = lambda c: (c & ~31) + 8 * ((((c & 31) >> 3) + 1) % 4) + (c & 7)
    other_half = lambda c: c ^ 4
    descs, pairs, want = [], [], []
    for entries in (5, 33, 129):
        a = rand_sift(rng, n1)
        b = rand_sift(rng, n2)
        used = set()
        for j in range(entries // 2):           # two entries per planted row of image b
            while True:
                c0 = int(rng.integers(0, n1 - 64))
                c1 = [same_set(c0), other_half(c0), c0 + 64][j % 3]
                if not {c0, c1} & used:
                    break
            used |= {c0, c1}
            if j % 2 and j % 3 != 2:
                c0, c1 = max(c0, c1), min(c0, c1)  # the runner-up at the LOWER column
            a[c0] = near(rng, b[j], 6)
            a[c1] = near(rng, b[j], 9)
        while True:                                # and one row with a single near copy: an odd count
            c0 = int(rng.integers(0, n1))
            if c0 not in used:
                break
        a[c0] = near(rng, b[entries // 2], 6)
        descs += [a, b]
        pairs.append((len(descs) - 2, len(descs) - 1))
        want.append(entries)
    for k, (i, j) in enumerate(pairs):  # the construction: the entry counts of pass 2, and most planted rows rejected
        assert len(oracle.match_sift_features_cpu(descs[i], descs[j], 0.8, 0.7, False)) == want[k]
    assert len(oracle.match_sift_features_cpu(descs[4], descs[5], 0.8, 0.7, True)) < 40
    dsm.set_images(descs)
    for ratio in (0.8, 0.95, 0.6):
        dsm.match_pairs(np.array(pairs, dtype=np.uint32), capi.default_match_options(max_ratio=ratio))
        offs, m = dsm.matches()
        for k, (i, j) in enumerate(pairs):
            check_equal(m[int(offs[k]):int(offs[k + 1])], oracle.match_sift_features_cpu(descs[i], descs[j], ratio, 0.7, True))


def test_pair_list_in_one_launch(dsm, oracle):
    """Six images of 0, 1, 255, 256, 513 and 700 features, every ordered pair in one call: the `order` indirection, empty
    images and the early return of row blocks without rows beside workgroups that run the tail."""
    rng = np.random.default_rng(31)
    sizes = [0, 1, 255, 256, 513, 700]
    base = rand_sift(rng, 800)
    descs = []
    for n in sizes:
        idx = rng.permutation(800)[:n]
        descs.append(np.clip(base[idx].astype(np.int32) + rng.integers(-5, 6, (n, 128)), 0, 255).astype(np.uint8))
    dsm.set_images(descs)
    pairs = [(i, j) for i in range(len(sizes)) for j in range(len(sizes)) if i != j]
    total = 0
    for cross in (1, 0):
        dsm.match_pairs(np.array(pairs, dtype=np.uint32), capi.default_match_options(cross_check=cross))
        offs, m = dsm.matches()
        for k, (i, j) in enumerate(pairs):
            check_equal(m[int(offs[k]):int(offs[k + 1])], oracle.match_sift_features_cpu(descs[i], descs[j], cross_check=bool(cross)))
        total += int(offs[-1])
    assert total > 2000


def test_fused_tail_equals_two_kernel_form(dsm, oracle, monkeypatch):
    """DSM_K1_RESOLVE_KERNEL=1 (check build): unfused k1_best_rows + k1_resolve_index, the independently scheduled form of the
    same arithmetic, gives the same offsets and matches as the product's fused kernel, and the oracle's."""
    from dagsfm_amd import synthetic
    scene = synthetic.Scene(4, 700, seed=12, n_pool=1500)
    ims = [scene.image(i) for i in range(4)]
    descs = [ims[0][0], ims[1][0][:513], ims[2][0][:255], ims[3][0]]
    pairs = synthetic.exhaustive_pairs(4)
    dsm.set_images(descs)
    dsm.match_pairs(pairs)
    offs0, m0 = dsm.matches()
    assert dsm.match_resolve_time() < 0.05  # ms: no resolve kernel, an empty interval between two events
    monkeypatch.setenv("DSM_K1_RESOLVE_KERNEL", "1")  # a check-build schedule: from here on `dsm` is the check library's context
    dsm.set_images(descs)
    dsm.match_pairs(pairs)
    offs1, m1 = dsm.matches()
    assert (offs0 == offs1).all() and (m0 == m1).all() and len(m0) > 100
    ref = oracle.match_sift_features_cpu(descs[0], descs[3])
    k = [tuple(p) for p in pairs].index((0, 3))
    assert (m1[int(offs1[k]):int(offs1[k + 1])] == ref).all()
