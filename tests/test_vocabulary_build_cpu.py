"""CPU-only: pins tests/vocabulary_build_ref.py -- the numpy restatement the device's vocabulary training is compared with -- to
the reference: to its own binary where oracle/_ref/libflann_ref.so exists (flann_ref_seed + flann_ref_quantize), and to the
answers recorded from it in tests/golden/vocab_quantize_v1.npz everywhere."""
import hashlib
import os

import numpy as np
import pytest

from tests import flann_ref
from tests import vocabulary_build_ref as R
from tests import vocabulary_build_scenes as S

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vocab_quantize_v1.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_golden_holds_data_only_and_is_small(golden):
    assert os.path.getsize(GOLDEN) < 600 * 1024
    assert all(golden[k].dtype.kind in "iub" for k in golden.files)  # np.load refuses pickled objects by default as well
    assert sorted({k.split("/")[0] for k in golden.files}) == sorted(list(S.CASES) + [S.LARGE])


def test_rand_stream_is_the_recorded_one(golden):
    """The recorded answers belong to this C library's rand(): its first draws after srand(seed) are recorded with them."""
    for name, (_, _, _, _, seed) in S.CASES.items():
        R.srand(seed)
        assert [R.libc_rand() for _ in range(8)] == list(golden[name + "/rand8"]), name


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_restatement_equals_recorded_reference(golden, name):
    d, nw, b, it, seed = S.CASES[name]
    assert [int(v) for v in golden[name + "/options"]] == [len(d), nw, b, it, seed]
    assert hashlib.sha256(d.tobytes()).digest() == golden[name + "/input_sha256"].tobytes()
    if name + "/input" in golden.files:
        assert (golden[name + "/input"] == d).all()
    R.srand(seed)
    words = R.quantize(d, nw, b, it)[0]
    assert len(words) == int(golden[name + "/count"]) and (words == golden[name + "/words"]).all()
    if name in S.EXPECTED_COUNT:
        assert len(words) == S.EXPECTED_COUNT[name]


@pytest.mark.parametrize("name", sorted(S.CASES))
def test_restatement_equals_reference_binary(name):
    lib = flann_ref.load()
    if lib is None:
        pytest.skip("oracle/_ref/libflann_ref.so was not built (no reference on this machine)")
    d, nw, b, it, seed = S.CASES[name]
    out = np.zeros((nw, 128), np.uint8)
    lib.flann_ref_seed(seed)
    count = lib.flann_ref_quantize(d.ctypes.data, len(d), nw, b, it, out.ctypes.data)
    R.srand(seed)
    words = R.quantize(d, nw, b, it)[0]
    assert count == len(words) and (out[:count] == words).all()


def test_identical_rows_give_few_distinct_words(golden):
    assert len(np.unique(golden["identical_597_of_600/words"], axis=0)) == 4
    assert int(golden["identical_597_of_600/count"]) == 40


def test_prefix_selection_equals_subtractive_walk():
    rng = np.random.default_rng(0)
    for trial in range(300):
        n = int(rng.integers(1, 40))
        closest = rng.integers(0, [1, 3, 1 << 23][trial % 3], n)
        pot = np.float64(closest.sum())
        draws = [0, 1, R.RAND_MAX, R.RAND_MAX - 1, int(rng.integers(0, R.RAND_MAX))]
        for r in draws:
            rv = R.rand_double(pot, lambda: r)
            assert R.select_prefix(rv, closest) == R.select_walk(rv, closest), (closest, r)
    zeros = np.zeros(9, np.int64)
    assert R.select_prefix(R.rand_double(0.0, lambda: 12345), zeros) == R.select_walk(np.float64(0.0), zeros) == 0
    # a draw that lands on the last point: everything before it weighs nothing
    last = np.array([0, 0, 0, 7])
    assert R.select_prefix(np.float64(6.5), last) == R.select_walk(np.float64(6.5), last) == 3
    assert R.select_prefix(np.float64(7.0), np.array([3, 4, 5])) == R.select_walk(np.float64(7.0), np.array([3, 4, 5])) == 1


def test_median():
    f = np.float32
    assert R.median_f32([f(3), f(1), f(2)]) == f(2)                       # odd
    assert R.median_f32([f(4), f(1), f(3), f(2)]) == f(2.5)               # even: (m1 + m2) / 2
    assert R.median_f32([f(1), f(5), f(5), f(5), f(9)]) == f(5)           # ties
    assert R.median_f32([f(2), f(2), f(7), f(7)]) == f(4.5)
    a, b = f(16777216.0), f(16777218.0)                                    # the sum rounds in float before the halving
    assert R.median_f32([a, b]) == f(np.float64(f(a + b)) / 2.0)
    big = f(3e38)
    assert np.isinf(R.median_f32([big, big]))                              # (m1 + m2) overflows in float, as in the reference


def test_binding_defaults():
    from dagsfm_amd import capi
    o = capi.default_vocabulary_build_options()
    assert (o.num_visual_words, o.branching, o.num_iterations, o.workgroup_node_max) == (65536, 256, 11, 0)
    assert len(capi.VOCABULARY_BUILD_STAGES) == 6
