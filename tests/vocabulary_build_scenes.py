"""Seeded descriptor sets for the vocabulary-training tests (tests/test_vocabulary_build_cpu.py, _gpu.py).

CASES: name -> (descriptors, num_visual_words, branching, num_iterations, srand seed).  Each case is small enough for the
reference's single-threaded k-means tree to take well under a second."""
import numpy as np


def modes(n, num_modes, seed, spread=12.0):
    """n SIFT-like uint8 descriptors around num_modes centres."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 160, (num_modes, 128)).astype(np.float64)
    which = rng.integers(0, num_modes, n)
    return np.clip(np.rint(centres[which] + rng.normal(0.0, spread, (n, 128))), 0, 255).astype(np.uint8)


def uniform(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 128)).astype(np.uint8)


def with_identical_rows(n, identical, seed):
    d = modes(n, 6, seed)
    d[:identical] = d[0]
    return d


def _cases():
    c = {}
    c["smallest_64_16_4"] = (uniform(64, 1), 16, 4, 11, 1)
    c["modes_3000_64_4"] = (modes(3000, 40, 2), 64, 4, 11, 2)
    c["break_3000_9_4"] = (modes(3000, 40, 2), 9, 4, 11, 3)
    c["exact_3000_10_4"] = (modes(3000, 40, 2), 10, 4, 11, 3)
    c["converged_5000_64_8"] = (modes(5000, 30, 4), 64, 8, 11, 4)
    c["one_iteration_5000_64_8"] = (modes(5000, 30, 4), 64, 8, 1, 4)
    c["batch_edges_1000_300_8"] = (modes(1000, 20, 5), 300, 8, 11, 5)
    c["branching_256_2048"] = (modes(2048, 50, 6), 256, 256, 11, 6)
    c["identical_500_of_600"] = (with_identical_rows(600, 500, 7), 40, 4, 11, 7)
    c["identical_597_of_600"] = (with_identical_rows(600, 597, 7), 40, 4, 11, 7)
    # one below and one above a multiple of 64 and of the 256-point chunk a workgroup takes
    c["n_255"] = (modes(255, 9, 8), 32, 4, 11, 8)
    c["n_257"] = (modes(257, 9, 8), 32, 4, 11, 8)
    c["n_511"] = (modes(511, 9, 9), 32, 8, 11, 9)
    c["n_513"] = (modes(513, 9, 9), 32, 8, 11, 9)
    return c


CASES = _cases()
# the count the reference returns where it is not num_visual_words (the issue's figures, pinned by the golden file too)
EXPECTED_COUNT = {"break_3000_9_4": 7, "exact_3000_10_4": 10, "batch_edges_1000_300_8": 295}


LARGE = "large_70000_64_64"


def large_case():
    """A root of more than 65 536 points: 274 chunks, more than the 256 threads that scan the chunk sums of the k-means++ draw, so
    every thread sums a run of chunks.  Too slow for the numpy restatement: compared with the recorded reference only."""
    return modes(70000, 50, 10), 64, 64, 11, 10


def embedding_scene(seed=11):
    """Descriptors whose exact nearest words have 0, 1, 4, 5, 6 and 65 members: (descriptors, words, projection, word ids)."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 4, 5, 6, 65, 7, 12]
    words = (np.arange(len(sizes))[:, None] * 30 + rng.integers(0, 8, (len(sizes), 128))).astype(np.uint8)
    rows, ids = [], []
    for w, s in enumerate(sizes):
        rows.append(np.clip(words[w].astype(np.int64) + rng.integers(-5, 6, (s, 128)), 0, 255).astype(np.uint8))
        ids += [w] * s
    desc = np.concatenate(rows)
    perm = rng.permutation(len(desc))
    projection = np.linalg.qr(rng.normal(size=(128, 128)))[0][:64].astype(np.float32)
    return desc[perm], words, projection, np.asarray(ids, np.int32)[perm]
