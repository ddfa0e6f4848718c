"""Seeded descriptor sets for the vocabulary-training tests (tests/test_vocabulary_build_cpu.py, _gpu.py).

CASES: name -> (descriptors, num_visual_words, branching, num_iterations, srand seed).  Each case is small enough for the
reference's single-threaded k-means tree to take well under a second.  EDGE_CASES (the same form) and DRAW_CASES (injected
draws instead of a seed) are the cases of tests/test_vocabulary_build_edges_cpu.py, _gpu.py."""
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


def _edge_cases():
    """What CASES leaves out (tests/test_vocabulary_build_edges_cpu.py, _gpu.py): branchings that are no power of two, one past a
    full tile of 16 centres and 15 past one, above the 256 threads of a block; 0, 2 and "until convergence" iterations; clusters
    the last iteration emptied (NaN centres); roots around the batching bound 2 * branching - 1."""
    c = {}
    c["branching_2"] = (modes(100, 5, 21), 20, 2, 11, 21)
    c["branching_3"] = (modes(200, 7, 22), 40, 3, 11, 22)
    c["branching_17"] = (modes(700, 12, 23), 120, 17, 11, 23)
    c["branching_31"] = (modes(900, 12, 24), 100, 31, 11, 24)
    # three clustered nodes: the root, the 700 identical rows (whole chip at the default switch), what the repair leaves of them
    c["branching_300"] = (with_identical_rows(1600, 700, 25), 900, 300, 11, 25)
    c["no_iteration"] = (modes(1000, 20, 26), 100, 8, 0, 26)
    c["until_convergence"] = (modes(2000, 30, 28), 64, 8, -1, 28)
    c["two_iterations"] = (modes(2000, 30, 28), 64, 8, 2, 28)
    # one iteration over identical rows: its repair fills the empty clusters, nothing recomputes the emptied one's 0 * inf centre
    c["emptied_clusters"] = (with_identical_rows(600, 500, 7), 40, 4, 1, 7)
    for n in (8, 9, 14, 15, 16):  # branching, + 1, 2 * branching - 2, - 1, 2 * branching
        c["root_%d" % n] = (modes(n, 3, 30 + n), 8, 8, 11, 30 + n)
    return c


EDGE_CASES = _edge_cases()
EDGE_EXPECTED_COUNT = {"branching_3": 39, "branching_17": 113, "branching_31": 91, "branching_300": 898, "no_iteration": 99}
EDGE_NAN_CASES = ("emptied_clusters",)

RAND_MAX = 2147483647


def cycled_draws(values):
    """A rand() that hands out `values` over and over."""
    state = [0]

    def rand():
        v = values[state[0] % len(values)]
        state[0] += 1
        return v
    return rand


def _draw_cases():
    """name -> (descriptors, num_visual_words, branching, num_iterations, the values rand() cycles through): the extremes of the
    k-means++ selection.  Draw 0 makes every seed point 0 (branching - 1 empty clusters, repaired one by one beside NaN centres),
    RAND_MAX lands on the last point that weighs anything.  The reference's binary draws from rand() alone: these are device
    against restatement."""
    d = modes(700, 12, 40)
    c = {}
    c["zero_8"] = (d, 64, 8, 11, (0,))
    c["zero_17"] = (d, 64, 17, 11, (0,))
    c["zero_one_iteration"] = (d, 64, 8, 1, (0,))
    c["rand_max"] = (d, 64, 8, 11, (RAND_MAX,))
    c["alternating"] = (d, 64, 8, 11, (0, RAND_MAX))
    return c


DRAW_CASES = _draw_cases()
DRAW_EXPECTED_COUNT = {"zero_17": 49, "zero_one_iteration": 1}


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


# word -> members of embedding_edge_scene; every other word has none
EDGE_MEMBERS = {2: 6, 10: 8, 63: 5, 65: 4, 70: 6, 100: 8, 127: 8, 128: 300}


def embedding_edge_scene(seed=51):
    """130 words -- two full 64-word tiles of the nearest-word search and two words past them, no multiple of the 4 words a block
    of the median kernel takes -- with ties that cross the tile edges: word 64 is a copy of word 63 and word 129 of word 2 (the
    lower id must win), and words 127 and 128 differ in byte 0 alone, by 6, with the 8 members of word 127 exactly between them
    (byte 0 three above the one, three below the other).  Members per word: EDGE_MEMBERS, i.e. 0, 4, 5, 6, 8 and 300.
    (descriptors [345, 128], words, projection, the intended word ids)."""
    rng = np.random.default_rng(seed)
    words = rng.integers(3, 253, (130, 128)).astype(np.uint8)
    words[64] = words[63]
    words[129] = words[2]
    words[127, 0] = 100
    words[128] = words[127]
    words[128, 0] = 106
    rows, ids = [], []
    for w, s in sorted(EDGE_MEMBERS.items()):
        r = (words[w].astype(np.int64) + rng.integers(-2, 3, (s, 128))).astype(np.uint8)
        if w == 127:
            r[:, 0] = 103
        rows.append(r)
        ids += [w] * s
    desc = np.concatenate(rows)
    perm = rng.permutation(len(desc))
    projection = np.linalg.qr(rng.normal(size=(128, 128)))[0][:64].astype(np.float32)
    return desc[perm], words, projection, np.asarray(ids, np.int32)[perm]


def overflow_scene(members, seed=52):
    """One word, a projection whose row 0 is 1e36 * e_0, byte 0 of every descriptor in 180 .. 255: the two middle values of
    column 0 are about 2e38 each and their float sum is past FLT_MAX.  (descriptors, words, projection)."""
    rng = np.random.default_rng(seed)
    desc = rng.integers(0, 256, (members, 128)).astype(np.uint8)
    desc[:, 0] = rng.integers(180, 256, members)
    projection = np.linalg.qr(rng.normal(size=(128, 128)))[0][:64].astype(np.float32)
    projection[0] = 0.0
    projection[0, 0] = 1e36
    return desc, desc[:1].copy(), projection
