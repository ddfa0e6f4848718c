"""Inputs for the retrieval edge-case suites (tests/test_retrieval_edges.py on the CPU, tests/test_retrieval_edges_gpu.py on
the device) and the arithmetic that says which path of dagsfm_amd/csrc/retrieval.hip an input reaches.  Everything here is
numpy: the properties are computed from word ids, the row padding rule and the signatures, never from a device result.

Layout facts restated from the kernels (the CPU tests pin them, so that a renumbering there shows up here):
  * word search (k_vocab_assign_mfma): the words stream in steps of 64, a step is two tiles of 32, and inside a tile a lane of
    half-wave `half` holds the columns 8*(r>>2) + 4*half + (r&3), r = 0..15 -- column c belongs to half (c >> 2) & 1;
  * rows: an image takes ceil(n / 256) * 256 rows (none when it is empty), a workgroup takes 512 rows;
  * scoring (k_vocab_score, k_vocab_matches): an inverted file is read in chunks of 64 entries from its own start;
  * query batches (dsm_retrieval_query): min(NI, 2^30 / (24 NI)) queries at a time."""
import numpy as np

INVALID = 0x7fffffff
RK_MAX = 8
CHUNK = 64
MAX_HAMMING = 24


# ------------------------------------------------------------------------------------------------ word search
def word_half(i):
    return (i >> 2) & 1


def word_tile(i):
    return (i >> 5) & 1


def word_step(i):
    return i >> 6


def exact_word_ids(desc, words, k):
    """The k nearest words by exact int64 squared distance, ties to the lower id (stable argsort); INVALID where the
    vocabulary has fewer than k words."""
    d = desc.astype(np.int64)
    w = words.astype(np.int64)
    dist = (d * d).sum(1)[:, None] + (w * w).sum(1)[None, :] - 2 * (d @ w.T)
    order = np.argsort(dist, axis=1, kind="stable")[:, :k]
    out = np.full((len(desc), k), INVALID, np.int64)
    out[:, :order.shape[1]] = order
    return out, dist


def padded_rows(feature_counts):
    return sum((n + 255) // 256 * 256 for n in feature_counts)


def last_workgroup_half_empty(feature_counts):
    return padded_rows(feature_counts) % 512 == 256


# feature counts per image; between them: images of 0, 1, 255, 256 and 257 features, padded totals of 256 .. 1280 rows
IMAGE_SETS = {
    256: [0, 1],
    512: [257],
    768: [0, 255, 256, 1],
    1024: [257, 256, 0, 255],
    1280: [1, 257, 0, 256, 255],
}

VOCABULARY_SIZES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097]


def byte_vocabulary(rng, n_words):
    """Arbitrary bytes, with an all-0 and an all-255 word where there is room (the int8 bias identity's extremes)."""
    words = rng.integers(0, 256, (n_words, 128)).astype(np.uint8)
    if n_words >= 3:
        words[n_words // 2] = 0
        words[n_words - 1] = 255
    return words


def byte_descriptors(rng, n, words):
    """Arbitrary bytes; the first rows are all 0, all 255, a copy of a word and a word's neighbour."""
    d = rng.integers(0, 256, (n, 128)).astype(np.uint8)
    special = [np.zeros(128, np.uint8), np.full(128, 255, np.uint8), words[int(rng.integers(0, len(words)))].copy(),
               (words[0].astype(np.int64) + rng.integers(-1, 2, 128)).clip(0, 255).astype(np.uint8)]
    for i, s in enumerate(special[:n]):
        d[i] = s
    return d


def identity_projection():
    """Projection row i = unit vector e_i, every threshold 127.5: bit i of a signature is descriptor[i] > 127."""
    proj = np.zeros((64, 128), np.float32)
    proj[np.arange(64), np.arange(64)] = 1.0
    return proj


def vocabulary_of(words, proj=None):
    proj = identity_projection() if proj is None else proj
    return words, proj, np.full((len(words), 64), 127.5, np.float32)


# Equal words planted by id.  Each group is one word repeated at these ids; `spans` names what the group must straddle.
TIE_WORDS = 200
TIE_GROUPS = {
    "halves": ([2, 6], {"half"}),                      # c and c ^ 4: the two halves of one tile
    "halves_high": ([27, 31], {"half"}),
    "tiles": ([10, 42], {"tile"}),                     # same half-wave, the two tiles of one step
    "tiles_and_halves": ([11, 61], {"half", "tile"}),
    "steps": ([21, 85], {"step"}),
    "steps_far": ([24, 152], {"step"}),
    "steps_and_halves": ([25, 190], {"half", "step"}),
    "nine": ([1, 5, 33, 37, 65, 69, 97, 101, 129], {"half", "tile", "step"}),
    "twelve": ([3, 7, 35, 39, 67, 71, 99, 103, 131, 135, 163, 167], {"half", "tile", "step"}),
    "twenty": (list(range(12, 20)) + list(range(44, 52)) + list(range(76, 80)), {"half", "tile", "step"}),
}
# Pairs of DIFFERENT words with a descriptor exactly between them (distance 1 to both)
EQUIDISTANT_PAIRS = {"halves": (56, 60), "tiles": (70, 102), "steps": (110, 180), "neighbours": (120, 121)}


def group_spans(ids):
    """What a set of word ids straddles: 'half' = both half-waves (their lists meet only in the final merge), 'tile' = both
    tiles of one 64-word step, 'step' = more than one step."""
    s = set()
    for a in ids:
        for b in ids:
            if word_half(a) != word_half(b):
                s.add("half")
            if word_step(a) == word_step(b) and word_tile(a) != word_tile(b):
                s.add("tile")
            if word_step(a) != word_step(b):
                s.add("step")
    return s


def tie_case(seed=11):
    """(words [200], descriptors, owner): random byte words with the groups of TIE_GROUPS planted, and descriptors that are
    copies / near copies of every planted word (equal distance to all its copies) or lie exactly between the two words
    of an EQUIDISTANT_PAIRS entry.  513 rows: with one image, two workgroups and a last one that is half empty."""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 256, (TIE_WORDS, 128)).astype(np.uint8)
    desc, owner = [], []
    for name, (ids, _) in TIE_GROUPS.items():
        base = rng.integers(2, 254, 128).astype(np.uint8)
        words[ids] = base
        desc.append(base.copy())
        owner.append(name)
        for _ in range(3):
            d = base.astype(np.int64)
            j = rng.choice(128, 5, replace=False)
            d[j] += rng.choice([-2, -1, 1, 2], 5)
            desc.append(d.astype(np.uint8))
            owner.append(name)
    for name, (a, b) in EQUIDISTANT_PAIRS.items():
        base = rng.integers(2, 254, 128).astype(np.uint8)
        j = int(rng.integers(0, 128))
        words[a] = base
        words[b] = base
        words[b, j] = base[j] + 2
        d = base.copy()
        d[j] = base[j] + 1
        desc.append(d)
        owner.append("between_" + name)
    desc = np.array(desc, np.uint8)
    filler = rng.integers(0, 256, (513 - len(desc), 128)).astype(np.uint8)
    return words, np.concatenate([desc, filler]), owner


# ------------------------------------------------------------------------------------------------ long inverted files
def centres(n_words):
    """Well separated word centres: the upper 64 bytes choose the word (40, 120, 200), the lower 64 sit at the threshold."""
    w = np.full((n_words, 128), 127, np.uint8)
    for i in range(n_words):
        w[i, 64:] = 40 + 80 * i
    return w


def feature(word, mask, centre_words, rng):
    """A descriptor of word `word` whose signature under identity_projection() is exactly `mask` (bit i <-> byte i > 127)."""
    d = centre_words[word].copy()
    bits = np.array([(int(mask) >> i) & 1 for i in range(64)])
    jitter = rng.integers(0, 4, 64)
    d[:64] = np.where(bits == 1, 128 + jitter, 127 - jitter)
    return d


def random_mask(rng, popcount):
    m = 0
    for b in rng.choice(64, popcount, replace=False):
        m |= 1 << int(b)
    return m


ALL_ONES = (1 << 64) - 1
# counts[image][word] of the long-file cases; what each layout is for is asserted by the CPU test from the oracle's word ids.
# "ones": (image, word) whose features all carry the all-ones signature -- a run no ordinary query votes for.
LONG_CASES = {
    # file 0: 40 | 50 (open over 64) | 110 (open over 128 and 192) | 56 (ends at 256) | 70 (open over 320)
    # file 1: 64 (ends at 64) | 64 (ends at 128) | 30 | 34 | 128 (a whole chunk, ends with the file at 320)
    # file 2: 30 | 80 all-ones (carried over 64 with no vote) | 40 | 300 | 130
    3: dict(counts=[[40, 64, 0], [50, 64, 0], [110, 30, 30], [56, 34, 80], [70, 0, 40], [0, 0, 300], [0, 128, 0], [0, 0, 130]],
            ones=[(3, 2)]),
    # file 0: 100 | 92 (open over 128, ends at 192) | 200 ;  file 1: 64 (ends at 64) | 100 all-ones (carried over 128) | 220 (ends with the file at 384)
    2: dict(counts=[[100, 0], [92, 64], [200, 0], [0, 100], [0, 220]], ones=[(3, 1)]),
    # one word, one file: 130 | 126 (ends at 256) | 100 all-ones (carried over 320) | 220 (ends with the file at 576)
    1: dict(counts=[[130], [126], [100], [220]], ones=[(2, 0)]),
}
POPCOUNTS = [0, 23, 24, 25, 64]  # Hamming distances from a zero signature that the cases place on purpose


def long_case(n_words, seed=5):
    """(vocabulary, descriptors per image, masks per image, intended word per image): the first feature of every (image,
    word) block has signature 0; the others take popcounts from POPCOUNTS and small random ones."""
    spec = LONG_CASES[n_words]
    rng = np.random.default_rng(seed + n_words)
    cw = centres(n_words)
    descs, masks, wordof = [], [], []
    for img, row in enumerate(spec["counts"]):
        d, m, wd = [], [], []
        for w, n in enumerate(row):
            for f in range(n):
                if (img, w) in spec["ones"]:
                    mask = ALL_ONES
                elif f == 0:
                    mask = 0
                elif f <= len(POPCOUNTS):
                    mask = random_mask(rng, POPCOUNTS[f - 1])
                else:
                    mask = random_mask(rng, int(rng.choice([0, 1, 3, 8, 15, 23, 24, 25, 40, 64])))
                d.append(feature(w, mask, cw, rng))
                m.append(mask)
                wd.append(w)
        order = rng.permutation(len(d))  # words interleaved inside an image: the inverted files still come out in feature order
        descs.append(np.array(d, np.uint8)[order])
        masks.append(np.array(m, np.uint64)[order])
        wordof.append(np.array(wd, np.int64)[order])
    return vocabulary_of(cw), descs, masks, wordof


def inverted_files(word_ids_per_image, n_words):
    """Entries (word, image, feature) in the order of the inverted files -> per word the list of runs (image, start, end)
    with positions relative to the file's start, and per word the (image, feature) arrays."""
    runs, entries = [], []
    for w in range(n_words):
        imgs, feats = [], []
        for img, ids in enumerate(word_ids_per_image):
            f = np.nonzero(np.asarray(ids) == w)[0]
            imgs += [img] * len(f)
            feats += list(f)
        imgs = np.array(imgs, np.int64)
        r, p = [], 0
        while p < len(imgs):
            e = p
            while e < len(imgs) and imgs[e] == imgs[p]:
                e += 1
            r.append((int(imgs[p]), p, e))
            p = e
        runs.append(r)
        entries.append((imgs, np.array(feats, np.int64)))
    return runs, entries


def boundaries_crossed(start, end):
    """Chunk boundaries strictly inside a run [start, end): the run is open at each of them."""
    return (end - 1) // CHUNK - start // CHUNK


def run_properties(runs):
    """Which of the chunk cases of k_vocab_score the runs of ONE set of inverted files contain."""
    p = set()
    for file_runs in runs:
        length = file_runs[-1][2] if file_runs else 0
        for (_, s, e) in file_runs:
            mid = s % CHUNK != 0
            if mid and boundaries_crossed(s, e) == 1:
                p.add("open_over_one")
            if mid and boundaries_crossed(s, e) >= 2:
                p.add("open_over_two")  # covers the whole chunk between the two boundaries
            if s % CHUNK == 0 and e - s >= CHUNK:
                p.add("whole_chunk_from_boundary")
            if e in (64, 128) and e < length:
                p.add("ends_at_%d_followed" % e)
            if mid and e % CHUNK == 0 and e < length:
                p.add("mid_start_ends_on_boundary_followed")
            if e == length and e % CHUNK == 0:
                p.add("ends_with_file_on_boundary")
    return p


def popcount64(x):
    return np.bitwise_count(np.asarray(x, np.uint64)).astype(np.int64)


def carried_run_without_votes(runs, entries, sigs_per_image, query_sig):
    """True when, for a query signature, some run is open at a chunk boundary with no entry within MAX_HAMMING and the next
    run of the file has one: the carry (image, 0 votes) must be dropped, not finalised."""
    for w, file_runs in enumerate(runs):
        imgs, feats = entries[w]
        esig = np.array([sigs_per_image[int(i)][int(f)] for i, f in zip(imgs, feats)], np.uint64)
        votes = popcount64(esig ^ np.uint64(query_sig)) <= MAX_HAMMING
        for a, b in zip(file_runs, file_runs[1:]):
            if boundaries_crossed(a[1], a[2]) >= 1 and not votes[a[1]:a[2]].any() and votes[b[1]:b[2]].any():
                return True
    return False


# ------------------------------------------------------------------------------------------------ query batches
def query_batch(n_images):
    return max(1, min(n_images, (1 << 30) // (24 * n_images)))


BATCH_IMAGES = 6700
BATCH_WORDS = 300


def clustered_case(rng, n_words, feature_counts, spread=12):
    """A vocabulary of arbitrary byte words with a random orthogonal projection, and images whose descriptors scatter around
    random words."""
    words = rng.integers(0, 256, (n_words, 128)).astype(np.uint8)
    q, _ = np.linalg.qr(rng.normal(size=(128, 128)))
    proj = np.ascontiguousarray(q[:64], np.float32)
    thr = (words.astype(np.float32) @ proj.T).astype(np.float32)
    descs = []
    for n in feature_counts:
        pick = rng.integers(0, n_words, n)
        d = words[pick].astype(np.int64) + rng.integers(-spread, spread + 1, (n, 128))
        descs.append(d.clip(0, 255).astype(np.uint8).reshape(n, 128))
    return (words, proj, thr), descs


def batch_case():
    rng = np.random.default_rng(77)
    counts = rng.integers(8, 17, BATCH_IMAGES)
    return clustered_case(rng, BATCH_WORDS, [int(c) for c in counts], spread=40)
