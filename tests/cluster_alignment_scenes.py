"""The scenes of the cluster-alignment edge tests (tests/test_cluster_alignment_edges_cpu.py, _gpu.py):
comparisons() lists (name, clusters, options, seeds, rule).

rule "clear": every pair of the entry has restatement margin >= 1e-9 (the CPU file asserts it), so the GPU file holds the
device to compare(...) == all True and to its own reported margins.
rule "graph": scenes whose all-inlier pairs tie by construction (the first PROSAC samples of a pair without outliers are
near-ties), so PROSAC's own choice is not compared; the counts, the inliers, the edge flags, the graph and the refitted Sim3s
are.  The CPU file asserts what makes that sound.

Seeds: a pair taken from a two-cluster starting point keeps that starting point's seeds (those of clusters (0, 1)) through an
explicit seeds matrix when it sits at other cluster indices, so that a scene of many pairs restates each of them as it was
chosen."""
import numpy as np

from tests import cluster_alignment_ref as ref
from tests.test_cluster_alignment_cpu import cluster, pair_of

CHUNK_NS = (255, 256, 257, 511, 512, 513, 769)  # AL_CHUNK = AL_BLOCK = 256: tail chunks of 255, 0, 1 and the refit's strides
BATCH_ENDS = (255, 256, 257, 512, 513)          # runs that end one trial before, at and after a batch of 256
THRESHOLD = 0.1


def scattered_pair(fx):
    """tests/test_cluster_alignment_gpu.py's scene of that name (that file needs the device library to import)."""
    out = sorted(np.random.default_rng(fx).choice(300, 150, replace=False))
    return pair_of(300, n_images=4, noise=0.04, seed=fx, outliers=out)[0]


def scattered(n, frac, rng_seed):
    return sorted(int(q) for q in np.random.default_rng(rng_seed).choice(n, int(frac * n), replace=False))


def pair_seeds(K, pairs, user_seed=0):
    """[K, K] seeds that give every listed pair (i, j) the default seeds of clusters (0, 1)."""
    s = np.zeros((K, K), np.uint32)
    for i, j in pairs:
        s[i, j] = ref.align_seed(0, 1, 0, user_seed)
        s[j, i] = ref.align_seed(0, 1, 1, user_seed)
    return s


def with_images(c, base):
    """the cluster with every image id moved up by base"""
    ob = np.array(c["obs"], np.int64).reshape(-1, 3)
    ob[:, 0] += base
    return dict(c, image_ids=(np.asarray(c["image_ids"], np.int64) + base).astype(np.uint32), obs=ob.astype(np.uint32))


def side_by_side(pairs, stride=10):
    """two-cluster scenes as clusters (0, 1), (2, 3), ... of one scene, on image ids of their own"""
    out = []
    for k, (a, b) in enumerate(pairs):
        out += [with_images(a, stride * k), with_images(b, stride * k)]
    return out


def merged(parts):
    """one cluster holding the points and observations of several"""
    xyz, ids, obs, imgs, base = [], [], [], [], 0
    for p in parts:
        ob = np.array(p["obs"], np.int64).reshape(-1, 3)
        ob[:, 2] += base
        xyz.append(np.asarray(p["xyz"]).reshape(-1, 3)), obs.append(ob), imgs.append(np.asarray(p["image_ids"], np.int64))
        ids.append(np.asarray(p["point_ids"], np.uint64) + np.uint64(base))
        base += len(xyz[-1])
    return cluster(np.concatenate(imgs), np.concatenate(xyz), np.concatenate(obs), ids=np.concatenate(ids))


def chain(links, stride=10):
    """links[c] = (a, b), a two-cluster scene: cluster c of the chain holds b of link c - 1 and a of link c"""
    sides = [(with_images(a, stride * k), with_images(b, stride * k)) for k, (a, b) in enumerate(links)]
    out = []
    for c in range(len(links) + 1):
        parts = ([sides[c - 1][1]] if c > 0 else []) + ([sides[c][0]] if c < len(links) else [])
        out.append(merged(parts))
    return out


# ---------------------------------------------------------------- PROSAC's chunks, strides and batches
def chunk_pair(n):
    return pair_of(n, n_images=4, noise=0.02, seed=1, outliers=scattered(n, 0.3, 1))[0]


def chunk_edges():
    cl = side_by_side([chunk_pair(n) for n in CHUNK_NS])
    K = len(cl)
    return [("chunk_edges", cl, {}, pair_seeds(K, [(2 * k, 2 * k + 1) for k in range(len(CHUNK_NS))]), "clear")]


def five_of_nine():
    return pair_of(9, outliers=(0, 2, 4, 6))[0]


FIVE_OF_NINE_OPTIONS = dict(max_reprojection_error=10.0)


def batch_ends():
    out = [("batch_end_%d" % it, scattered_pair(4), dict(min_iterations=it, max_iterations=it), None, "clear") for it in BATCH_ENDS]
    easy = pair_of(50, n_images=4, noise=0.001, seed=3)[0]
    out.append(("min_iterations_0", easy, dict(min_iterations=0), None, "clear"))
    out.append(("one_iteration", easy, dict(min_iterations=1, max_iterations=1), None, "clear"))
    # the cap moves to 2227 / 2234 inside the ninth batch: 4 or 5 inliers of 9
    out.append(("four_or_five_inliers", five_of_nine(), FIVE_OF_NINE_OPTIONS, None, "clear"))
    return out


# ---------------------------------------------------------------- the rulings
def one_common_image_scene():
    """(0, 1) share image 0 alone and 10 observation keys on it: correspondences, but no pair and no separator but those of
    (1, 2), a plain pair on images 10 and 11"""
    a, b = pair_of(10, n_images=1, seed=5)[0]
    c, d = pair_of(40, n_images=2, noise=0.02, seed=3, outliers=scattered(40, 0.3, 3))[0]
    return [a, merged([b, with_images(c, 10)]), with_images(d, 10)]


def fewer_than_four_scene():
    rng = np.random.default_rng(2)
    X = rng.uniform(-2, 2, (8, 3))
    Y = rng.uniform(-50, 50, (8, 3))
    obs = [(q % 2, q, q) for q in range(8)]
    return [cluster([0, 1], X, obs), cluster([0, 1], Y, obs)]


def weight_above_limit_pair():
    return pair_of(30, n_images=2, noise=0.002, seed=2, outliers=range(10, 30))[0]


def source_at_one_place():
    X = np.ones((4, 3))
    Y = np.random.default_rng(0).uniform(-1, 1, (4, 3))
    obs = [(q % 2, q, q) for q in range(4)]
    return [cluster([0, 1], X, obs), cluster([0, 1], Y, obs)]


DESTINATION = (0.5, -0.25, 2.0)
DESTINATION_MSD = 2.0766559657295187  # |DESTINATION|: s = 0 sends every source point to t = 0


def destination_at_one_place():
    """FindRTS' S < eps path: sigma = 0, c = 0, cR = 0, det = 0, s = 0; R stays cR = 0 and t stays Sim3()'s 0"""
    X = np.random.default_rng(0).uniform(-1, 1, (4, 3))
    Y = np.tile(DESTINATION, (4, 1))
    obs = [(q % 2, q, q) for q in range(4)]
    return [cluster([0, 1], X, obs), cluster([0, 1], Y, obs)]


def degenerate_head():
    """40 points over 5 common images; point 0 (the lowest id of the second cluster) is seen in the images 1 .. 4 as well, so
    the first five of the 44 correspondences are the same point: PROSAC's first samples fit a source of zero variance"""
    (a, b), _ = pair_of(40, n_images=5, noise=0.01, seed=4)
    extra = np.array([(im, 1000, 0) for im in range(1, 5)], np.uint32)
    return [dict(c, obs=np.concatenate([c["obs"], extra])) for c in (a, b)]


def rulings():
    out = [("one_common_image", one_common_image_scene(), {}, pair_seeds(3, [(1, 2)]), "clear"),
           ("fewer_than_four_inliers", fewer_than_four_scene(), {}, None, "clear"),
           ("weight_above_limit", weight_above_limit_pair(), {}, None, "clear"),
           ("source_at_one_place", source_at_one_place(), {}, None, "clear"),
           ("destination_at_one_place", destination_at_one_place(), {}, None, "clear")]
    for us in (0, 1):
        out.append(("degenerate_head_seed_%d" % us, degenerate_head(), dict(random_seed=us), None, "clear"))
    out.append(("degenerate_head_one_iteration", degenerate_head(), dict(min_iterations=1, max_iterations=1), None, "clear"))
    return out


# ---------------------------------------------------------------- the join: shared keys, empty clusters, wide ids
SAME_KEYS_SEED = 1  # clear at 1e-8 (so are 6 and 7; 3 and 4 are not, 2 and 5 lose an edge)


def same_keys():
    """three clusters that see the same 90 points under the same keys: every key yields 3 correspondences.  The point ids
    are permuted per cluster, so the canonical order (the id's rank in the second cluster) is not the point order."""
    n = 90
    rng = np.random.default_rng(SAME_KEYS_SEED)
    X = rng.uniform(-2, 2, (n, 3))
    obs = [(q % 4, q, q) for q in range(n)]
    out = []
    for c in range(3):
        s, R, t = float(rng.uniform(0.5, 2.0)), ref.random_rotation(rng), rng.uniform(-3, 3, 3)
        Y = s * X @ R.T + t + rng.normal(0, 0.02, X.shape)
        bad = rng.choice(n, n // 10, replace=False)
        Y[bad] += rng.uniform(-5, 5, (len(bad), 3))
        out.append(cluster(range(4), Y, obs, ids=rng.permutation(n) + 7))
    return [("same_keys", out, {}, None, "clear")]


def empty_base():
    return chain([chunk_pair(257), chunk_pair(255)])


EMPTY_BASE_PAIRS = ((0, 1), (1, 2))


def empty_cluster(kind):
    none = cluster([], np.zeros((0, 3)), np.zeros((0, 3)))
    # images only: the four images of the first link, so it pairs with clusters 0 and 1 of the base on no correspondence
    return none if kind == "nothing" else dict(none, image_ids=np.arange(4, dtype=np.uint32))


def with_empty(kind, where):
    """the base with an empty cluster first, in the middle or last; returns (clusters, seeds, position)"""
    base = empty_base()
    pos = dict(first=0, middle=1, last=len(base))[where]
    cl = base[:pos] + [empty_cluster(kind)] + base[pos:]
    moved = lambda c: c + (c >= pos)
    return cl, pair_seeds(len(cl), [(moved(i), moved(j)) for i, j in EMPTY_BASE_PAIRS]), pos


def empties():
    base = empty_base()
    out = [("empty_base", base, {}, pair_seeds(len(base), EMPTY_BASE_PAIRS), "clear")]
    for kind in ("nothing", "images_only"):
        for where in ("first", "middle", "last"):
            cl, seeds, _ = with_empty(kind, where)
            out.append(("empty_%s_%s" % (kind, where), cl, {}, seeds, "clear"))
    return out


WIDE_IMAGE = 0xFFFFFFFF


def wide_ids():
    """image id 2^32 - 1, point2D_idx up to 2^32 - 1, and point ids that differ only above bit 32, half of them >= 2^63:
    an order by the low word, or as int64, is another canonical order"""
    n = 64
    (a, b), _ = pair_of(n, n_images=2, noise=0.02, seed=7, outliers=scattered(n, 0.25, 7))
    high = np.random.default_rng(7).permutation(n).astype(np.uint64)  # bit 5 of it is bit 63 of the id
    ids = [(int(h) << 58) | 0x12345678 for h in high]
    obs = np.array(a["obs"], np.int64)
    obs[:, 0] = np.where(obs[:, 0] == 1, WIDE_IMAGE, 3)
    obs[:, 1] = WIDE_IMAGE - obs[:, 1] * 0x01000000
    imgs = [3, WIDE_IMAGE]
    return [("wide_ids", [cluster(imgs, a["xyz"], obs, ids=a["point_ids"]), cluster(imgs, b["xyz"], obs, ids=ids)], {}, None, "clear")]


# ---------------------------------------------------------------- the host graph
def good_pair(seed):
    """30 inliers of 30 (the seeds used: float32 margin of the weight >= 3e-9; seed 12's is 5e-10)"""
    return pair_of(30, n_images=2, noise=0.002, seed=seed)[0]


def five_clusters():
    """(0, 1) share one image and 30 keys: no pair.  (1, 2) and (3, 4) are good pairs of 30, (2, 3) has 20 gross outliers of
    30: a pair, no edge.  Two components of two: the one holding the smaller index wins, its larger node is the anchor."""
    a, b = pair_of(30, n_images=1, seed=11)[0]
    l12, l23, l34 = good_pair(10), weight_above_limit_pair(), good_pair(13)
    rest = chain([l12, l23, l34], stride=10)
    cl = [with_images(a, 90), merged([with_images(b, 90), rest[0]])] + rest[1:]
    return ("graph_five_clusters", cl, {}, pair_seeds(5, [(1, 2), (2, 3), (3, 4)]), "graph")


TIED_EDGES = ((0, 1), (1, 4))


def tied_path():
    """a path 0 - 1 - 2 - 3 and cluster 4 tied on to 1 by the data of (0, 1): cluster 4 is cluster 0 on other images, so the
    edges (0, 1) and (1, 4) have the same weight to the bit and Kruskal's sort orders them by (i, j).  Neither is on a
    cycle.  Leaves 0, 3, 4 go first, then 1 (the smaller of two): the anchor is 2."""
    l01, l12, l23 = good_pair(21), good_pair(22), good_pair(23)
    rest = chain([l01, l12, l23], stride=10)
    a, b = l01
    rest[1] = merged([rest[1], with_images(b, 50)])
    rest.append(with_images(a, 50))
    return ("graph_tied_path", rest, {}, None, "graph")


def graphs():
    return [five_clusters(), tied_path()]


KINDS = (("chunks", chunk_edges), ("batches", batch_ends), ("rulings", rulings), ("same_keys", same_keys), ("empties", empties),
         ("wide_ids", wide_ids), ("graphs", graphs))


def of_kind(kind):
    return tuple(dict(KINDS)[kind]())


def comparisons():
    return tuple(entry for kind, _ in KINDS for entry in of_kind(kind))


def flatten(clusters):
    """the arrays of the C call, as capi.Context.align_clusters builds them: offsets (images, points, observations), image
    ids, point ids, xyz, observations"""
    K = len(clusters)
    cat = lambda key, dt, shape: [np.ascontiguousarray(c[key], dt).reshape(shape) for c in clusters]
    imgs, pids = cat("image_ids", np.uint32, -1), cat("point_ids", np.uint64, -1)
    xyz, obs = cat("xyz", np.float64, (-1, 3)), cat("obs", np.uint32, (-1, 3))
    offs = lambda arrs: np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.uint32)
    return dict(K=K, image_offsets=offs(imgs), point_offsets=offs(pids), obs_offsets=offs(obs),
                image_ids=np.ascontiguousarray(np.concatenate(imgs), np.uint32),
                point_ids=np.ascontiguousarray(np.concatenate(pids), np.uint64),
                xyz=np.ascontiguousarray(np.concatenate(xyz), np.float64),
                obs=np.ascontiguousarray(np.concatenate(obs), np.uint32))
