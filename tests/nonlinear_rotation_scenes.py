"""The graphs of the NONLINEAR rotation estimator's device tests (tests/test_nonlinear_rotation_gpu.py): the shapes at which
its kernels can go wrong.  tests/test_nonlinear_rotation_cpu.py asserts without a device that every one of them is clear by
the restatement's margins and stable under the conditioning probe, so the device comparison is always the strict one.

A scene is a dict: pairs, qvecs, use (or None), options (restatement keywords; the same names are the C-ABI's fields)."""
import numpy as np

from tests.test_rotation_averaging import _edges_random, _graph, _qvecs, _rand_q


def _ring_plus(rng, n_img, n_edges):
    """a ring over n_img images plus random chords up to exactly n_edges edges"""
    s = {(i, (i + 1) % n_img) if i + 1 < n_img else (0, i) for i in range(n_img)}
    while len(s) < n_edges:
        a, b = (int(v) for v in rng.choice(n_img, 2, replace=False))
        s.add((min(a, b), max(a, b)))
    return np.array(sorted(s), np.int64)


def _moderate_graph(seed, n_img, pairs, spread, noise=0.0, n_corrupt=0):
    """test_rotation_averaging._graph with absolute rotations of `spread` rad (normal, per axis) instead of uniform ones: a
    sparse graph whose rotations reach pi is a hard non-convex problem from the zero start (the restatement then wanders for
    its 200 iterations, and no two summation orders agree on such a path); the shapes below are about the kernels, not that"""
    rng = np.random.default_rng(seed)
    aa = rng.normal(scale=spread, size=(n_img, 3))
    ang = np.linalg.norm(aa, axis=1, keepdims=True)
    absq = np.hstack([np.cos(ang / 2.0), np.sin(ang / 2.0) * aa / ang])
    corrupt = rng.choice(len(pairs), n_corrupt, replace=False) if n_corrupt else []
    q = _qvecs(rng, absq, pairs, noise, corrupt)
    o = rng.permutation(len(pairs))
    return pairs[o].astype(np.uint32), q[o]


def _scene(p, q, use=None, **options):
    return {"pairs": p, "qvecs": q, "use": use, "options": options}


def two_images():
    return _scene(*_moderate_graph(41, 2, np.array([(0, 1)]), 0.3, noise=0.01))


def triangle():
    p, q, _, _ = _graph(42, 3, np.array([(0, 1), (0, 2), (1, 2)]), noise=0.01)
    return _scene(p, q)


def identity():
    """every relative rotation the identity, from zero: cost 0, gradient 0 at iteration 0, every residual on the k = 2 branch"""
    pairs = _ring_plus(np.random.default_rng(43), 12, 20).astype(np.uint32)
    return _scene(pairs, np.tile([1.0, 0.0, 0.0, 0.0], (len(pairs), 1)))


def tree():
    rng = np.random.default_rng(44)
    pairs = np.array([(int(rng.integers(0, i)), i) for i in range(1, 40)], np.int64)
    return _scene(*_moderate_graph(45, 40, pairs, 0.3, noise=0.01))


def sized(n_img, n_edges, seed):
    def make():
        return _scene(*_moderate_graph(seed, n_img, _ring_plus(np.random.default_rng(seed), n_img, n_edges), 0.3, noise=0.003))
    return make


def hub():
    """image 0 joined to 300 images of a ring, and 20 images of degree 1: the long and the short CSR row"""
    ring = [(i, i + 1) for i in range(1, 300)] + [(1, 300)]
    spokes = [(0, i) for i in range(1, 301)]
    leaves = [(7 * k + 3, 301 + k) for k in range(20)]
    return _scene(*_moderate_graph(46, 321, np.array(ring + spokes + leaves, np.int64), 0.3, noise=0.004, n_corrupt=6))


def sparse_ids():
    ids = np.sort(np.random.default_rng(47).permutation(100000)[:60]).astype(np.int64) * 13 + 7
    p, q, _, _ = _graph(48, 60, _edges_random(np.random.default_rng(48), 60, 6), noise=0.004, n_corrupt=5, ids=ids)
    return _scene(p, q)


def repeats_and_mask():
    """repeats of earlier pairs in both orders with other rotations (ignored), and a mask that removes a tenth of the edges"""
    rng = np.random.default_rng(49)
    p, q, _, _ = _graph(50, 40, _edges_random(rng, 40, 6), noise=0.004)
    extra = rng.choice(len(p), 12, replace=False)
    p2 = np.vstack([p, p[extra[:6]], p[extra[6:], ::-1]])
    q2 = np.vstack([q, _rand_q(rng, 12)])
    use = np.ones(len(p2), np.uint8)
    use[rng.choice(len(p), len(p) // 10, replace=False)] = 0
    return _scene(p2, q2, use)


def two_components():
    rng = np.random.default_rng(51)
    big = _edges_random(rng, 50, 5)
    small = _edges_random(rng, 9, 3) + 50
    p, q, _, _ = _graph(52, 59, np.vstack([big, small]), noise=0.004, n_corrupt=4)
    return _scene(p, q)


def filter_splits():
    """a sparse noisy graph under a 0.3 degree orientation filter: the final component is a part of the first"""
    pairs = _edges_random(np.random.default_rng(25), 30, 3)
    rng = np.random.default_rng(25)
    q = _qvecs(rng, _rand_q(rng, 30), pairs, 0.004)
    return _scene(pairs.astype(np.uint32), q, max_relative_rotation_difference_degrees=0.3)


def corrupted40():
    """40 images, 8 neighbours, six corrupted edges"""
    p, q, bad, _ = _graph(5, 40, _edges_random(np.random.default_rng(4), 40, 8), noise=0.002, n_corrupt=6)
    s = _scene(p, q)
    s["bad"] = bad
    return s


SCENES = {
    "two_images": two_images, "triangle": triangle, "identity": identity, "tree": tree,
    "img255_e511": sized(255, 511, 61), "img256_e512": sized(256, 512, 62), "img257_e513": sized(257, 513, 63),
    "img150_e255": sized(150, 255, 64), "img150_e256": sized(150, 256, 65), "img150_e257": sized(150, 257, 66),
    "hub300": hub, "sparse_ids": sparse_ids, "repeats_and_mask": repeats_and_mask, "two_components": two_components,
    "filter_splits": filter_splits, "corrupted40": corrupted40,
}
# the scene that is also started from the robust estimator's result
CHAINED = "corrupted40"
