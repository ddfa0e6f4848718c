"""The pose check of EstimateWithRelativePose stops a candidate pose once it can no longer win (k_final_pose: probe of 4 x 16
inliers, the leader over its remaining inliers, the others while still open).  Product against the oracle, and product against
the check build's every-candidate form (DSM_POSE_FULL, k_final_pose_full) record for record, on the cases where the
schedule's choices matter: calibrated and planar scenes, pure rotation (PANORAMIC: one candidate, t = 0), inlier sets of fewer
than 16 and exactly 16 points (the probe alone), two candidates with equal counts (the later one must win), and pairs where
every candidate has count 0 (nothing settles; the last candidate wins)."""
import contextlib
import os

import numpy as np
import pytest

from dagsfm_amd import capi, synthetic
from tests.test_verify_gpu import tvg_equal

pytestmark = pytest.mark.gpu

F, CX, CY = 800.0, 500.0, 375.0


def _cam():
    return capi.simple_pinhole(F, CX, CY, 1000, 750, 1)


def _rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def _pixels(Xc):
    return np.c_[F * Xc[:, 0] / Xc[:, 2] + CX, F * Xc[:, 1] / Xc[:, 2] + CY]


def _pair(X, R, t, rng, noise=0.05):
    """Correspondences of the points X (camera-1 frame) in camera 1 = [I | 0] and camera 2 = [R | t], pixel noise added."""
    p1 = _pixels(X) + rng.normal(scale=noise, size=(len(X), 2))
    p2 = _pixels(X @ R.T + t) + rng.normal(scale=noise, size=(len(X), 2))
    m = np.stack([np.arange(len(X)), np.arange(len(X))], axis=1).astype(np.uint32)
    return p1, p2, m


def _front_points(rng, n, depth=(4.0, 8.0)):
    z = rng.uniform(*depth, n)
    return np.c_[rng.uniform(-0.4, 0.4, n) * z, rng.uniform(-0.3, 0.3, n) * z, z]


def _record(g):
    return bytes(memoryview(g).cast("B"))


@contextlib.contextmanager
def _pose_full():
    """DSM_POSE_FULL for the calls inside (the binding forwards the process's DSM_* variables to a context before every
    call; the product context must not see this check-only switch)."""
    os.environ["DSM_POSE_FULL"] = "1"
    try:
        yield
    finally:
        del os.environ["DSM_POSE_FULL"]


def _leaf_both_forms(prod, full, oracle, p1, p2, m, opts, seed, tag):
    cam = _cam()
    ref, ref_inl = oracle.estimate_two_view_geometry(cam, p1, cam, p2, m, opts, seed)
    got, got_inl = prod.estimate_two_view_geometry(cam, p1, cam, p2, m, opts, seed)
    with _pose_full():
        full_rec, full_inl = full.estimate_two_view_geometry(cam, p1, cam, p2, m, opts, seed)
    tvg_equal(got, ref, tag)
    assert (got_inl == ref_inl).all(), tag
    assert _record(got) == _record(full_rec), (tag, "product vs every-candidate form")
    assert (got_inl == full_inl).all(), tag
    return got


@pytest.fixture(scope="module")
def contexts():
    """The product context, and a context of the check build for the every-candidate pose check."""
    return capi.Context(0, check=False), capi.Context(0, check=True)


def _stage_both_forms(contexts, oracle, scene, n_img, tag, want_configs):
    prod, full = contexts
    ims = [scene.image(i) for i in range(n_img)]
    cams = [_cam() for _ in range(n_img)]
    pairs = synthetic.exhaustive_pairs(n_img)
    opts = capi.default_two_view_options()
    recs = []
    for ctx, env in ((prod, contextlib.nullcontext()), (full, _pose_full())):
        with env:
            ctx.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
            ctx.match_pairs(pairs)
            ctx.verify_pairs(opts, user_seed=3, stage_filter=False)
            recs.append((ctx.matches(), ctx.two_view_geometries(), ctx.inlier_matches()))
    (offs, m), tvgs, (ioffs, im) = recs[0]
    _, tvgs_full, (ioffs_full, im_full) = recs[1]
    assert (np.array(ioffs) == np.array(ioffs_full)).all() and (np.array(im) == np.array(im_full)).all(), tag
    seen = set()
    for k, (i, j) in enumerate(pairs):
        assert _record(tvgs[k]) == _record(tvgs_full[k]), (tag, i, j, "product vs every-candidate form")
        mk = m[int(offs[k]):int(offs[k + 1])]
        ref, ref_inl = oracle.estimate_two_view_geometry(cams[i], ims[i][1].astype(np.float64), cams[j],
                                                         ims[j][1].astype(np.float64), mk, opts, capi.pair_seed(int(i), int(j), 3))
        tvg_equal(tvgs[k], ref, (tag, i, j))
        assert (im[int(ioffs[k]):int(ioffs[k + 1])] == ref_inl).all(), (tag, i, j)
        seen.add(int(ref.config))
    assert want_configs & seen, (tag, seen)


def test_calibrated_scene(contexts, oracle):
    _stage_both_forms(contexts, oracle, synthetic.Scene(6, 1024, seed=21, n_pool=3072), 6, "calibrated", {2})


def test_planar_scene(contexts, oracle):
    _stage_both_forms(contexts, oracle, synthetic.Scene(6, 1024, seed=22, n_pool=3072, planar=True, planar_depth=0.0), 6,
                      "planar", {4})


def test_pure_rotation_panoramic(contexts, oracle):
    """One candidate, t = 0: max_depth is 0, so its count is 0 and it wins alone."""
    prod, full = contexts
    rng = np.random.default_rng(5)
    X = _front_points(rng, 200)
    opts = capi.default_two_view_options()
    got = _leaf_both_forms(prod, full, oracle, *_pair(X, _rot([0.2, 1.0, 0.1], 0.15), np.zeros(3), rng), opts, 9, "panoramic")
    assert got.config == 5 and got.tri_angle == 0.0


@pytest.mark.parametrize("n", [9, 12, 15, 16, 17])
def test_few_inliers(contexts, oracle, n):
    """Fewer than 16 inliers and exactly 16: the probe is the whole check; 17: one point after it."""
    prod, full = contexts
    rng = np.random.default_rng(100 + n)
    opts = capi.default_two_view_options()
    opts.min_num_inliers = 8
    X = _front_points(rng, n)
    got = _leaf_both_forms(prod, full, oracle, *_pair(X, _rot([0.1, 1.0, 0.0], 0.2), np.array([1.0, 0.1, 0.05]), rng, noise=0.0),
                           opts, 4, ("few", n))
    assert got.config == 2 and got.num_inliers == n


@pytest.mark.parametrize("n_front,n_behind", [(40, 40), (41, 40), (40, 41), (20, 20), (8, 8), (100, 100)])
def test_equal_and_near_equal_counts(contexts, oracle, n_front, n_behind):
    """Points behind both cameras satisfy the same epipolar geometry; for them the candidate with the opposite translation
    puts the triangulated point in front of both cameras.  So two candidates count n_front and n_behind: on a tie the
    later one must win, and the interleaving puts either of them ahead in the probe."""
    prod, full = contexts
    rng = np.random.default_rng(7 * n_front + n_behind)
    R, t = _rot([0.1, 1.0, 0.0], 0.2), np.array([1.0, 0.1, 0.05])
    Xf = _front_points(rng, n_front)
    # behind both cameras: camera-1 depth < 0 and camera-2 depth < 0
    Xb = -_front_points(rng, n_behind)
    assert ((Xb @ R.T + t)[:, 2] < 0).all()
    X = np.empty((n_front + n_behind, 3))
    order = rng.permutation(len(X))
    X[order[:n_front]] = Xf
    X[order[n_front:]] = Xb
    opts = capi.default_two_view_options()
    got = _leaf_both_forms(prod, full, oracle, *_pair(X, R, t, rng, noise=0.0), opts, 11, ("tie", n_front, n_behind))
    assert got.config == 2 and got.num_inliers == len(X)


@pytest.mark.parametrize("t", [[0.0, 0.0, 0.004], [0.001, 0.0, 0.004]])
def test_every_count_zero(contexts, oracle, t):
    """Motion towards a plane 5 units away by 0.004: the homography decomposition's translation (baseline over plane
    distance) is below 1 / 1000, so max_depth is below the points' depth, all four candidates count 0, nothing settles
    and the last candidate wins with tri_angle 0."""
    prod, full = contexts
    rng = np.random.default_rng(13)
    n = 120
    X = np.c_[rng.uniform(-2.0, 2.0, n), rng.uniform(-1.5, 1.5, n), np.full(n, 5.0)]
    opts = capi.default_two_view_options()
    got = _leaf_both_forms(prod, full, oracle, *_pair(X, _rot([0.0, 1.0, 0.0], 0.05), np.array(t), rng, noise=0.0), opts, 2,
                           ("zero", t))
    assert got.config == 4 and got.tri_angle == 0.0
