"""The bound steps' packed-f32 loops (k_prescore_h2, k_prescore_compact2) after their per-pair set-up moved into
k_verify_prep and their loops were trimmed: every case runs the check build with the product's loops (DSM_SCORE_PREFILTER=1) and with
the loops as they were before (=65: in-kernel staging, both bounds counted, the odd last point tested on every trip) and holds

  * the TwoViewGeometry records and the inlier matches of the two to be the same bytes,
  * both to be the oracle's (tests/test_verify_gpu.py::tvg_equal),
  * under =check / =check65 (every slot scored exactly and held against its bounds) the number of slots the filter skips -- counter
    [15] -- to be the same, i.e. the same bounds skip the same slots, and no bound to be violated (counter [14]).

The shapes are the smallest at which the new code takes another path: an odd last point and fewer trips than an unrolled group
(1 .. 8 matches), groups + single trips + odd tail (around 40), the LDS limit VP_LDS_PTS = 1 536, lists that pass PRESCORE_LIST_CAP
(planar scene: the H step redoes the lane in FP64; a loose threshold on an 8 192-feature pair: the E / F stretches end on the cap),
the f32 stage switched off (threshold 0.1 px, coordinates x 40), a second call on the same context (the per-pair buffer must be
rewritten) and multiple_models (the points change between the passes)."""
import ctypes
import os

import numpy as np
import pytest

from dagsfm_amd import capi, synthetic
from tests.test_verify_gpu import tvg_equal

pytestmark = pytest.mark.gpu

VP_LDS_PTS = 1536  # csrc/verify_kernels.hip
W, H, FOCAL = 1000, 750, 800.0


def _rot(rng, mag):
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * rng.uniform(0.1, mag)
    th = np.linalg.norm(a)
    k = a / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _problem(seed, n, planar=False, noise=0.5, outlier_frac=0.2, scale=1.0, two_motions=False):
    """n correspondences of a rigid scene seen by two pinhole cameras: (kp1, kp2 float32 [n, 2], matches uint32 [n, 2])."""
    rng = np.random.default_rng(seed)
    X = np.c_[rng.uniform(-1.5, 1.5, n), rng.uniform(-1.1, 1.1, n), rng.uniform(3.0, 7.0, n)]
    if planar:
        X[:, 2] = 5.0 - 0.15 * X[:, 0] + 0.1 * X[:, 1]
    R, t = _rot(rng, 0.3), rng.normal(size=3) * 0.4
    Y = X @ R.T + t
    if two_motions:
        g = np.arange(n) % 5 < 2
        Y[g] = X[g] @ _rot(rng, 0.3).T + rng.normal(size=3) * 0.6
    p1 = np.c_[FOCAL * X[:, 0] / X[:, 2] + W / 2, FOCAL * X[:, 1] / X[:, 2] + H / 2] + rng.normal(scale=noise, size=(n, 2))
    p2 = np.c_[FOCAL * Y[:, 0] / Y[:, 2] + W / 2, FOCAL * Y[:, 1] / Y[:, 2] + H / 2] + rng.normal(scale=noise, size=(n, 2))
    k = int(outlier_frac * n)
    if k:
        sel = rng.choice(n, k, replace=False)
        p2[sel] = np.c_[rng.uniform(0, W, k), rng.uniform(0, H, k)]
    m = np.stack([np.arange(n), np.arange(n)], axis=1).astype(np.uint32)
    return (p1 * scale).astype(np.float32), (p2 * scale).astype(np.float32), m


def _camera(prior, scale=1.0):
    return capi.simple_pinhole(FOCAL * scale, W / 2.0 * scale, H / 2.0 * scale, int(W * scale), int(H * scale), prior)


@pytest.fixture(scope="module")
def check_ctx():
    ctx = capi.Context(0, check=True)
    yield ctx
    ctx.close()


def _install(ctx, problems, cam):
    """problems: [(kp1, kp2, matches)] -> images 2 k, 2 k + 1 and pair k of the context, the given matches installed."""
    descs, kps, pairs = [], [], []
    for k, (kp1, kp2, _) in enumerate(problems):
        for kp in (kp1, kp2):
            descs.append(np.zeros((len(kp), 128), np.uint8))
            kps.append(kp)
        pairs.append((2 * k, 2 * k + 1))
    ctx.set_images(descs, kps, [cam] * len(kps))
    ctx.set_matches(np.array(pairs, np.uint32), [p[2] for p in problems])
    return pairs


def _verify(ctx, opts, mode, monkeypatch, user_seed=3):
    monkeypatch.setenv("DSM_SCORE_PREFILTER", mode)
    ctx.verify_pairs(opts, user_seed=user_seed, stage_filter=False)
    recs = np.zeros((ctx.n_pairs, ctypes.sizeof(capi.TwoViewGeometry)), dtype=np.uint8)
    assert ctx._L.dsm_get_two_view_geometries(ctx._h, recs.ctypes.data) == 0
    ioffs, inl = ctx.inlier_matches()
    return recs, np.array(ioffs).copy(), np.array(inl).copy(), ctx.two_view_geometries(), ctx.debug_verify_counters().copy()


def _hold(ctx, oracle, monkeypatch, kps, cams, pairs, matches, opts, tag, user_seed=3):
    """The four runs of a pair list that is installed on the context, and what the module's docstring asks of them."""
    new = _verify(ctx, opts, "1", monkeypatch, user_seed)
    old = _verify(ctx, opts, "65", monkeypatch, user_seed)
    assert (new[0] == old[0]).all(), (tag, "records", np.nonzero((new[0] != old[0]).any(axis=1))[0][:8])
    assert (new[1] == old[1]).all() and new[2].shape == old[2].shape and (new[2] == old[2]).all(), (tag, "inlier matches")
    n_geo = 0
    for k, (i, j) in enumerate(pairs):
        ref, ref_inl = oracle.estimate_two_view_geometry(cams[i], kps[i].astype(np.float64), cams[j], kps[j].astype(np.float64),
                                                         matches[k], opts, capi.pair_seed(int(i), int(j), user_seed))
        for got in (new, old):
            tvg_equal(got[3][k], ref, (tag, k))
            assert (got[2][int(got[1][k]):int(got[1][k + 1])] == ref_inl).all(), (tag, k)
        n_geo += ref.config > 1
    chk_new = _verify(ctx, opts, "check", monkeypatch, user_seed)
    chk_old = _verify(ctx, opts, "check65", monkeypatch, user_seed)
    print("%s: pairs %d, with geometry %d, slots skipped %d (staged loops %d), bounds violated %d (%d)"
          % (tag, len(pairs), n_geo, chk_new[4][15], chk_old[4][15], chk_new[4][14], chk_old[4][14]))
    assert (chk_new[0] == new[0]).all() and (chk_old[0] == new[0]).all(), (tag, "the checking schedule's records")
    assert int(chk_new[4][15]) == int(chk_old[4][15]), (tag, "slots never scored exactly", int(chk_new[4][15]), int(chk_old[4][15]))
    assert int(chk_new[4][14]) == 0 and int(chk_old[4][14]) == 0, (tag, "bounds violated", int(chk_new[4][14]), int(chk_old[4][14]))
    return n_geo, int(chk_new[4][15])


def _hold_problems(ctx, oracle, monkeypatch, problems, prior, opts, tag, scale=1.0):
    cam = _camera(prior, scale)
    pairs = _install(ctx, problems, cam)
    kps = [kp for p in problems for kp in p[:2]]
    return _hold(ctx, oracle, monkeypatch, kps, [cam] * len(kps), pairs, [p[2] for p in problems], opts, tag)


@pytest.mark.parametrize("prior", [0, 1])
def test_few_matches_and_odd_tails(check_ctx, oracle, monkeypatch, prior):
    """1, 2, 3, 7, 8 matches: nothing but the odd last point, a single trip, fewer trips than a group; 39 .. 46: whole groups of the H
    loop (8 trips) and of the E / F loop (4), single trips behind them, with and without an odd last point."""
    opts = capi.default_two_view_options(min_num_inliers=4)
    problems = [_problem(100 + n, n, noise=0.3, outlier_frac=0.0) for n in (1, 2, 3, 7, 8)]
    problems += [_problem(200 + n, n, noise=0.5, outlier_frac=0.2) for n in (39, 40, 41, 46)]
    n_geo, skipped = _hold_problems(check_ctx, oracle, monkeypatch, problems, prior, opts, ("few", prior))
    assert n_geo >= 5 and skipped > 0


def test_pairs_around_the_lds_limit(check_ctx, oracle, monkeypatch):
    """VP_LDS_PTS - 1 and VP_LDS_PTS matches (odd and even: the records fill the LDS), VP_LDS_PTS + 1 (the FP64 loop over global
    memory, its maxima from the per-pair buffer)."""
    opts = capi.default_two_view_options()
    problems = [_problem(300 + d, VP_LDS_PTS + d, noise=0.7, outlier_frac=0.3) for d in (-1, 0, 1)]
    n_geo, skipped = _hold_problems(check_ctx, oracle, monkeypatch, problems, 1, opts, "lds")
    assert n_geo == 3 and skipped > 0


def test_planar_scene_overflows_the_h_lists(check_ctx, oracle, monkeypatch):
    """~1 000 matches on a plane with noise of the order of the threshold: the residuals of most homographies sit near it, lists of
    every length up to and beyond PRESCORE_LIST_CAP (the lane redoes its points in FP64), drains 1, 2 and 4 wide."""
    opts = capi.default_two_view_options()
    problems = [_problem(400, 1001, planar=True, noise=1.6, outlier_frac=0.15), _problem(401, 1000, planar=True, noise=0.4, outlier_frac=0.3)]
    for prior in (0, 1):
        n_geo, skipped = _hold_problems(check_ctx, oracle, monkeypatch, problems, prior, opts, ("planar", prior))
        assert n_geo == 2 and skipped > 0


def test_loose_threshold_ends_stretches_on_the_cap(check_ctx, oracle, monkeypatch):
    """An 8 192-feature pair (about 500 matches) at max_error 12: dozens of points per model inside the E / F band, the stretches of
    the packed loop end on the list cap (tested once per group of trips) and go on behind a drain."""
    scene = synthetic.Scene(2, 8192, seed=7)
    ims = [scene.image(i) for i in range(2)]
    opts = capi.default_two_view_options(max_error=12.0)
    for prior in (1, 0):
        cams = [capi.simple_pinhole(scene.focal, scene.width / 2.0, scene.height / 2.0, scene.width, scene.height, prior) for _ in range(2)]
        monkeypatch.delenv("DSM_SCORE_PREFILTER", raising=False)
        check_ctx.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
        pairs = synthetic.exhaustive_pairs(2)
        check_ctx.match_pairs(pairs)
        offs, m = check_ctx.matches()
        assert 300 < len(m) < 1200, len(m)
        n_geo, skipped = _hold(check_ctx, oracle, monkeypatch, [im[1] for im in ims], cams, pairs, [np.array(m).copy()], opts, ("loose", prior))
        assert n_geo == 1 and skipped > 0


@pytest.mark.parametrize("scale,max_error", [(1.0, 0.1), (40.0, 160.0)])
def test_f32_stage_switched_off(check_ctx, oracle, monkeypatch, scale, max_error):
    """A threshold below the bounds' range and coordinates beyond 2^14 px: the band's constants never classify a point, every point is
    listed (E / F: stretch after stretch; H: overflow) -- the loops must still count as before."""
    opts = capi.default_two_view_options(max_error=max_error)
    problems = [_problem(500, 257, noise=0.05 if scale == 1.0 else 0.5, outlier_frac=0.2, scale=scale),
                _problem(501, 64, planar=True, noise=0.05 if scale == 1.0 else 0.5, outlier_frac=0.2, scale=scale)]
    for prior in (0, 1):
        n_geo, _ = _hold_problems(check_ctx, oracle, monkeypatch, problems, prior, opts, ("off", scale, prior), scale=scale)
        assert n_geo >= 1


def test_second_call_rewrites_the_per_pair_buffer(check_ctx, oracle, monkeypatch):
    """Other images behind the same pair list and the same match counts: what k_verify_prep wrote for the first call must not be read
    by the second (a stale maximum or record would move the bounds)."""
    opts = capi.default_two_view_options()
    first = [_problem(600 + k, n, noise=0.5, outlier_frac=0.2) for k, n in enumerate((255, 300))]
    second = [_problem(700 + k, n, planar=bool(k), noise=1.0, outlier_frac=0.3, scale=3.0) for k, n in enumerate((255, 300))]
    _hold_problems(check_ctx, oracle, monkeypatch, first, 1, opts, "first call")
    n_geo, skipped = _hold_problems(check_ctx, oracle, monkeypatch, second, 1, opts, "second call", scale=3.0)
    assert n_geo == 2 and skipped > 0


@pytest.mark.parametrize("prior", [0, 1])
def test_multiple_models_changes_the_points_between_passes(check_ctx, oracle, monkeypatch, prior):
    """EstimateMultiple on one pair with two motions: every pass verifies the matches the passes before it left over, so the pair's
    points, maxima and count change from pass to pass."""
    opts = capi.default_two_view_options()
    opts.multiple_models = 1
    cam = _camera(prior)
    kp1, kp2, m = _problem(800, 301, noise=0.5, outlier_frac=0.1, two_motions=True)
    ref, ref_inl = oracle.estimate_two_view_geometry(cam, kp1.astype(np.float64), cam, kp2.astype(np.float64), m, opts, 19)
    assert ref.config == 8, ref.config  # MULTIPLE
    got = {}
    for mode in ("1", "65"):
        monkeypatch.setenv("DSM_SCORE_PREFILTER", mode)
        tv, inl = check_ctx.estimate_two_view_geometry(cam, kp1.astype(np.float64), cam, kp2.astype(np.float64), m, opts, 19)
        tvg_equal(tv, ref, ("multiple", prior, mode))
        assert (inl == ref_inl).all()
        got[mode] = (bytes(tv), inl)
    assert got["1"][0] == got["65"][0] and (got["1"][1] == got["65"][1]).all()
    # and through the stage call, next to a pair that ends after its first pass
    problems = [(kp1, kp2, m), _problem(801, 120, noise=0.5, outlier_frac=0.2)]
    _hold_problems(check_ctx, oracle, monkeypatch, problems, prior, opts, ("multiple stage", prior))
