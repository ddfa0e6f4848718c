"""GPU: the minimal solvers' pivot norms as certified decisions (csrc/colpiv_norms.h) change no byte.

The lane-per-hypothesis solvers (k_solve<F>, k_solve<H>, k_solve_e_build) run their pivoted QR with certified pivot norms and
fall back, a wave at a time, to the exact bookkeeping.  Every case below runs the check build twice -- as it is, and with
DSM_NORMS_EXACT (the exact bookkeeping for every wave) -- and holds the TwoViewGeometry records and the inlier matches of the
two runs to be the same BYTES, and both to the CPU oracle under test_verify_gpu.tvg_equal's bar.  DSM_VERIFY_DEBUG counts the
waves of each solver and those that ran the exact form (Context.debug_solver_fallbacks)."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi, synthetic
from tests.test_verify_gpu import tvg_equal

pytestmark = pytest.mark.gpu

W, H = 1000, 750


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0, check=True)


def run(ctx, monkeypatch, exact, opts, seed, stage_filter=False):
    """verify_pairs on the context's current images and matches; (records as bytes, list of records, offsets, inlier matches,
    fallback counters)."""
    monkeypatch.setenv("DSM_VERIFY_DEBUG", "1")
    if exact:
        monkeypatch.setenv("DSM_NORMS_EXACT", "1")
    else:
        monkeypatch.delenv("DSM_NORMS_EXACT", raising=False)
    ctx.verify_pairs(opts, user_seed=seed, stage_filter=stage_filter)
    tvgs = ctx.two_view_geometries()
    raw = b"".join(ctypes.string_at(ctypes.addressof(t), ctypes.sizeof(t)) for t in tvgs)
    ioffs, im = ctx.inlier_matches()
    return raw, tvgs, ioffs.copy(), im.copy(), ctx.debug_solver_fallbacks().astype(np.int64)


def both_forms_and_oracle(ctx, oracle, monkeypatch, cams, kps, pairs, opts, seed, tag):
    """Runs both forms, asserts byte identity and oracle parity; returns (records, counters of the default run)."""
    raw_c, tv_c, io_c, im_c, cnt_c = run(ctx, monkeypatch, False, opts, seed)
    raw_e, tv_e, io_e, im_e, cnt_e = run(ctx, monkeypatch, True, opts, seed)
    assert raw_c == raw_e, (tag, "TwoViewGeometry records differ between the certified and the exact pivot norms")
    assert (io_c == io_e).all() and im_c.shape == im_e.shape and (im_c == im_e).all(), tag
    # the switch does what it says: every wave ran the exact form, and the same waves were launched
    assert (cnt_e[0:3] == cnt_e[3:6]).all() and (cnt_e[3:6] == cnt_c[3:6]).all(), (tag, cnt_c, cnt_e)
    assert (cnt_c[0:3] <= cnt_c[3:6]).all()
    offs, m = ctx.matches()
    for k, (i, j) in enumerate(pairs):
        mk = m[int(offs[k]):int(offs[k + 1])]
        ref, ref_inl = oracle.estimate_two_view_geometry(cams[i], kps[i].astype(np.float64), cams[j], kps[j].astype(np.float64), mk, opts,
                                                         capi.pair_seed(int(i), int(j), seed))
        tvg_equal(tv_c[k], ref, (tag, int(i), int(j)))
        assert (im_c[int(io_c[k]):int(io_c[k + 1])] == ref_inl).all(), (tag, int(i), int(j))
    return tv_c, cnt_c


@pytest.mark.parametrize("prior", [1, 0])
def test_small_scene_calibrated_and_not(ctx, oracle, monkeypatch, prior):
    """6 images x 256 features, exhaustive (15 pairs), calibrated (prior focal length: E, F and H run) and not (F and H)."""
    scene = synthetic.Scene(6, 256, seed=41, n_pool=384)  # (a small pool: about 40 matches per pair)
    ims = [scene.image(i) for i in range(6)]
    cams = [capi.simple_pinhole(800.0, W / 2.0, H / 2.0, W, H, prior) for _ in range(6)]
    ctx.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
    pairs = synthetic.exhaustive_pairs(6)
    ctx.match_pairs(pairs)
    tv, cnt = both_forms_and_oracle(ctx, oracle, monkeypatch, cams, [im[1] for im in ims], pairs, capi.default_two_view_options(), 17, ("scene", prior))
    assert sum(t.config > 1 for t in tv) >= 5
    assert (cnt[4:6] > 0).all() and (cnt[3] > 0) == bool(prior), cnt  # F and H ran, and E where the cameras are calibrated
    print("prior %d: waves that ran the exact form E/F/H %s of %s" % (prior, cnt[0:3].tolist(), cnt[3:6].tolist()))


def planted_pair(rng, kind):
    """About 40 matches between two keypoint sets related by a mild homography, with structure that makes four- and seven-point
    samples degenerate: collinear runs, duplicated keypoints, an axis-aligned square grid."""
    if kind == "collinear":  # three runs of 12 points on lines, plus a few scattered ones
        p = []
        for d in ((16.0, 0.0), (0.0, 16.0), (12.0, 16.0)):  # whole numbers: exactly collinear as float32 keypoints too
            a = np.floor(rng.uniform(100, 400, 2))
            p.append(a + np.arange(12)[:, None] * np.array(d))
        p.append(rng.uniform(50, 700, (5, 2)))
        p1 = np.concatenate(p)
    elif kind == "duplicates":  # 14 distinct keypoints, each three times
        p1 = np.repeat(rng.uniform(50, 700, (14, 2)), 3, axis=0)
    else:  # a 6 x 7 grid with integer coordinates, axis-aligned
        gx, gy = np.meshgrid(np.arange(6) * 64.0 + 128.0, np.arange(7) * 64.0 + 64.0)
        p1 = np.stack([gx.ravel(), gy.ravel()], axis=1)
    if kind == "grid":
        p2 = p1 + np.array([32.0, 16.0])  # an exact translation: squares map to squares, norms tie
    else:
        Hm = np.array([[1.02, 0.03, 12.0], [-0.02, 0.99, -7.0], [2e-5, -1e-5, 1.0]])
        q = np.concatenate([p1, np.ones((len(p1), 1))], axis=1) @ Hm.T
        p2 = q[:, :2] / q[:, 2:3]
    kp1, kp2 = p1.astype(np.float32), p2.astype(np.float32)
    m = np.stack([np.arange(len(kp1)), np.arange(len(kp1))], axis=1).astype(np.uint32)
    return kp1, kp2, m


def test_planted_degenerate_samples_take_the_fallback(ctx, oracle, monkeypatch):
    """3 pairs x about 40 matches whose minimal samples are often degenerate (collinear triples, repeated points, exact squares):
    the H solver must hit the fallback, and nothing may change."""
    rng = np.random.default_rng(8)
    kps, cams, pairs, matches = [], [], [], []
    for k, kind in enumerate(("collinear", "duplicates", "grid")):
        kp1, kp2, m = planted_pair(rng, kind)
        kps += [kp1, kp2]
        cams += [capi.simple_pinhole(800.0, W / 2.0, H / 2.0, W, H, 1)] * 2
        pairs.append((2 * k, 2 * k + 1))
        matches.append(m)
    ctx.set_images([np.zeros((len(kp), 128), np.uint8) for kp in kps], kps, cams)
    ctx.set_matches(np.array(pairs, np.uint32), matches)
    tv, cnt = both_forms_and_oracle(ctx, oracle, monkeypatch, cams, kps, np.array(pairs), capi.default_two_view_options(), 5, "planted")
    print("planted: waves that ran the exact form E/F/H %s of %s" % (cnt[0:3].tolist(), cnt[3:6].tolist()))
    assert cnt[2] > 0, "no H wave took the fallback: the planted samples are not degenerate enough"


def test_waves_with_lanes_without_a_trial(ctx, oracle, monkeypatch):
    """One pair with 8 matches and one with 3 (fewer than any minimal sample but the translation's): partial waves, and a pair
    whose families do not run at all."""
    scene = synthetic.Scene(2, 256, seed=3)
    a, b = scene.image(0), scene.image(1)
    m_all = oracle.match_sift_features_cpu(a[0], b[0])
    assert len(m_all) >= 8
    kps = [a[1], b[1], a[1], b[1]]
    cams = [capi.simple_pinhole(800.0, W / 2.0, H / 2.0, W, H, 1)] * 4
    pairs = np.array([(0, 1), (2, 3)], np.uint32)
    ctx.set_images([a[0], b[0], a[0], b[0]], kps, cams)
    ctx.set_matches(pairs, [m_all[:8], m_all[:3]])
    opts = capi.default_two_view_options(min_num_inliers=4)
    both_forms_and_oracle(ctx, oracle, monkeypatch, cams, kps, pairs, opts, 23, "partial waves")


def test_compact_grid_of_later_rounds(ctx, oracle, monkeypatch):
    """300 pairs x 64 features at a low inlier ratio: E and F go beyond their first round, where the solvers take 64 hypotheses
    per wave across the pairs (k_solve<F, true>, k_solve_e_build<true>)."""
    n_img = 25
    scene = synthetic.Scene(n_img, 64, seed=77, outlier_frac=0.5, n_pool=96)  # (about 10 matches per pair)
    ims = [scene.image(i) for i in range(n_img)]
    cams = [capi.simple_pinhole(800.0, W / 2.0, H / 2.0, W, H, 1) for _ in range(n_img)]
    ctx.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
    pairs = synthetic.exhaustive_pairs(n_img)
    assert len(pairs) == 300
    ctx.match_pairs(pairs)
    tv, cnt = both_forms_and_oracle(ctx, oracle, monkeypatch, cams, [im[1] for im in ims], pairs, capi.default_two_view_options(), 9, "compact")
    assert any(t.num_trials[0] > 64 for t in tv) and any(t.num_trials[1] > 128 for t in tv), "no pair went beyond the first round of E and of F"
    print("compact: waves that ran the exact form E/F/H %s of %s" % (cnt[0:3].tolist(), cnt[3:6].tolist()))
