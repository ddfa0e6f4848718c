"""CPU-only: csrc/colpiv_norms.h, the minimal solvers' pivot norms as certified decisions, compiled for the host
(libdsm_colpiv_norms.so).  The library walks ColPivHouseholderQR over a 9 x M matrix twice -- with Eigen's exact bookkeeping
and with the certified tracker of squared norms -- and reports every decision: the pivot of each step and, per step and
column, whether the norm was recomputed directly.  Wherever the tracker says `certain`, the two traces must be identical; that
is the property the device solvers rest on (an uncertain lane runs the exact form).

The matrices are built the way the three register solvers build theirs (verify_estimators.h): 9 x 8 for the 4-point homography
(centred and normalised points), 9 x 7 for the 7-point F (pixel coordinates), 9 x 5 for the 5-point E (normalised image
coordinates), each divided by its largest entry as JacobiSVD does."""
import ctypes
import os

import numpy as np
import pytest

N_GENERIC = 100000


@pytest.fixture(scope="module")
def lib():
    from dagsfm_amd import capi
    path = os.path.join(os.path.dirname(capi.LIB_PATH), "libdsm_colpiv_norms.so")
    assert os.path.exists(path), "build first: " + path
    L = ctypes.CDLL(path)
    for fn in (L.dsm_cpn_trace_exact, L.dsm_cpn_trace_certified):
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        fn.restype = ctypes.c_int
    L.dsm_cpn_margin.restype = ctypes.c_double
    return L


def traces(lib, mats, m):
    """(pivots [n, 8], recomputes [n, 64], certain [n]) of the exact and of the certified tracker."""
    mats = np.ascontiguousarray(mats, np.float64).reshape(-1, 9 * m)
    n = mats.shape[0]
    out = []
    for fn in (lib.dsm_cpn_trace_exact, lib.dsm_cpn_trace_certified):
        pv, rc, ce = np.zeros((n, 8), np.int32), np.zeros((n, 64), np.int32), np.zeros(n, np.int32)
        assert fn(mats.ctypes.data, n, m, pv.ctypes.data, rc.ctypes.data, ce.ctypes.data) == 0
        out.append((pv, rc, ce))
    return out


def agree_where_certain(lib, mats, m):
    """Asserts the property; returns (uncertain samples, recomputes among the certain ones)."""
    (pe, re_, ce), (pc, rc, cc) = traces(lib, mats, m)
    assert ce.all()  # the exact form has nothing to be unsure of
    ok = cc != 0
    bad_p = np.flatnonzero(ok & (pe != pc).any(axis=1))
    bad_r = np.flatnonzero(ok & (re_ != rc).any(axis=1))
    assert bad_p.size == 0, "certified pivots differ from the exact ones at samples %s" % bad_p[:5]
    assert bad_r.size == 0, "certified recompute decisions differ from the exact ones at samples %s" % bad_r[:5]
    return int((~ok).sum()), int(re_[ok].sum())


def scaled(mats):
    """m / scale of JacobiSVD: by the largest absolute entry (1 where that is 0)."""
    flat = mats.reshape(mats.shape[0], -1)
    sc = np.abs(flat).max(axis=1)
    sc[sc == 0] = 1.0
    return mats / sc[:, None, None]


def h_matrices(xs):
    """xs [n, 4, 4] (x1 y1 x2 y2) -> [n, 8, 9]: column c of A^T = row c of homography_four_point_reg's A."""
    def norm(p):
        c = p.sum(axis=1) / 4
        d = p - c[:, None, :]
        rms = np.sqrt((d * d).sum(axis=2).sum(axis=1) / 4)
        with np.errstate(divide="ignore", invalid="ignore"):
            nf = np.sqrt(2.0) / rms
        return nf[:, None, None] * p + (-nf[:, None] * c)[:, None, :]
    s, d = norm(xs[:, :, 0:2]), norm(xs[:, :, 2:4])
    n = xs.shape[0]
    a = np.zeros((n, 8, 9))
    a[:, 0:4, 0], a[:, 0:4, 1], a[:, 0:4, 2] = -s[:, :, 0], -s[:, :, 1], -1
    a[:, 0:4, 6], a[:, 0:4, 7], a[:, 0:4, 8] = s[:, :, 0] * d[:, :, 0], s[:, :, 1] * d[:, :, 0], d[:, :, 0]
    a[:, 4:8, 3], a[:, 4:8, 4], a[:, 4:8, 5] = -s[:, :, 0], -s[:, :, 1], -1
    a[:, 4:8, 6], a[:, 4:8, 7], a[:, 4:8, 8] = s[:, :, 0] * d[:, :, 1], s[:, :, 1] * d[:, :, 1], d[:, :, 1]
    return scaled(a)


def ef_matrices(xs, swap):
    """xs [n, K, 4] -> [n, K, 9]: seven_point_reg's rows (swap = False) or five_point_basis_reg's (True)."""
    x0, y0, x1, y1 = xs[:, :, 0], xs[:, :, 1], xs[:, :, 2], xs[:, :, 3]
    one = np.ones_like(x0)
    if swap:  # five_point_basis_reg: x1 * x2, ...
        rows = [x0 * x1, y0 * x1, x1, x0 * y1, y0 * y1, y1, x0, y0, one]
    else:
        rows = [x1 * x0, x1 * y0, x1, y1 * x0, y1 * y0, y1, x0, y0, one]
    return scaled(np.stack(rows, axis=2))


def samples(rng, n, k, pixels):
    """Half random correspondences, half a smooth displacement of the first image's points."""
    lo, hi = (0.0, 1000.0) if pixels else (-0.6, 0.6)
    p1 = rng.uniform(lo, hi, (n, k, 2))
    p2 = rng.uniform(lo, hi, (n, k, 2))
    h = n // 2
    ang = rng.uniform(-0.3, 0.3, (h, 1))
    sc = rng.uniform(0.8, 1.25, (h, 1))
    t = rng.uniform(-0.1, 0.1, (h, 1, 2)) * (hi - lo)
    c, s = np.cos(ang), np.sin(ang)
    q = p1[:h]
    p2[:h, :, 0] = sc * (c * q[:, :, 0] - s * q[:, :, 1]) + t[:, :, 0]
    p2[:h, :, 1] = sc * (s * q[:, :, 0] + c * q[:, :, 1]) + t[:, :, 1]
    return np.concatenate([p1, p2], axis=2)


@pytest.mark.parametrize("m", [8, 7, 5])
def test_generic_samples_are_certain_and_agree(lib, m):
    rng = np.random.default_rng(1000 + m)
    if m == 8:
        mats = h_matrices(samples(rng, N_GENERIC, 4, True))
    elif m == 7:
        mats = ef_matrices(samples(rng, N_GENERIC, 7, True), False)
    else:
        mats = ef_matrices(samples(rng, N_GENERIC, 5, False), True)
    uncertain, _ = agree_where_certain(lib, mats, m)
    print("M = %d: %d of %d generic samples uncertain" % (m, uncertain, N_GENERIC))
    assert uncertain <= N_GENERIC // 100  # otherwise the test could pass by comparing nothing


def degenerate_h_samples(rng):
    out = []
    for eps in (0.0, 1e-12, 1e-10, 1e-8, 1e-6, 1e-4, 1e-2):
        n = 400
        x = samples(rng, n, 4, True)
        # three collinear points in the first image, off the line by eps
        a, b = x[:, 0, 0:2], x[:, 1, 0:2]
        lam = rng.uniform(0.2, 0.8, (n, 1))
        x[:, 2, 0:2] = a + lam * (b - a) + eps * rng.standard_normal((n, 2))
        out.append(x)
        # near-duplicate correspondences
        y = samples(rng, n, 4, True)
        y[:, 3, :] = y[:, 2, :] + eps * rng.standard_normal((n, 4))
        out.append(y)
    # exactly symmetric squares, mapped by a translation, a scaling, a quarter turn
    n = 300
    side = rng.integers(1, 200, (n, 1)).astype(np.float64)
    c = rng.integers(0, 500, (n, 1, 2)).astype(np.float64)
    corners = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float64)[None] * side[:, :, None] + c
    for k in range(3):
        sq = np.zeros((n, 4, 4))
        sq[:, :, 0:2] = corners
        sq[:, :, 2:4] = (corners + 7.0, 2.0 * corners, np.roll(corners, 1, axis=1))[k]
        out.append(sq)
    return np.concatenate(out, axis=0)


def dependent_columns(rng, base, eps_list):
    """base [n, M, 9]: the last column becomes a combination of two others plus eps * noise -- its norm collapses under the
    first reflections, which is what makes the bookkeeping recompute it."""
    out = []
    for eps in eps_list:
        a = base.copy()
        w = rng.uniform(0.3, 1.0, (a.shape[0], 2, 1))
        a[:, -1, :] = w[:, 0] * a[:, 0, :] + w[:, 1] * a[:, 1, :] + eps * rng.standard_normal((a.shape[0], 9))
        out.append(scaled(a))
    return np.concatenate(out, axis=0)


def test_degenerate_samples_agree_where_certain(lib):
    rng = np.random.default_rng(77)
    eps_list = (0.0, 1e-12, 1e-10, 1e-8, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2)
    total_uncertain = total_recomputes = 0
    sets = {
        8: [h_matrices(degenerate_h_samples(rng)), dependent_columns(rng, h_matrices(samples(rng, 300, 4, True)), eps_list)],
        7: [dependent_columns(rng, ef_matrices(samples(rng, 300, 7, True), False), eps_list)],
        5: [dependent_columns(rng, ef_matrices(samples(rng, 300, 5, False), True), eps_list)],
    }
    # columns scaled far apart (the small ones live on what cancellation leaves) and entries at the exponent guards of the
    # squared norms, 2^-500 and 2^500: inside, at and beyond them, and not finite
    for m in (8, 7, 5):
        g = rng.standard_normal((200, m, 9))
        sets[m].append(g * np.exp2(rng.integers(-30, 1, (200, m, 1)).astype(np.float64)))
        for e in (-260.0, -251.0, -250.0, -249.0, -200.0, 200.0, 249.0, 250.0, 251.0, 260.0):
            sets[m].append(rng.standard_normal((20, m, 9)) * np.exp2(e))
        mixed = rng.standard_normal((40, m, 9))
        mixed[:, 1, :] *= np.exp2(-255.0)
        mixed[:20, 2, :] = 0.0
        sets[m].append(mixed)
        bad = rng.standard_normal((4, m, 9))
        bad[0, 0, 0], bad[1, 2, 3], bad[2, 1, 1], bad[3, m - 1, 8] = np.nan, np.inf, -np.inf, np.nan
        sets[m].append(bad)
    for m, parts in sets.items():
        with np.errstate(all="ignore"):
            mats = np.concatenate(parts, axis=0)
        u, r = agree_where_certain(lib, mats, m)
        print("M = %d: %d of %d degenerate samples uncertain, %d recomputes among the certain" % (m, u, mats.shape[0], r))
        total_uncertain += u
        total_recomputes += r
    assert total_uncertain > 0, "the degenerate set must reach the uncertain side"
    assert total_recomputes > 0, "the degenerate set must recompute a norm in a certain sample"
    # what is not finite, or outside the guards, is never certified
    for m in (8, 7, 5):
        bad = np.random.default_rng(5).standard_normal((3, m, 9))
        bad[0, 0, 0] = np.nan
        bad[1] *= np.exp2(260.0)
        bad[2] *= np.exp2(-260.0)
        assert not traces(lib, bad, m)[1][2].any()


@pytest.mark.parametrize("m", [8, 7, 5])
def test_exact_ties_are_never_certified(lib, m):
    rng = np.random.default_rng(3)
    ties = []
    a = rng.standard_normal((1, m, 9))
    a[0, m - 1] = a[0, 0]  # two identical columns
    ties.append(a)
    b = rng.standard_normal((1, m, 9))
    b[0, 2] = b[0, 1] * -1.0  # a negated copy: the same squares
    ties.append(b)
    e = np.zeros((1, m, 9))
    for c in range(m):
        e[0, c, c] = 1.0  # unit columns: every norm is 1
    ties.append(e)
    z = np.zeros((1, m, 9))  # all columns zero: the pivot is a tie of zeros
    ties.append(z)
    p = rng.standard_normal((1, m, 9))
    p[0, 3] = p[0, 0] * (1.0 + 2.0 ** -50)  # inside the margin, not equal
    ties.append(p)
    (pe, re_, ce), (pc, rc, cc) = traces(lib, np.concatenate(ties, axis=0), m)
    assert not cc.any(), cc
    assert 2.0 ** -50 < lib.dsm_cpn_margin() <= 2.0 ** -40
