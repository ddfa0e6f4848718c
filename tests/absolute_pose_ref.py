"""Sequential numpy restatement of EstimateAbsolutePose (src/estimators/pose.cc:48-158): LORANSAC<P3PEstimator, EPNPEstimator>
(src/optim/loransac.h:91-233, src/estimators/absolute_pose.cc:47-609) per focal-length factor, written without the device's
batches -- what tests/test_absolute_pose_*.py compare dsm_estimate_absolute_poses with.

TEST INFRASTRUCTURE ONLY.  The blocks the oracle library already pins to the reference are called through tests/oracle_lib.py
(jacobi_svd, poly_roots, image_to_world, sample_sequence, rotation_to_quaternion, and -- bound here from the loaded handle --
oracle_inlier_support, oracle_image_to_world_threshold).  What they do not cover is written out in the device's operation order:
the pivoted QR with its permutation, the 6 x k SVD solve, the 3-point Umeyama, the polynomial arithmetic, and EPnP's sums
over the points (a fixed-order tree: 64 interleaved partial sums, then the xor butterfly 32 .. 1; a point outside the input
set adds +0.0).

Every decision a rounding difference could flip records its margin (MARGINS, the order of dsm_absolute_pose_report.min_margin).
"""
import ctypes
import math

import numpy as np

from dagsfm_amd import capi
from tests import oracle_lib

EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
DBL_MIN = float(np.finfo(np.float64).tiny)
MARGINS = capi.ABSOLUTE_POSE_MARGINS
M_RES, M_DEPTH, M_TIE, M_IMAG, M_SIGN, M_RANK, M_BETA, M_ERR, M_DET = range(9)
CLEAR_MARGIN = 1e-9
SATURATED = 1e150   # an EPnP total error that holds a point behind the camera (sqrt(DBL_MAX) = 1.3e154 per point)
SAME_MODEL = 1e-10  # two EPnP candidates closer than this (max-abs, relative) count as one in the comparison margin
# A swap between two such candidates moves the model by up to SAME_MODEL, a projected point by about as much, and a residual r
# by 2 SAME_MODEL / sqrt(r) relative.  At the threshold sqrt(r) = max_error / focal, at least 12 / 24000 = 5e-4 over the test
# scenes (the largest focal length a sweep tries is 10 x 2400), so the change is below 4e-7: a problem is clear only if its
# residual and support-tie margins also stay above SWAP_BAR.
SWAP_BAR = 1e-6
MAX_TRIALS = 1000000  # DSM_ABSOLUTE_POSE_MAX_TRIALS

DEFAULTS = dict(num_focal_length_samples=30, min_focal_length_ratio=0.1, max_focal_length_ratio=10.0, max_error=12.0,
                min_inlier_ratio=0.25, confidence=0.9999, min_num_trials=30, max_num_trials=2 ** 64 - 1, random_seed=0)

_f64p = ctypes.POINTER(ctypes.c_double)
_bound = False


def _orc():
    global _bound
    o = oracle_lib.load()
    if not _bound:
        L = o.lib
        L.oracle_inlier_support.restype = None
        L.oracle_inlier_support.argtypes = [_f64p, ctypes.c_uint64, ctypes.c_double, ctypes.POINTER(ctypes.c_uint64), _f64p]
        L.oracle_image_to_world_threshold.restype = ctypes.c_double
        L.oracle_image_to_world_threshold.argtypes = [ctypes.POINTER(capi.Camera), ctypes.c_double]
        _bound = True
    return o


def inlier_support(residuals, max_residual):
    """InlierSupportMeasurer::Evaluate: the count and the in-order residual sum of the inliers."""
    r = np.ascontiguousarray(residuals, np.float64)
    n, s = ctypes.c_uint64(0), ctypes.c_double(0)
    _orc().lib.oracle_inlier_support(r.ctypes.data_as(_f64p), len(r), max_residual, ctypes.byref(n), ctypes.byref(s))
    return int(n.value), float(s.value)


# ------------------------------------------------------------------------------------------------ item 1: the factors
def focal_length_factors(num_samples=30, min_ratio=0.1, max_ratio=10.0):
    """pose.cc:92-98, the loop as written: its length is decided by the accumulated rounding of f += fstep."""
    fstep = 1.0 / num_samples
    fscale = max_ratio - min_ratio
    out = []
    f = 0.0
    while f <= 1.0:
        out.append(min_ratio + fscale * f * f)
        f += fstep
    return out


def compute_num_trials(num_inliers, num_samples, confidence):
    """RANSAC::ComputeNumTrials (ransac.h:151-167), kMinNumSamples = 3; no inlier (ceil(-inf)) and a confidence of 1 mean
    'never below the trial count', as the device's table has it."""
    ratio = num_inliers / float(num_samples)
    nom = 1 - confidence
    if nom <= 0:
        return 2 ** 32 - 1
    denom = 1 - math.pow(ratio, 3)
    if denom <= 0:
        return 1
    ld = math.log(denom)
    if ld == 0:
        return 2 ** 32 - 1
    v = math.ceil(math.log(nom) / ld)
    return 2 ** 32 - 1 if (not v >= 0 or v >= 4294967295.0) else int(v)


def max_num_trials(opts):
    """RANSAC's constructor (ransac.h:141-147)."""
    dyn = compute_num_trials(int(opts["min_inlier_ratio"] * 100000), 100000, opts["confidence"])
    return opts["max_num_trials"] if dyn == 2 ** 32 - 1 else min(opts["max_num_trials"], dyn)


# ------------------------------------------------------------------------------------------------ small linear algebra
def det3(m):
    """Eigen's 3 x 3 determinant (bruteforce_det3_helper order)."""
    m = np.asarray(m, np.float64).reshape(9)
    return float(m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2]))


def inverse3(M):
    """Eigen's 3 x 3 inverse by cofactors (the device's m3_inverse)."""
    M = np.asarray(M, np.float64)

    def cof(i, j):
        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
        return M[i1, j1] * M[i2, j2] - M[i1, j2] * M[i2, j1]
    c00, c10, c20 = cof(0, 0), cof(1, 0), cof(2, 0)
    det = c00 * M[0, 0] + c10 * M[1, 0] + c20 * M[2, 0]
    invdet = 1.0 / det
    R = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            R[r, c] = cof(c, r) * invdet
    return R


def make_householder(x):
    """Eigen's makeHouseholderInPlace on x (modified): returns tau, beta."""
    tail_sq = 0.0
    for i in range(1, len(x)):
        tail_sq += x[i] * x[i]
    c0 = x[0]
    if tail_sq <= DBL_MIN:
        x[1:] = 0.0
        return 0.0, c0
    b = math.sqrt(c0 * c0 + tail_sq)
    if c0 >= 0.0:
        b = -b
    for i in range(1, len(x)):
        x[i] = x[i] / (c0 - b)
    return (b - c0) / b, b


def colpiv_qr(A):
    """ColPivHouseholderQR::computeInPlace: returns qr (the reflectors below the diagonal), hcoeffs, perm (the original column at
    each position) and nonzeroPivots()."""
    qr = np.array(A, np.float64)
    rows, cols = qr.shape
    nu, nd = np.zeros(cols), np.zeros(cols)
    for k in range(cols):
        s = 0.0
        for i in range(rows):
            s += qr[i, k] * qr[i, k]
        nu[k] = nd[k] = math.sqrt(s)
    perm = list(range(cols))
    maxn = float(max(nu)) if cols else 0.0
    thr_helper = (maxn * EPS) * (maxn * EPS) / float(rows)
    downdate = math.sqrt(EPS)
    nzp = cols
    hco = np.zeros(cols)
    for k in range(cols):
        big, mx = k, nu[k]
        for j in range(k + 1, cols):
            if nu[j] > mx:
                mx, big = nu[j], j
        if nzp == cols and mx * mx < thr_helper * float(rows - k):
            nzp = k
        if k != big:
            qr[:, [k, big]] = qr[:, [big, k]]
            nu[k], nu[big] = nu[big], nu[k]
            nd[k], nd[big] = nd[big], nd[k]
            perm[k], perm[big] = perm[big], perm[k]
        col = qr[k:, k].copy()
        tau, beta = make_householder(col)
        qr[k:, k] = col
        hco[k] = tau
        qr[k, k] = beta
        nr = rows - k
        ess = qr[k + 1:, k]
        for j in range(k + 1, cols):  # apply_householder_left
            if nr == 1:
                qr[k, j] *= (1.0 - tau)
            elif tau != 0.0:
                tmp = 0.0
                for i in range(1, nr):
                    tmp += ess[i - 1] * qr[k + i, j]
                tmp += qr[k, j]
                qr[k, j] -= tau * tmp
                for i in range(1, nr):
                    qr[k + i, j] -= tau * ess[i - 1] * tmp
        for j in range(k + 1, cols):
            if nu[j] != 0.0:
                temp = abs(qr[k, j]) / nu[j]
                temp = (1.0 + temp) * (1.0 - temp)
                temp = 0.0 if temp < 0.0 else temp
                ratio = nu[j] / nd[j]
                temp2 = temp * (ratio * ratio)
                if temp2 <= downdate:
                    s = 0.0
                    for i in range(k + 1, rows):
                        s += qr[i, j] * qr[i, j]
                    nd[j] = nu[j] = math.sqrt(s)
                else:
                    nu[j] *= math.sqrt(temp)
    return qr, hco, perm, nzp


def apply_qt(qr, hco, b):
    rows, cols = qr.shape
    c = np.array(b, np.float64)
    for k in range(cols):
        nr, tau = rows - k, hco[k]
        if nr == 1:
            c[k] *= (1.0 - tau)
        elif tau != 0.0:
            tmp = 0.0
            for i in range(1, nr):
                tmp += qr[k + i, k] * c[k + i]
            tmp += c[k]
            c[k] -= tau * tmp
            for i in range(1, nr):
                c[k + i] -= tau * qr[k + i, k] * tmp
    return c


def qr_solve(A, b):
    """A.colPivHouseholderQr().solve(b)."""
    qr, hco, perm, nzp = colpiv_qr(A)
    c = apply_qt(qr, hco, b)
    for i in range(nzp - 1, -1, -1):
        s = c[i]
        for j in range(i + 1, nzp):
            s -= qr[i, j] * c[j]
        c[i] = s / qr[i, i]
    x = np.zeros(A.shape[1])
    for i in range(nzp):
        x[perm[i]] = c[i]
    return x


def svd_solve_tall(A, b):
    """JacobiSVD<6 x K>(A).solve(b): the pivoted QR preconditioner of A / max|A|, the Jacobi sweeps on its K x K triangle (the
    oracle's jacobi_svd), then V_r diag(1 / s) U_r^T (Q^T b) over the numerical rank."""
    A = np.asarray(A, np.float64)
    K = A.shape[1]
    scale = float(np.max(np.abs(A)))
    if scale == 0.0:
        scale = 1.0
    qr, hco, perm, _ = colpiv_qr(A / scale)
    R = np.triu(qr[:K, :K])
    U, sv, V = _orc().jacobi_svd(R)
    c = apply_qt(qr, hco, b)
    t0 = sv[0] * (K * EPS)
    thr = t0 if t0 > DBL_MIN else DBL_MIN
    rank = K
    while rank > 0 and sv[rank - 1] < thr:
        rank -= 1
    tmp = np.zeros(rank)
    for j in range(rank):
        s = 0.0
        for i in range(K):
            s += U[i, j] * c[i]
        tmp[j] = (1.0 / (sv[j] * scale)) * s
    x = np.zeros(K)
    for i in range(K):
        s = 0.0
        for j in range(rank):
            s += V[i, j] * tmp[j]
        x[perm[i]] = s
    return x


def tree_sum(terms, mask=None):
    """The fixed-order sum over the points: terms [N] or [N, C]; lane l accumulates points l, l + 64, ... in order from 0.0, the 64
    partial sums are combined by the xor butterfly 32, 16, ..., 1.  mask == 0 adds +0.0."""
    t = np.asarray(terms, np.float64)
    one = t.ndim == 1
    if one:
        t = t[:, None]
    if mask is not None:
        t = np.where(np.asarray(mask, bool)[:, None], t, 0.0)
    n, c = t.shape
    rows = (n + 63) // 64
    pad = np.zeros((rows * 64, c))
    pad[:n] = t
    pad = pad.reshape(rows, 64, c)
    acc = np.zeros((64, c))
    for r in range(rows):
        if r == rows - 1 and n % 64:
            k = n % 64
            acc[:k] = acc[:k] + pad[r, :k]  # lanes beyond the end add nothing
        else:
            acc = acc + pad[r]
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[idx ^ o]
    return float(acc[0, 0]) if one else acc[0].copy()


# ------------------------------------------------------------------------------------------------ residuals
def residuals(P, x, X, margins=None):
    """ComputeSquaredReprojectionError (src/estimators/utils.cc:133-180); a point at depth <= epsilon gets the maximum."""
    P = np.asarray(P, np.float64).reshape(3, 4)
    X0, X1, X2 = X[:, 0], X[:, 1], X[:, 2]
    pz = P[2, 0] * X0 + P[2, 1] * X1 + P[2, 2] * X2 + P[2, 3]
    with np.errstate(all="ignore"):
        if margins is not None and len(pz):
            apz = np.abs(pz)
            m = np.abs(pz - EPS) / np.where(apz > EPS, apz, EPS)
            m = m[~np.isnan(m)]
            if len(m):
                margins[M_DEPTH] = min(margins[M_DEPTH], float(m.min()))
        front = pz > EPS
        px = P[0, 0] * X0 + P[0, 1] * X1 + P[0, 2] * X2 + P[0, 3]
        py = P[1, 0] * X0 + P[1, 1] * X1 + P[1, 2] * X2 + P[1, 3]
        inv = 1.0 / pz
        dx = x[:, 0] - px * inv
        dy = x[:, 1] - py * inv
        r = np.where(front, dx * dx + dy * dy, DBL_MAX)
    return r


def _res_margin(r, thr, margins):
    ok = r != DBL_MAX
    if ok.any():
        m = np.abs(r[ok] - thr) / thr
        m = m[~np.isnan(m)]
        if len(m):
            margins[M_RES] = min(margins[M_RES], float(m.min()))


# ------------------------------------------------------------------------------------------------ item 3: P3P
def umeyama3(src, dst):
    """Eigen::umeyama(src, dst, false) of three points (rows), 3 x 4."""
    third = 1.0 / 3.0
    ms = ((src[0] + src[1]) + src[2]) * third
    md = ((dst[0] + dst[1]) + dst[2]) * third
    sig = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            sig[i, j] = ((third * (dst[0][i] - md[i])) * (src[0][j] - ms[j]) + (third * (dst[1][i] - md[i])) * (src[1][j] - ms[j])) + \
                (third * (dst[2][i] - md[i])) * (src[2][j] - ms[j])
    U, _, V = _orc().jacobi_svd(sig)
    S = [1.0, 1.0, 1.0]
    if det3(U) * det3(V) < 0.0:
        S[2] = -1.0
    out = np.zeros((3, 4))
    for i in range(3):
        for j in range(3):
            out[i, j] = ((U[i, 0] * S[0]) * V[j, 0] + (U[i, 1] * S[1]) * V[j, 1]) + (U[i, 2] * S[2]) * V[j, 2]
        out[i, 3] = md[i] - ((out[i, 0] * ms[0] + out[i, 1] * ms[1]) + out[i, 2] * ms[2])
    return out


def p3p(x, Xw, margins=None):
    """P3PEstimator::Estimate (absolute_pose.cc:47-174): x [3, 2] normalised image points, Xw [3, 3]; up to four 3 x 4 models."""
    mg = margins if margins is not None else [math.inf] * 9
    x = [[float(v) for v in row] for row in x]
    Xw = np.asarray(Xw, np.float64)
    uvw = []
    for k in range(3):
        s = math.sqrt((x[k][0] * x[k][0] + x[k][1] * x[k][1]) + 1)
        uvw.append((x[k][0] / s, x[k][1] / s, 1.0 / s))
    u, v, w = uvw
    cos_uv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]
    cos_uw = (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]
    cos_vw = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2]

    def d2(i, j):
        a0, a1, a2 = float(Xw[i][0] - Xw[j][0]), float(Xw[i][1] - Xw[j][1]), float(Xw[i][2] - Xw[j][2])
        return (a0 * a0 + a1 * a1) + a2 * a2
    dist_AB_2, dist_AC_2, dist_BC_2 = d2(0, 1), d2(0, 2), d2(1, 2)
    if dist_AB_2 == 0.0:
        return []  # a / b are not finite: the eigen-solver fails on the NaN matrix
    dist_AB = math.sqrt(dist_AB_2)
    a = dist_BC_2 / dist_AB_2
    b = dist_AC_2 / dist_AB_2
    a2 = a * a
    b2 = b * b
    p = 2 * cos_vw
    q = 2 * cos_uw
    r = 2 * cos_uv
    p2 = p * p
    p3 = p2 * p
    q2 = q * q
    r2 = r * r
    r3 = r2 * r
    r4 = r3 * r
    r5 = r4 * r
    coeffs = [0.0] * 5
    coeffs[0] = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a
    coeffs[1] = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q
    coeffs[2] = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2
    coeffs[3] = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q
    coeffs[4] = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1
    if not all(math.isfinite(c) for c in coeffs):
        return []
    re, im = _orc().poly_roots(coeffs)
    if re is None:
        return []
    models = []
    for i in range(len(re)):
        mg[M_IMAG] = min(mg[M_IMAG], abs(abs(im[i]) - 1e-10) / 1e-10)
        if abs(im[i]) > 1e-10:
            continue
        x_ = float(re[i])
        mg[M_SIGN] = min(mg[M_SIGN], abs(x_))
        if x_ < 0:
            continue
        x2 = x_ * x_
        x3 = x2 * x_
        bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2
        b1 = b * bb1 * bb1
        b0 = ((1 - a - b) * x2 + (a - 1) * q * x_ - a + b + 1) * \
            (r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
             r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a +
                   q * r3 * a * b - 2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) * x2 +
             (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
              r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
              r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) * x_ +
             (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
             (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a +
             (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b + (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b +
             p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q)
        with np.errstate(all="ignore"):
            y = float(np.float64(b0) / np.float64(b1))
            y2 = y * y
            nu = x2 + y2 - 2 * x_ * y * cos_uv
            dist_PC = float(np.float64(dist_AB) / np.sqrt(np.float64(nu)))
        dist_PB = y * dist_PC
        dist_PA = x_ * dist_PC
        cam = np.array([[u[k] * dist_PA for k in range(3)], [v[k] * dist_PB for k in range(3)], [w[k] * dist_PC for k in range(3)]])
        models.append(umeyama3(Xw, cam))
    return models


# ------------------------------------------------------------------------------------------------ item 4: EPnP
def _sign_margin(mg, b, which):
    mx = float(np.max(np.abs(b)))
    if mx > 0.0:
        mg[M_BETA] = min(mg[M_BETA], abs(float(b[which])) / mx)


def _gauss_newton(L, rho, be):
    for _ in range(5):
        A, bb = np.zeros((6, 4)), np.zeros(6)
        for i in range(6):
            A[i, 0] = 2 * L[i, 0] * be[0] + L[i, 1] * be[1] + L[i, 3] * be[2] + L[i, 6] * be[3]
            A[i, 1] = L[i, 1] * be[0] + 2 * L[i, 2] * be[1] + L[i, 4] * be[2] + L[i, 7] * be[3]
            A[i, 2] = L[i, 3] * be[0] + L[i, 4] * be[1] + 2 * L[i, 5] * be[2] + L[i, 8] * be[3]
            A[i, 3] = L[i, 6] * be[0] + L[i, 7] * be[1] + L[i, 8] * be[2] + 2 * L[i, 9] * be[3]
            bb[i] = rho[i] - (L[i, 0] * be[0] * be[0] + L[i, 1] * be[0] * be[1] + L[i, 2] * be[1] * be[1] + L[i, 3] * be[0] * be[2] +
                              L[i, 4] * be[1] * be[2] + L[i, 5] * be[2] * be[2] + L[i, 6] * be[0] * be[3] + L[i, 7] * be[1] * be[3] +
                              L[i, 8] * be[2] * be[3] + L[i, 9] * be[3] * be[3])
        x = qr_solve(A, bb)
        for i in range(4):
            be[i] = be[i] + x[i]
    return be


def epnp(x, X, mask=None, margins=None, trace=None):
    """EPNPEstimator::ComputePose (absolute_pose.cc:204-609) on the points with mask != 0 (x [N, 2] normalised, X [N, 3]):
    the 3 x 4 model or None.  SolveForSign is the reference's: it negates whenever pcs_[0][2] is non-zero."""
    mg = margins if margins is not None else [math.inf] * 9
    x, X = np.asarray(x, np.float64).reshape(-1, 2), np.asarray(X, np.float64).reshape(-1, 3)
    N = len(x)
    mask = np.ones(N, bool) if mask is None else np.asarray(mask, bool)
    n = int(mask.sum())
    dn = float(n)
    with np.errstate(all="ignore"):
        c0 = tree_sum(X, mask) / dn
        d = X - c0
        six = tree_sum(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 1], d[:, 1] * d[:, 2],
                                 d[:, 2] * d[:, 2]], axis=1), mask)
        A = np.array([[six[0], six[1], six[2]], [six[1], six[3], six[4]], [six[2], six[4], six[5]]])
        U, D, _ = _orc().jacobi_svd(A)
        cws = np.zeros((4, 3))
        cws[0] = c0
        for i in range(1, 4):
            kk = math.sqrt(D[i - 1] / dn)
            cws[i] = c0 + kk * U[:, i - 1]
        CC = np.zeros((3, 3))
        for i in range(3):
            for j in range(1, 4):
                CC[i, j - 1] = cws[j][i] - cws[0][i]
        qr, _, _, nzp = colpiv_qr(CC)
        maxpiv = max(abs(qr[i, i]) for i in range(3))
        thr = maxpiv * (3.0 * EPS)
        rank = 0
        for i in range(nzp):
            piv = abs(qr[i, i])
            rank += piv > thr
            if thr > 0.0:
                mg[M_RANK] = min(mg[M_RANK], abs(piv - thr) / thr)
        if rank < 3:
            return None
        cinv = inverse3(CC)
        al = np.zeros((N, 4))
        for j in range(3):
            al[:, 1 + j] = (cinv[j, 0] * d[:, 0] + cinv[j, 1] * d[:, 1]) + cinv[j, 2] * d[:, 2]
        al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
        # M's rows: 2i -> (alpha, 0, -alpha x), 2i + 1 -> (0, alpha, -alpha y) per control point
        M0, M1 = np.zeros((N, 12)), np.zeros((N, 12))
        for j in range(4):
            M0[:, 3 * j] = al[:, j]
            M0[:, 3 * j + 2] = -al[:, j] * x[:, 0]
            M1[:, 3 * j + 1] = al[:, j]
            M1[:, 3 * j + 2] = -al[:, j] * x[:, 1]
        MtM = np.zeros((12, 12))
        for a in range(12):
            MtM[a] = tree_sum(M0[:, a:a + 1] * M0 + M1[:, a:a + 1] * M1, mask)
        Um, _, _ = _orc().jacobi_svd(MtM)
        Ut = Um.T  # Ut(r, c)
        dv = np.zeros((4, 6, 3))
        for i in range(4):
            a, b = 0, 1
            for j in range(6):
                for k in range(3):
                    dv[i, j, k] = Ut[11 - i, 3 * a + k] - Ut[11 - i, 3 * b + k]
                b += 1
                if b > 3:
                    a += 1
                    b = a + 1

        def dot(p, q, i):
            return (dv[p, i, 0] * dv[q, i, 0] + dv[p, i, 1] * dv[q, i, 1]) + dv[p, i, 2] * dv[q, i, 2]
        L = np.zeros((6, 10))
        for i in range(6):
            L[i] = [dot(0, 0, i), 2.0 * dot(0, 1, i), dot(1, 1, i), 2.0 * dot(0, 2, i), 2.0 * dot(1, 2, i), dot(2, 2, i),
                    2.0 * dot(0, 3, i), 2.0 * dot(1, 3, i), 2.0 * dot(2, 3, i), dot(3, 3, i)]
        rho = np.zeros(6)
        k = 0
        for a in range(4):
            for b in range(a + 1, 4):
                dd = cws[a] - cws[b]
                rho[k] = (dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2]
                k += 1
        betas = []
        b4 = svd_solve_tall(L[:, [0, 1, 3, 6]], rho)
        _sign_margin(mg, b4, 0)
        be = np.zeros(4)
        if b4[0] < 0:
            be[0] = math.sqrt(-b4[0])
            be[1:] = -b4[1:] / be[0]
        else:
            be[0] = math.sqrt(b4[0])
            be[1:] = b4[1:] / be[0]
        betas.append(_gauss_newton(L, rho, be))
        for ncol in (3, 5):
            bk = svd_solve_tall(L[:, :ncol], rho)
            for w in range(3):
                _sign_margin(mg, bk, w)
            be = np.zeros(4)
            if bk[0] < 0:
                be[0] = math.sqrt(-bk[0])
                be[1] = math.sqrt(-bk[2]) if bk[2] < 0 else 0.0
            else:
                be[0] = math.sqrt(bk[0])
                be[1] = math.sqrt(bk[2]) if bk[2] > 0 else 0.0
            if bk[1] < 0:
                be[0] = -be[0]
            if ncol == 5:
                be[2] = bk[3] / be[0]
            betas.append(_gauss_newton(L, rho, be))
        first = int(np.argmax(mask))
        cands, errs = [], []
        for be in betas:
            ccs = np.zeros((4, 3))
            for j in range(4):
                for k in range(3):
                    s = 0.0
                    for i in range(4):
                        s += be[i] * Ut[11 - i, 3 * j + k]
                    ccs[j, k] = s
            z = ((al[first, 0] * ccs[0, 2] + al[first, 1] * ccs[1, 2]) + al[first, 2] * ccs[2, 2]) + al[first, 3] * ccs[3, 2]
            negated = bool(z < 0.0 or z > 0.0)
            if negated:
                ccs = -ccs
            if trace is not None:
                trace.append(dict(first_depth_before=float(z), negated=negated))
            pcs = np.zeros((N, 3))
            for k in range(3):
                pcs[:, k] = ((al[:, 0] * ccs[0, k] + al[:, 1] * ccs[1, k]) + al[:, 2] * ccs[2, k]) + al[:, 3] * ccs[3, k]
            s6 = tree_sum(np.concatenate([pcs, X], axis=1), mask)
            pc0, pw0 = s6[:3] / dn, s6[3:] / dn
            t9 = np.zeros((N, 9))
            for j in range(3):
                for c in range(3):
                    t9[:, j * 3 + c] = (pcs[:, j] - pc0[j]) * (X[:, c] - pw0[c])
            abt = tree_sum(t9, mask).reshape(3, 3)
            Ua, _, Va = _orc().jacobi_svd(abt)
            R = np.zeros((3, 3))
            for i in range(3):
                for j in range(3):
                    R[i, j] = (Ua[i, 0] * Va[j, 0] + Ua[i, 1] * Va[j, 1]) + Ua[i, 2] * Va[j, 2]
            det = det3(R)
            if not math.isnan(det):
                mg[M_DET] = min(mg[M_DET], abs(det))
            if det < 0:
                for i in range(3):
                    for j in range(3):
                        R[i, j] = (Ua[i, 0] * Va[j, 0] + Ua[i, 1] * Va[j, 1]) + Ua[i, 2] * (-Va[j, 2])
            P = np.zeros((3, 4))
            P[:, :3] = R
            for i in range(3):
                P[i, 3] = pc0[i] - ((R[i, 0] * pw0[0] + R[i, 1] * pw0[1]) + R[i, 2] * pw0[2])
            cands.append(P)
            residuals(P, x[mask], X[mask], mg)  # the depth margins of the input points
            errs.append(tree_sum(np.sqrt(residuals(P, x, X)), mask))

        def cmp(i, j):
            # not a decision rounding can flip: two errors saturated by points behind the camera that are equal (n times
            # sqrt(DBL_MAX) on both sides), and two candidates that are one model up to rounding (the Gauss-Newton steps
            # of two approximations ended in the same betas) -- either choice is the same model within SAME_MODEL
            a, b = errs[i], errs[j]
            if a == b and a >= SATURATED:
                return
            if float(np.max(np.abs(cands[i] - cands[j]))) <= SAME_MODEL * float(np.max(np.abs(cands[j]))):
                return
            mx = max(abs(a), abs(b))
            if mx > 0.0 and not math.isnan(abs(a - b) / mx):
                mg[M_ERR] = min(mg[M_ERR], abs(a - b) / mx)
        bi = 0
        cmp(1, 0)
        if errs[1] < errs[0]:
            bi = 1
        cmp(2, bi)
        if errs[2] < errs[bi]:
            bi = 2
    return cands[bi]


# ------------------------------------------------------------------------------------------------ item 2: LO-RANSAC of one run
def loransac(x, X, max_residual, seed, opts):
    """LORANSAC<P3PEstimator, EPNPEstimator>::Estimate (loransac.h:91-233) on normalised points x [N, 2], X [N, 3]."""
    N = len(x)
    mg = [math.inf] * 9
    rep = dict(success=False, num_trials=0, num_inliers=0, model=np.zeros((3, 4)), model_is_local=False, mask=np.zeros(N, np.uint8),
               num_models=0, num_lo=0, margins=mg)
    if N < 3:
        return rep
    max_trials = max_num_trials(opts)
    if max_trials > MAX_TRIALS:
        raise ValueError("the options leave a run's trial count above DSM_ABSOLUTE_POSE_MAX_TRIALS")
    samples = _orc().sample_sequence(seed, 3, N, max_trials)
    best_cnt, best_sum, best_model, is_local = 0, DBL_MAX, None, False
    dyn = max_trials
    abort = False
    nt = 0
    while nt < max_trials:
        if abort:
            nt += 1
            break
        s = samples[nt]
        for model in p3p(x[s], X[s], mg):
            rep["num_models"] += 1
            r = residuals(model, x, X, mg)
            _res_margin(r, max_residual, mg)
            cnt, rsum = inlier_support(r, max_residual)
            better = cnt > best_cnt
            if cnt == best_cnt:
                mx = max(abs(rsum), abs(best_sum))
                if best_sum != DBL_MAX and mx > 0.0:
                    mg[M_TIE] = min(mg[M_TIE], abs(rsum - best_sum) / mx)
                better = rsum < best_sum
            if better:
                best_cnt, best_sum, best_model, is_local = cnt, rsum, model, False
                if cnt > 3 and cnt >= 4:
                    rep["num_lo"] += 1
                    local = epnp(x, X, r <= max_residual, mg)
                    if local is not None:
                        rep["num_models"] += 1
                        lr = residuals(local, x, X, mg)
                        _res_margin(lr, max_residual, mg)
                        lcnt, lsum = inlier_support(lr, max_residual)
                        lbetter = lcnt > best_cnt
                        if lcnt == best_cnt:
                            mx = max(abs(lsum), abs(best_sum))
                            if mx > 0.0:
                                mg[M_TIE] = min(mg[M_TIE], abs(lsum - best_sum) / mx)
                            lbetter = lsum < best_sum
                        if lbetter:
                            best_cnt, best_sum, best_model, is_local = lcnt, lsum, local, True
                dyn = compute_num_trials(best_cnt, N, opts["confidence"])
            if nt >= dyn and nt >= opts["min_num_trials"]:
                abort = True
                break
        nt += 1
    rep["num_trials"] = nt
    rep["num_inliers"] = best_cnt
    if best_model is not None and best_cnt > 0:
        rep["model"] = best_model
    if best_cnt < 3:
        return rep
    rep["success"] = True
    rep["model_is_local"] = is_local
    rep["mask"] = (residuals(best_model, x, X) <= max_residual).astype(np.uint8)
    return rep


# ------------------------------------------------------------------------------------------------ item 5: the problem
def scaled_camera(cam, factor):
    c = capi.Camera.from_buffer_copy(bytes(cam))
    c.params[0] = c.params[0] * factor
    if cam.model_id in (1, 4, 5, 6, 7, 10):
        c.params[1] = c.params[1] * factor
    return c


def estimate_absolute_pose(cam, points2D, points3D, estimate_focal_length, opts=None, seeds=None, problem=0):
    """EstimateAbsolutePose (pose.cc:79-158) of one problem; run s is seeded by seeds[s] or dsm_absolute_pose_seed(problem, s)."""
    o = dict(DEFAULTS)
    o.update(opts or {})
    orc = _orc()
    p2 = np.asarray(points2D, np.float64).reshape(-1, 2)
    X = np.asarray(points3D, np.float64).reshape(-1, 3)
    factors = focal_length_factors(o["num_focal_length_samples"], o["min_focal_length_ratio"], o["max_focal_length_ratio"]) \
        if estimate_focal_length else [1.0]
    out = dict(success=False, factor_index=-1, num_inliers=0, num_trials=0, model_is_local=False, focal_length_factor=0.0,
               proj_matrix=np.zeros((3, 4)), qvec=np.zeros(4), tvec=np.zeros(3), mask=np.zeros(len(p2), np.uint8),
               margins=[math.inf] * 9, runs=[])
    two = cam.model_id in (1, 4, 5, 6, 7, 10)
    out["focal_params"] = [cam.params[0], cam.params[1] if two else cam.params[0]]
    best = None
    for s, f in enumerate(factors):
        sc = scaled_camera(cam, f)
        xn = np.array([orc.image_to_world(sc, p) for p in p2]).reshape(-1, 2)
        me = float(orc.lib.oracle_image_to_world_threshold(ctypes.byref(sc), o["max_error"]))
        seed = int(seeds[s]) if seeds is not None else capi.absolute_pose_seed(problem, s, o["random_seed"])
        rep = loransac(xn, X, me * me, seed, o)
        out["runs"].append(rep)
        out["margins"] = [min(a, b) for a, b in zip(out["margins"], rep["margins"])]
        if rep["success"] and rep["num_inliers"] > out["num_inliers"]:
            out["num_inliers"] = rep["num_inliers"]
            best = (s, f, rep)
    if best is None:
        return out
    s, f, rep = best
    out.update(factor_index=s, focal_length_factor=f, num_trials=rep["num_trials"], model_is_local=rep["model_is_local"],
               proj_matrix=rep["model"].copy())
    if estimate_focal_length:
        out["focal_params"] = [cam.params[0] * f, cam.params[1] * f if two else cam.params[0] * f]
    out["qvec"] = orc.rotation_to_quaternion(np.ascontiguousarray(rep["model"][:, :3]))
    out["tvec"] = rep["model"][:, 3].copy()
    if np.isnan(out["qvec"]).any() or np.isnan(out["tvec"]).any():
        return out
    out["success"] = True
    out["mask"] = rep["mask"].copy()
    return out


def is_clear(margins, bar=CLEAR_MARGIN):
    return all(m >= bar for m in margins) and margins[M_RES] >= SWAP_BAR and margins[M_TIE] >= SWAP_BAR
