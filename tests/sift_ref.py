"""What COLMAP's ExtractSiftFeaturesCPU (src/feature/sift.cc:278-423) does with what VLFeat returns, restated in numpy with
float32 kept float32: the groups per DoG level, the first max_num_orientations orientations of a keypoint, L1_ROOT / L2
(src/feature/utils.cc:47-77, plain left-to-right float sums), round(512 v) truncated to 0 .. 255, the VLFeat -> UBC bin order
(sift.cc:58-74) and the max_num_features cut (sift.cc:387-398).  Its input is VLFeat's own output as tests/golden/
sift_vlfeat_v1.npz and sift_vlfeat_v2.npz store it (tools/make_sift_golden.py), so the expected features of a case are the reference library's
bytes carried through this host half -- the same structure as the host half of dagsfm_amd/csrc/sift_extraction.hip.

The second half of this file restates the VLFeat stage itself (scale space, detection, refinement, gradient, orientations,
float descriptors) in numpy; tests/test_sift_extraction_cpu.py holds it to the golden file bit for bit, and the GPU tests use it
(`extract`) on shapes the golden file does not store.
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_vlfeat_v1.npz")
GOLDEN_V2 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sift_vlfeat_v2.npz")  # sift_scenes.cases_v2()
L1_ROOT, L2 = 0, 1
OPTION_KEYS = ("num_octaves", "octave_resolution", "first_octave", "upright", "peak_threshold", "edge_threshold")
_golden = {}


def golden(path=GOLDEN):
    """{case: {image, options (dict), ints, floats, num_angles, angles, descriptors}} -- loaded once, shared, read-only."""
    if path not in _golden:
        z = np.load(path)
        out = {}
        for key in z.files:
            case, field = key.split("/")
            a = z[key]
            a.setflags(write=False)
            out.setdefault(case, {})[field] = a
        for case in out.values():
            o = dict(zip(OPTION_KEYS, case["options"].tolist()))
            for k in OPTION_KEYS[:4]:
                o[k] = int(o[k])
            case["options"] = o
        _golden[path] = out
    return _golden[path]


def golden_v2():
    """The cases of sift_scenes.cases_v2(), as golden() gives those of cases()."""
    return golden(GOLDEN_V2)


def ubc_permutation():
    """index[k] with ubc[:, index] = vlfeat: bin k of every cell goes to (0, 7, 6, 5, 4, 3, 2, 1)[k]."""
    q = (0, 7, 6, 5, 4, 3, 2, 1)
    return np.array([8 * c + q[k] for c in range(16) for k in range(8)])


def normalize(desc, normalization):
    """L1RootNormalizeFeatureDescriptors / L2NormalizeFeatureDescriptors on float32 rows, the sums left to right."""
    d = np.asarray(desc, np.float32)
    acc = np.zeros(len(d), np.float32)
    for i in range(d.shape[1]):
        acc = acc + (d[:, i] * d[:, i] if normalization == L2 else np.abs(d[:, i]))
    with np.errstate(invalid="ignore", divide="ignore"):
        if normalization == L2:
            norm = np.sqrt(acc)
            return np.where((acc > 0)[:, None], d / norm[:, None], d).astype(np.float32)  # Eigen's normalized(): a zero row stays
        return np.sqrt(d / acc[:, None]).astype(np.float32)


def to_unsigned_byte(desc):
    """FeatureDescriptorsToUnsignedByte: std::round (half away from zero) of 512 v, then TruncateCast (a NaN gives 0)."""
    with np.errstate(invalid="ignore"):
        v = np.float32(512.0) * np.asarray(desc, np.float32)
        t = np.trunc(v)
        r = t + np.where(v - t >= np.float32(0.5), np.float32(1), np.float32(0)) - np.where(v - t <= np.float32(-0.5), np.float32(1), np.float32(0))
        lo = np.where(np.float32(0) < r, r, np.float32(0))
        return np.where(lo < np.float32(255), lo, np.float32(255)).astype(np.uint8)


def level_cut(level_num_features, max_num_features):
    """first_level_to_keep of sift.cc:387-398: from the coarsest level down until the count of keypoints exceeds the limit."""
    total = 0
    for i in range(len(level_num_features) - 1, -1, -1):
        total += level_num_features[i]
        if total > max_num_features:
            return i
    return 0


def assemble(case, max_num_orientations=2, normalization=L1_ROOT, max_num_features=8192, descriptors=True):
    """(keypoints float32 [n, 4], descriptors uint8 [n, 128] or None) COLMAP returns for VLFeat's output `case` (golden()[name])."""
    ints, flts, nang, angles = case["ints"], case["floats"], case["num_angles"], case["angles"]
    first_desc = np.concatenate([[0], np.cumsum(nang)])
    levels, prev = [], None  # (number of keypoints, [feature rows], [descriptor rows])
    for i in range(len(ints)):
        key = (int(ints[i, 0]), int(ints[i, 3]))
        if key != prev:
            levels.append([0, [], []])
            prev = key
        levels[-1][0] += 1
        for a in range(min(int(nang[i]), max_num_orientations)):
            levels[-1][1].append((flts[i, 0] + np.float32(0.5), flts[i, 1] + np.float32(0.5), flts[i, 3], np.float32(angles[i, a])))
            levels[-1][2].append(int(first_desc[i]) + a)
    keep = level_cut([lv[0] for lv in levels], max_num_features)
    kps = [k for lv in levels[keep:] for k in lv[1]]
    rows = [r for lv in levels[keep:] for r in lv[2]]
    kp = np.array(kps, np.float32).reshape(-1, 4)
    if not descriptors:
        return kp, None
    d = to_unsigned_byte(normalize(case["descriptors"][rows].reshape(-1, 128), normalization))
    ubc = np.zeros_like(d)
    ubc[:, ubc_permutation()] = d
    return kp, ubc


# ---------------------------------------------------------------------------------------------------------------------------
# The VLFeat stage itself (lib/VLFeat/sift.c with mathop.h and imopv.c), restated in numpy: float32 where the source is float,
# float64 (or a Python float) where it is double, every operation in the source's order.  Taps are accumulated in a Python loop
# over taps, vectorised over pixels; orientation and descriptor run per keypoint in the window's pixel order (numpy's ufunc.at
# adds its operands one after the other, in index order).  Whatever the source takes from libm goes through `math`, which calls
# the host libm (numpy's own exp / sin are other implementations).  The host half (taps, table, pow, sin / cos) has the structure
# of dagsfm_amd/csrc/sift_extraction.hip.
import math

f32, f64 = np.float32, np.float64
VL_PI = 3.141592653589793
EPS_F = f32(1.19209290E-07)
EPS_D = 2.220446049250313e-16
TWO_PI_F = f32(2 * VL_PI)
_EXPN = np.array([math.exp(-float(k) * (25.0 / 256)) for k in range(257)] + [0.0], f64)  # fast_expn_init, sift.c:713-720


def fast_expn(x):
    """sift.c:691-706 on a float64 array of non-negative arguments."""
    x = np.asarray(x, f64)
    t = np.minimum(x, 25.0) * (256 / 25.0)
    i = t.astype(np.int64)
    r = t - i
    a, b = _EXPN[i], _EXPN[i + 1]
    return np.where(x > 25.0, 0.0, a + r * (b - a))


def fast_resqrt(x):
    """mathop.h:479-501 on a float32 array."""
    x = np.ascontiguousarray(x, f32)
    xhalf = f32(0.5) * x
    u = (np.int32(0x5f3759df) - (x.view(np.int32) >> 1)).view(f32)
    with np.errstate(all="ignore"):
        u = u * (f32(1.5) - xhalf * u * u)
        u = u * (f32(1.5) - xhalf * u * u)
    return u


def fast_sqrt(x):
    x = np.ascontiguousarray(x, f32)
    with np.errstate(all="ignore"):
        return np.where(x.astype(f64) < 1e-8, f32(0), x * fast_resqrt(x)).astype(f32)


def fast_atan2(y, x):
    """mathop.h:407-424 on float32 arrays."""
    c3, c1 = f32(0.1821), f32(0.9675)
    abs_y = np.abs(y) + EPS_F
    with np.errstate(all="ignore"):
        r = np.where(x >= 0, (x - abs_y) / (x + abs_y), (x + abs_y) / (abs_y - x)).astype(f32)
    angle = np.where(x >= 0, f32(VL_PI / 4), f32(3 * VL_PI / 4)).astype(f32)
    angle = angle + (c3 * r * r - c1) * r
    return np.where(y < 0, -angle, angle).astype(f32)


def mod_2pi(x):
    """mathop.h:109-115 on a float32 array."""
    x = np.array(x, f32)
    while (x > TWO_PI_F).any():
        x = np.where(x > TWO_PI_F, x - TWO_PI_F, x).astype(f32)
    while (x < 0).any():
        x = np.where(x < 0, x + TWO_PI_F, x).astype(f32)
    return x


def gaussian_taps(sigma):
    """_vl_sift_smooth's filter (sift.c:782-798): (taps float32, half-width)."""
    W = max(int(math.ceil(4.0 * sigma)), 1)
    g = np.zeros(2 * W + 1, f32)
    acc = f32(0)
    for j in range(2 * W + 1):
        d = f32(j - W) / f32(sigma)
        g[j] = f32(math.exp(-0.5 * float(d * d)))
        acc = acc + g[j]
    return g / acc, W


def smooth(img, sigma):
    """_vl_sift_smooth: vl_imconvcol_vf with VL_PAD_BY_CONTINUITY down the columns, then along the rows."""
    g, W = gaussian_taps(sigma)
    out = np.asarray(img, f32)
    for axis in (0, 1):
        n = out.shape[axis]
        pos = np.arange(n)
        acc = np.zeros_like(out)
        for j in range(2 * W + 1):
            acc = acc + np.take(out, np.clip(pos - W + j, 0, n - 1), axis=axis) * g[2 * W - j]
        out = acc
    return out


def upsample_rows(src, width, height):
    """copy_and_upsample_rows (sift.c:738-758) on flat buffers: the result is the transpose, 2 width rows of height."""
    s = np.asarray(src, f32).ravel()[:width * height].reshape(height, width)
    d = np.zeros((2 * width, height), f32)
    d[0::2] = s.T
    d[1:-1:2] = (f32(0.5) * (s[:, :-1] + s[:, 1:])).T
    d[-1] = s[:, -1]
    return d.ravel()


def _shift(x, n):
    return x << n if n >= 0 else x >> -n


def _refine(D, x, y, s, w, h, S, tp, te):
    """One candidate of sift.c:1267-1427; D is the DoG [S + 2, h, w].  Returns None or (ix, iy, is, xn, yn, sn)."""
    b = [0.0, 0.0, 0.0]
    dx = dy = 0
    tiny = float(f32(1e-10))
    for _ in range(5):
        x += dx
        y += dy
        at = lambda i, j, k: D[s + 1 + k, y + j, x + i]  # float32 scalars: float arithmetic until the source promotes
        Dx = 0.5 * float(at(1, 0, 0) - at(-1, 0, 0))
        Dy = 0.5 * float(at(0, 1, 0) - at(0, -1, 0))
        Ds = 0.5 * float(at(0, 0, 1) - at(0, 0, -1))
        c2 = 2.0 * float(at(0, 0, 0))
        Dxx = float(at(1, 0, 0) + at(-1, 0, 0)) - c2
        Dyy = float(at(0, 1, 0) + at(0, -1, 0)) - c2
        Dss = float(at(0, 0, 1) + at(0, 0, -1)) - c2
        Dxy = 0.25 * float(at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0))
        Dxs = 0.25 * float(at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1))
        Dys = 0.25 * float(at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1))
        A = [[Dxx, Dxy, Dxs], [Dxy, Dyy, Dys], [Dxs, Dys, Dss]]  # A[i][j] = Aat(i, j)
        b = [-Dx, -Dy, -Ds]
        for j in range(3):
            maxa, maxabsa, maxi = 0.0, 0.0, -1
            for i in range(j, 3):
                if abs(A[i][j]) > maxabsa:
                    maxa, maxabsa, maxi = A[i][j], abs(A[i][j]), i
            if maxabsa < tiny:
                b = [0.0, 0.0, 0.0]
                break
            i = maxi
            for jj in range(j, 3):
                A[i][jj], A[j][jj] = A[j][jj], A[i][jj]
                A[j][jj] /= maxa
            b[j], b[i] = b[i], b[j]
            b[j] /= maxa
            for ii in range(j + 1, 3):
                f = A[ii][j]
                for jj in range(j, 3):
                    A[ii][jj] -= f * A[j][jj]
                b[ii] -= f * b[j]
        for i in (2, 1):
            f = b[i]
            for ii in range(i - 1, -1, -1):
                b[ii] -= f * A[ii][i]
        dx = (1 if b[0] > 0.6 and x < w - 2 else 0) + (-1 if b[0] < -0.6 and x > 1 else 0)
        dy = (1 if b[1] > 0.6 and y < h - 2 else 0) + (-1 if b[1] < -0.6 and y > 1 else 0)
        if dx == 0 and dy == 0:
            break
    val = float(D[s + 1, y, x]) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2])
    den = Dxx * Dyy - Dxy * Dxy
    num = (Dxx + Dyy) * (Dxx + Dyy)
    score = num / den if den != 0 else (math.copysign(math.inf, num) * math.copysign(1.0, den) if num != 0 else math.nan)
    xn, yn, sn = x + b[0], y + b[1], s + b[2]
    good = (abs(val) > tp and score < (te + 1) * (te + 1) / te and score >= 0 and abs(b[0]) < 1.5 and abs(b[1]) < 1.5 and abs(b[2]) < 1.5
            and 0 <= xn <= w - 1 and 0 <= yn <= h - 1 and -1 <= sn <= S + 1)
    return (x, y, s, xn, yn, sn) if good else None


def _gradient(level):
    """update_gradient (sift.c:1447-1530) of one level: (modulus, angle) float32."""
    src = level
    gx, gy = np.zeros_like(src), np.zeros_like(src)
    gx[:, 1:-1] = f32(0.5) * (src[:, 2:] - src[:, :-2])
    gx[:, 0] = src[:, 1] - src[:, 0]
    gx[:, -1] = src[:, -1] - src[:, -2]
    gy[1:-1] = f32(0.5) * (src[2:] - src[:-2])
    gy[0] = src[1] - src[0]
    gy[-1] = src[-1] - src[-2]
    mod = fast_sqrt(gx * gx + gy * gy)
    ang = mod_2pi((fast_atan2(gy, gx).astype(f64) + 2 * VL_PI).astype(f32))
    return mod, ang


def _orientations(mod, ang, kx, ky, ksigma, xper):
    """vl_sift_calc_keypoint_orientations (sift.c:1559-1692; the bilinear branch, :669) -> list of angles (Python floats)."""
    h, w = mod.shape
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    sigmaw = 1.5 * sigma
    W = int(max(math.floor(3.0 * sigmaw), 1))
    if xi < 0 or xi > w - 1 or yi < 0 or yi > h - 1:
        return []
    ys = np.arange(max(-W, -yi), min(W, h - 1 - yi) + 1)
    xs = np.arange(max(-W, -xi), min(W, w - 1 - xi) + 1)
    YS, XS = np.meshgrid(ys, xs, indexing="ij")
    YS, XS = YS.ravel(), XS.ravel()
    dx, dy = (xi + XS).astype(f64) - x, (yi + YS).astype(f64) - y
    r2 = dx * dx + dy * dy
    keep = ~(r2 >= W * W + 0.6)
    YS, XS, r2 = YS[keep], XS[keep], r2[keep]
    wgt = fast_expn(r2 / (2 * sigmaw * sigmaw))
    m, a = mod[yi + YS, xi + XS].astype(f64), ang[yi + YS, xi + XS].astype(f64)
    fbin = 36 * a / (2 * VL_PI)
    b = np.floor(fbin - 0.5)
    rbin = fbin - b - 0.5
    b = b.astype(np.int64)
    idx = np.stack([(b + 36) % 36, (b + 1) % 36], axis=1).ravel()
    val = np.stack([(1 - rbin) * m * wgt, rbin * m * wgt], axis=1).ravel()
    hist = np.zeros(36, f64)
    np.add.at(hist, idx, val)
    hist = hist.tolist()
    for _ in range(6):
        prev, first = hist[35], hist[0]
        for i in range(35):
            newh = (prev + hist[i] + hist[(i + 1) % 36]) / 3.0
            prev = hist[i]
            hist[i] = newh
        hist[35] = (prev + hist[35] + first) / 3.0
    maxh = 0.0
    for v in hist:
        maxh = maxh if maxh > v else v
    out = []
    for i in range(36):
        h0, hm, hp = hist[i], hist[(i - 1 + 36) % 36], hist[(i + 1 + 36) % 36]
        if h0 > 0.8 * maxh and h0 > hm and h0 > hp:
            di = -0.5 * (hp - hm) / (hp + hm - 2 * h0)
            out.append(2 * VL_PI * (i + di + 0.5) / 36)
            if len(out) == 4:
                break
    return out


def _normalize_histogram(d):
    norm = f32(0)
    for v in d:
        norm = norm + v * v
    norm = fast_sqrt(np.array([norm], f32))[0] + EPS_F
    return (d / norm).astype(f32)


def _descriptor(mod, ang, kx, ky, ksigma, xper, angle0):
    """vl_sift_calc_keypoint_descriptor (sift.c:1923-2093) -> float32 [128]; zeros where its bound check returns early."""
    h, w = mod.shape
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    st0, ct0 = math.sin(angle0), math.cos(angle0)
    SBP = 3.0 * sigma + EPS_D
    W = int(math.floor(math.sqrt(2.0) * SBP * 5 / 2.0 + 0.5))
    descr = np.zeros(128, f32)
    if xi < 0 or xi >= w or yi < 0 or yi >= h - 1:
        return descr
    dys = np.arange(max(-W, 1 - yi), min(W, h - yi - 2) + 1)
    dxs = np.arange(max(-W, 1 - xi), min(W, w - xi - 2) + 1)
    DY, DX = np.meshgrid(dys, dxs, indexing="ij")
    DY, DX = DY.ravel(), DX.ravel()
    if len(DY):
        m, angle = mod[yi + DY, xi + DX], ang[yi + DY, xi + DX]
        theta = mod_2pi((angle.astype(f64) - angle0).astype(f32))
        dx = ((xi + DX).astype(f64) - x).astype(f32).astype(f64)
        dy = ((yi + DY).astype(f64) - y).astype(f32).astype(f64)
        nx = ((ct0 * dx + st0 * dy) / SBP).astype(f32)
        ny = ((-st0 * dx + ct0 * dy) / SBP).astype(f32)
        nt = ((f32(8) * theta).astype(f64) / (2 * VL_PI)).astype(f32)
        win = fast_expn((nx * nx + ny * ny).astype(f64) / 8.0).astype(f32)
        binx = np.floor((nx.astype(f64) - 0.5).astype(f32)).astype(np.int64)
        biny = np.floor((ny.astype(f64) - 0.5).astype(f32)).astype(np.int64)
        bint = np.floor(nt).astype(np.int64)
        rbinx = (nx.astype(f64) - (binx + 0.5)).astype(f32)
        rbiny = (ny.astype(f64) - (biny + 0.5)).astype(f32)
        rbint = nt - bint.astype(f32)
        idx, val, ok = [], [], []
        for dbx in (0, 1):
            for dby in (0, 1):
                for dbt in (0, 1):
                    ok.append((binx + dbx >= -2) & (binx + dbx < 2) & (biny + dby >= -2) & (biny + dby < 2))
                    val.append(win * m * np.abs(f32(1 - dbx) - rbinx) * np.abs(f32(1 - dby) - rbiny) * np.abs(f32(1 - dbt) - rbint))
                    idx.append(80 + (bint + dbt) % 8 + (biny + dby) * 32 + (binx + dbx) * 8)
        ok = np.stack(ok, axis=1).ravel()
        np.add.at(descr, np.stack(idx, axis=1).ravel()[ok], np.stack(val, axis=1).ravel()[ok].astype(f32))
    descr = _normalize_histogram(descr)
    descr = np.where(descr.astype(f64) > 0.2, f32(0.2), descr).astype(f32)
    return _normalize_histogram(descr)


def vlfeat(image, num_octaves=4, octave_resolution=3, first_octave=-1, upright=0, peak_threshold=0.02 / 3, edge_threshold=10.0,
           trace=None):
    """The VLFeat stage in COLMAP's call sequence (sift.cc:266-385) on a uint8 image: the fields of a golden case.  A list given
    as `trace` receives, per octave that is searched, {octave, dog float32 [S + 2, h, w], flags bool [S, h, w]}: the DoG and the
    candidates before refinement, in the scan order (s, y, x) the device compacts them in."""
    height, width = image.shape
    S, o_min, tp, te = octave_resolution, first_octave, peak_threshold, edge_threshold
    O = num_octaves if num_octaves >= 0 else int(max(math.floor(math.log2(min(width, height))) - o_min - 3, 1))
    sigmak = math.pow(2.0, 1.0 / S)
    sigma0 = 1.6 * sigmak
    dsigma0 = sigma0 * math.sqrt(1.0 - 1.0 / (sigmak * sigmak))
    im = (np.asarray(image, np.uint8).astype(f32) / f32(255.0)).astype(f32)
    ints, flts, nangs, angs, descs = [], [], [], [], []
    levels = None
    for oc in range(o_min, o_min + O):
        w, h = _shift(width, -oc), _shift(height, -oc)
        if w < 2 or h < 2:
            break
        if oc == o_min:  # vl_sift_process_first_octave
            if o_min < 0:
                t = upsample_rows(im, width, height)
                base = upsample_rows(t, height, 2 * width)
                for q in range(-1, o_min, -1):  # the source's arguments as they are (sift.c:1023-1028)
                    t = upsample_rows(base, width << -q, height << -q)
                    base = upsample_rows(t, width << -q, 2 * (height << -q))
                base = base.reshape(h, w)
            else:
                base = im[::1 << o_min, ::1 << o_min][:h, :w]
            sa, sb = sigma0 * math.pow(sigmak, -1), 0.5 * math.pow(2.0, -o_min)
            if sa > sb:
                base = smooth(base, math.sqrt(sa * sa - sb * sb))
        else:  # vl_sift_process_next_octave
            s_best = min(-1 + S, S + 1)
            base = levels[s_best + 1][::2, ::2][:h, :w]
            sa = sigma0 * float(f32(sigmak) ** f32(-1))
            sb = sigma0 * float(f32(sigmak) ** f32(s_best - S))
            if sa > sb:
                base = smooth(base, math.sqrt(sa * sa - sb * sb))
        levels = [np.ascontiguousarray(base, f32)]
        for s in range(0, S + 2):
            levels.append(smooth(levels[-1], dsigma0 * math.pow(sigmak, s)))
        if w < 3 or h < 3:
            continue
        D = np.stack([levels[k + 1] - levels[k] for k in range(S + 2)])
        xper = math.pow(2.0, oc)
        keys = []
        flags = np.zeros((S, h, w), bool)
        for s in range(S):  # vl_sift_detect: the strict 26-neighbour test, candidates in (s, y, x) order
            v = D[s + 1, 1:-1, 1:-1]
            mx, mn = v.astype(f64) >= 0.8 * tp, v.astype(f64) <= -0.8 * tp
            for ds in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if ds or dy or dx:
                            u = D[s + 1 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                            mx &= v > u
                            mn &= v < u
            flags[s, 1:-1, 1:-1] = mx | mn
            for y, x in zip(*np.nonzero(mx | mn)):
                r = _refine(D, int(x) + 1, int(y) + 1, s, w, h, S, tp, te)
                if r is not None:
                    ix, iy, is_, xn, yn, sn = r
                    keys.append((ix, iy, is_, f32(xn * xper), f32(yn * xper), f32(sn), f32(sigma0 * math.pow(2.0, sn / S) * xper)))
        if trace is not None:
            trace.append({"octave": oc, "dog": D, "flags": flags})
        grads = {}
        for ix, iy, is_, kx, ky, ks, ksigma in keys:
            if is_ not in grads:
                grads[is_] = _gradient(levels[is_ + 1])
            mod, ang = grads[is_]
            a = [0.0] if upright else _orientations(mod, ang, kx, ky, ksigma, xper)
            ints.append((oc, ix, iy, is_))
            flts.append((kx, ky, ks, ksigma))
            nangs.append(len(a))
            angs.append(a + [0.0] * (4 - len(a)))
            descs.extend(_descriptor(mod, ang, kx, ky, ksigma, xper, t) for t in a)
    n = len(ints)
    return {"ints": np.array(ints, np.int32).reshape(n, 4), "floats": np.array(flts, f32).reshape(n, 4), "num_angles": np.array(nangs, np.int32),
            "angles": np.array(angs, f64).reshape(n, 4), "descriptors": np.array(descs, f32).reshape(len(descs), 128)}


def extract(image, options=None, max_num_orientations=2, normalization=L1_ROOT, max_num_features=8192, descriptors=True):
    """ExtractSiftFeaturesCPU restated end to end: (keypoints, descriptors) of a uint8 image."""
    return assemble(vlfeat(image, **(options or {})), max_num_orientations, normalization, max_num_features, descriptors)
