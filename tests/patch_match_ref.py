"""The normative restatement of PatchMatch multi-view stereo in numpy: PatchMatchCuda of the reference's
src/mvs/patch_match_cuda.cu operation for operation in float32 and in its evaluation order, with the points the reference
leaves to the hardware fixed as DESIGN.md 24 lists them.  dsm_patch_match equals it bit for bit.

Written in the rotated-frame formulation of the reference: a sweep walks the rows of the current frame top to bottom, every
column at once (the arrays below are vectors over the columns, window taps are trailing axes), and every map is turned a
quarter counter-clockwise between sweeps (np.rot90 = CudaRotate).  In-order float sums are np.cumsum(..., dtype=float32)
behind a leading zero, as vocabulary_build_ref.py does them.

exp / sin / cos are the host libm's double value of the float argument rounded to float (math.exp, math.sin, math.cos):
the correctly rounded float, which is what exact_exp.h and exact_trig.h return on the device.
"""
import math
from dataclasses import dataclass, fields

import numpy as np

f32 = np.float32
POSE = 43  # K[4], R[9], T[3], C[3], P[12], inv_P[12]
MAX_REJECT = 64
FLT_EPSILON = f32(1.1920928955078125e-07)


# ---------------------------------------------------------------- options

@dataclass
class Options:
    """PatchMatchOptions (patch_match.h:59-139): the numerical fields, the reference's defaults."""
    window_radius: int = 5
    window_step: int = 1
    num_samples: int = 15
    num_iterations: int = 5
    geom_consistency: bool = True
    filter: bool = True
    filter_min_num_consistent: int = 2
    seed: int = 0
    sigma_spatial: float = -1.0
    sigma_color: float = float(f32(0.2))
    ncc_sigma: float = float(f32(0.6))
    min_triangulation_angle: float = 1.0
    incident_angle_sigma: float = float(f32(0.9))
    geom_consistency_regularizer: float = float(f32(0.3))
    geom_consistency_max_cost: float = 3.0
    filter_min_ncc: float = float(f32(0.1))
    filter_min_triangulation_angle: float = 3.0
    filter_geom_consistency_max_cost: float = 1.0

    def check(self):
        """PatchMatchOptions::Check (patch_match.h:141-168) + the window limits; the first violated condition, or None."""
        tests = [
            (self.window_radius > 0, "window_radius <= 0"), (self.window_radius <= 32, "window_radius > 32"),
            (self.window_step > 0, "window_step <= 0"), (self.window_step <= 2, "window_step > 2"),
            (self.sigma_color > 0, "sigma_color <= 0"), (self.num_samples > 0, "num_samples <= 0"),
            (self.ncc_sigma > 0, "ncc_sigma <= 0"), (self.min_triangulation_angle >= 0, "min_triangulation_angle < 0"),
            (self.min_triangulation_angle < 180, "min_triangulation_angle >= 180"),
            (self.incident_angle_sigma > 0, "incident_angle_sigma <= 0"), (self.num_iterations > 0, "num_iterations <= 0"),
            (self.geom_consistency_regularizer >= 0, "geom_consistency_regularizer < 0"),
            (self.geom_consistency_max_cost >= 0, "geom_consistency_max_cost < 0"),
            (self.filter_min_ncc >= -1, "filter_min_ncc < -1"), (self.filter_min_ncc <= 1, "filter_min_ncc > 1"),
            (self.filter_min_triangulation_angle >= 0, "filter_min_triangulation_angle < 0"),
            (self.filter_min_triangulation_angle <= 180, "filter_min_triangulation_angle > 180"),
            (self.filter_min_num_consistent >= 0, "filter_min_num_consistent < 0"),
            (self.filter_geom_consistency_max_cost >= 0, "filter_geom_consistency_max_cost < 0"),
        ]
        for ok, msg in tests:
            if not ok:
                return msg
        return None

    def as_dict(self):
        return {f.name: getattr(self, f.name) for f in fields(self)}


# ---------------------------------------------------------------- exact scalar functions

def _map(fn, x):
    x = np.asarray(x, dtype=f32)
    flat = x.astype(np.float64).ravel()
    out = np.empty(flat.shape, dtype=np.float64)
    for i, v in enumerate(flat.tolist()):
        try:
            out[i] = fn(v)
        except OverflowError:
            out[i] = math.inf
        except ValueError:  # sin / cos of an infinity
            out[i] = math.nan
    return out.astype(f32).reshape(x.shape)


def exp32(x):
    return _map(math.exp, x)


def sin32(x):
    return _map(math.sin, x)


def cos32(x):
    return _map(math.cos, x)


def seqsum(x, axis=-1):
    """The float32 sum of x along axis in index order, starting from 0.0f."""
    x = np.asarray(x, dtype=f32)
    shape = list(x.shape)
    shape[axis] = 1
    return np.take(np.cumsum(np.concatenate([np.zeros(shape, f32), x], axis=axis), axis=axis, dtype=f32), -1, axis=axis)


def requantise(b):
    """uint8(255.0f * (b / 255.0f)) of gpu_mat_ref_image.cu:80 under IEEE float."""
    b = np.asarray(b, dtype=np.uint8)
    return (f32(255.0) * (b.astype(f32) / f32(255.0))).astype(np.uint8)


# ---------------------------------------------------------------- Philox4x32-10

def philox4x32_10(counter, key):
    """counter: four uint32 (arrays broadcast), key: two uint32 -> the four output words (Salmon et al., SC'11)."""
    M = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) for c in counter])
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & M, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & M
        k0 = (k0 + np.uint64(0x9E3779B9)) & M
        k1 = (k1 + np.uint64(0xBB67AE85)) & M
    return c0.astype(np.uint32), c1.astype(np.uint32), c2.astype(np.uint32), c3.astype(np.uint32)


def uniform(seed, key1, a, b, kind, d):
    """Draw d of the stream (a, b, kind) under the key (seed, key1): u = ((word0 >> 8) + 1) * 2^-24, in (0, 1]."""
    r = philox4x32_10((d, a, b, kind), (seed, key1))[0]
    return ((r >> np.uint32(8)) + np.uint32(1)).astype(f32) * f32(2.0 ** -24)


# ---------------------------------------------------------------- the constants of a call

def constants(o):
    """Everything dsm_patch_match computes once on the host, in the same float / double operations."""
    c = {}
    radius, step = int(o.window_radius), int(o.window_step)
    sigma_spatial = f32(radius) if o.sigma_spatial <= 0 else f32(o.sigma_spatial)
    sigma_color, ncc_sigma, inc_sigma = f32(o.sigma_color), f32(o.ncc_sigma), f32(o.incident_angle_sigma)
    sn = f32(1.0) / (f32(2.0) * sigma_spatial * sigma_spatial)
    cn = f32(1.0) / (f32(2.0) * sigma_color * sigma_color)
    offs = list(range(-radius, radius + 1, step))
    c["radius"], c["step"], c["offs"] = radius, step, offs
    c["w_spatial"] = np.array([f32(math.exp(float(-f32(wr * wr + wc * wc) * sn))) for wr in offs for wc in offs], dtype=f32)
    cd = np.arange(256, dtype=f32) / f32(255.0)
    c["w_color"] = np.array([f32(math.exp(float(v))) for v in (-(cd * cd) * cn)], dtype=f32)
    c["tex"] = np.arange(256, dtype=f32) / f32(255.0)
    min_tri = f32(o.min_triangulation_angle * 0.0174532925199432)
    filter_tri = f32(o.filter_min_triangulation_angle * 0.0174532925199432)
    c["cos_min_tri"] = f32(math.cos(float(min_tri)))
    c["inv_inc"] = f32(-0.5) / (inc_sigma * inc_sigma)
    c["inv_ncc"] = f32(-0.5) / (ncc_sigma * ncc_sigma)
    erf_val = f32(math.erf(float(f32(2.0) / (ncc_sigma * f32(1.414213562)))))
    c["ncc_norm"] = f32(2.0 / (math.sqrt(2.0 * math.pi) * float(ncc_sigma) * float(erf_val)))
    c["geom_reg"] = f32(o.geom_consistency_regularizer)
    c["geom_max_cost"] = f32(o.geom_consistency_max_cost)
    cc = f32(1.0) - f32(o.filter_min_ncc)
    c["filter_min_ncc_prob"] = f32(math.exp(float(cc * cc * c["inv_ncc"]))) * c["ncc_norm"]
    c["filter_cos_min_tri"] = f32(math.cos(float(filter_tri)))
    c["filter_geom_max_cost"] = f32(o.filter_geom_consistency_max_cost)
    c["filter_min_num_consistent"] = int(o.filter_min_num_consistent)
    c["num_samples"] = int(o.num_samples)
    c["seed"] = int(o.seed)
    return c


def sweep_schedule(o, iteration, sweep):
    """RunWithWindowSizeAndStep :1283-1294: (perturbation, perturbation * pi, prev_sel_prob_weight); pow in double."""
    exponent = f32(iteration) + f32(sweep) / f32(4.0)
    perturbation = f32(1.0) / f32(math.pow(2.0, float(exponent)))
    return perturbation, f32(float(perturbation) * math.pi), f32(iteration * 4 + sweep) / f32(o.num_iterations * 4)


# ---------------------------------------------------------------- InitTransforms

def _mat33_mul(A, B):
    C = np.zeros(9, f32)
    for r in range(3):
        for c in range(3):
            C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c]
    return C


def _mat33_vec(A, v):
    return np.array([A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2] for r in range(3)], dtype=f32)


def _transpose33(A):
    return np.asarray(A, dtype=f32).reshape(3, 3).T.reshape(9).copy()


def compose_pose(R1, T1, image):
    """mvs/image.cc:92-130 against the (rotated) reference pose: the POSE floats of one source image."""
    K, R2, T2 = [np.asarray(image[k], dtype=f32) for k in ("K", "R", "T")]
    out = np.zeros(POSE, f32)
    out[0:4] = [K[0], K[2], K[4], K[5]]
    rel_R = _mat33_mul(R2, _transpose33(R1))
    rel_T = (T2 - _mat33_vec(rel_R, T1)).astype(f32)
    out[4:13], out[13:16] = rel_R, rel_T
    out[16:19] = -_mat33_vec(_transpose33(rel_R), rel_T)
    KR, KT = _mat33_mul(K, rel_R), _mat33_vec(K, rel_T)
    P = np.zeros(12, f32)
    for r in range(3):
        P[4 * r:4 * r + 3] = KR[3 * r:3 * r + 3]
        P[4 * r + 3] = KT[r]
    out[19:31] = P
    m00, m01, m02, t0, m10, m11, m12, t1, m20, m21, m22, t2 = [float(v) for v in P]
    c00, c01, c02 = m11 * m22 - m12 * m21, m12 * m20 - m10 * m22, m10 * m21 - m11 * m20
    with np.errstate(all="ignore"):
        det = np.float64(m00 * c00 + m01 * c01 + m02 * c02)
        inv = [np.float64(c00) / det, np.float64(m02 * m21 - m01 * m22) / det, np.float64(m01 * m12 - m02 * m11) / det,
               np.float64(c01) / det, np.float64(m00 * m22 - m02 * m20) / det, np.float64(m02 * m10 - m00 * m12) / det,
               np.float64(c02) / det, np.float64(m01 * m20 - m00 * m21) / det, np.float64(m00 * m11 - m01 * m10) / det]
        for r in range(3):
            for c in range(3):
                out[31 + 4 * r + c] = f32(inv[3 * r + c])
            out[31 + 4 * r + 3] = f32(-(inv[3 * r] * t0 + inv[3 * r + 1] * t1 + inv[3 * r + 2] * t2))
    return out


def init_transforms(images, ref_idx, src_idxs):
    """InitTransforms :1500-1608 -> K [4][4] = {fx, cx, fy, cy}, inv_K [4][4], poses [4][S][POSE] per rotation."""
    ref = images[ref_idx]
    h, w = ref["data"].shape
    Kf = np.asarray(ref["K"], dtype=f32)
    K = np.array([[Kf[0], Kf[2], Kf[4], Kf[5]]] * 4, dtype=f32)
    wm1, hm1 = f32(w - 1), f32(h - 1)
    K[1] = [K[1][2], K[1][3], K[1][0], K[1][1]]
    K[1][3] = wm1 - K[1][3]
    K[2][1] = wm1 - K[2][1]
    K[2][3] = hm1 - K[2][3]
    K[3] = [K[3][2], K[3][3], K[3][0], K[3][1]]
    K[3][1] = hm1 - K[3][1]
    iK = np.zeros((4, 4), f32)
    for r in range(4):
        iK[r] = [f32(1.0) / K[r][0], -K[r][1] / K[r][0], f32(1.0) / K[r][2], -K[r][3] / K[r][2]]
    R, T = np.asarray(ref["R"], dtype=f32).copy(), np.asarray(ref["T"], dtype=f32).copy()
    R_z90 = np.array([0, 1, 0, -1, 0, 0, 0, 0, 1], dtype=f32)
    poses = np.zeros((4, len(src_idxs), POSE), f32)
    for r in range(4):
        for s, idx in enumerate(src_idxs):
            poses[r, s] = compose_pose(R, T, images[idx])
        R, T = _mat33_mul(R_z90, R), _mat33_vec(R_z90, T)
    return K, iK, poses


def rotate_map(a):
    """GpuMat::Rotate / CudaRotate: a quarter turn counter-clockwise of the last two axes."""
    return np.ascontiguousarray(np.rot90(a, 1, axes=(-2, -1)))


def rotate_normal_map(n):
    """RotateNormalMap :746-758, then the rotation of the map."""
    return rotate_map(np.stack([n[1], -n[0], n[2]]))


# ---------------------------------------------------------------- the reference image

def filter_ref_image(img, c):
    """GpuMatRefImage::Filter (gpu_mat_ref_image.cu:44-83) -> (re-quantised image, sum image, squared sum image)."""
    h, w = img.shape
    r, offs = c["radius"], c["offs"]
    pad = np.pad(img, r)
    taps = np.stack([pad[r + wr:r + wr + h, r + wc:r + wc + w] for wr in offs for wc in offs], axis=-1)  # [h, w, taps]
    color = c["tex"][taps]
    diff = np.abs(taps.astype(np.int32) - img.astype(np.int32)[..., None])
    weight = c["w_spatial"][None, None, :] * c["w_color"][diff]
    color_sum = seqsum(weight * color)
    color_squared_sum = seqsum(weight * color * color)
    weight_sum = seqsum(weight)
    return requantise(img), color_sum / weight_sum, color_squared_sum / weight_sum


# ---------------------------------------------------------------- the source images

class Sources:
    """The source images (and depth maps) of a problem, zero-padded to a common size; per-image sizes rule the border."""

    def __init__(self, images, src_idxs, with_depth):
        self.S = len(src_idxs)
        hs = [images[i]["data"].shape[0] for i in src_idxs] or [1]
        ws = [images[i]["data"].shape[1] for i in src_idxs] or [1]
        self.h, self.w = np.array(hs, np.int64), np.array(ws, np.int64)
        self.px = np.zeros((max(self.S, 1), max(hs), max(ws)), np.uint8)
        self.depth = np.zeros(self.px.shape, f32) if with_depth else None
        for s, i in enumerate(src_idxs):
            self.px[s, :hs[s], :ws[s]] = images[i]["data"]
            if with_depth:
                self.depth[s, :hs[s], :ws[s]] = images[i]["depth_map"]

    def _guard(self, sidx, x, y):
        wf, hf = self.w[sidx].astype(f32), self.h[sidx].astype(f32)
        return (x >= f32(-1.0)) & (x <= wf) & (y >= f32(-1.0)) & (y <= hf)

    def _texel(self, tex, sidx, ix, iy):
        w, h = self.w[sidx], self.h[sidx]
        inb = (ix >= 0) & (iy >= 0) & (ix < w) & (iy < h)
        v = tex[self.px[sidx, np.where(inb, iy, 0), np.where(inb, ix, 0)]]
        return np.where(inb, v, f32(0.0))

    def sample(self, tex, sidx, x, y):
        """tex2DLayered, linear filtering, border 0, at the unnormalised coordinate (x, y); sidx broadcasts against x."""
        sidx, x, y = np.broadcast_arrays(sidx, x, y)
        ok = self._guard(sidx, x, y)
        xb, yb = np.where(ok, x, f32(0.0)) - f32(0.5), np.where(ok, y, f32(0.0)) - f32(0.5)
        fx, fy = np.floor(xb), np.floor(yb)
        a, b = xb - fx, yb - fy
        a1, b1 = f32(1.0) - a, f32(1.0) - b
        ix, iy = fx.astype(np.int64), fy.astype(np.int64)
        v = (a1 * b1) * self._texel(tex, sidx, ix, iy)
        v = v + (a * b1) * self._texel(tex, sidx, ix + 1, iy)
        v = v + (a1 * b) * self._texel(tex, sidx, ix, iy + 1)
        v = v + (a * b) * self._texel(tex, sidx, ix + 1, iy + 1)
        return np.where(ok, v, f32(0.0)).astype(f32)

    def sample_depth(self, sidx, x, y):
        """tex2DLayered of the depth maps: nearest, border 0."""
        sidx, x, y = np.broadcast_arrays(sidx, x, y)
        ok = self._guard(sidx, x, y)
        ix = np.floor(np.where(ok, x, f32(0.0))).astype(np.int64)
        iy = np.floor(np.where(ok, y, f32(0.0))).astype(np.int64)
        inb = ok & (ix >= 0) & (iy >= 0) & (ix < self.w[sidx]) & (iy < self.h[sidx])
        v = self.depth[sidx, np.where(inb, iy, 0), np.where(inb, ix, 0)]
        return np.where(inb, v, f32(0.0)).astype(f32)


# ---------------------------------------------------------------- geometry (every argument broadcasts; pose[..., POSE])

def point_at_depth(iK, row, col, depth):
    return depth * (iK[0] * col + iK[1]), depth * (iK[2] * row + iK[3]), depth


def propagate_depth(iK, depth1, normal1, row1, row2):
    """PropagateDepth :202-227; normal1 = (n0, n1, n2)."""
    x1 = depth1 * (iK[2] * f32(row1) + iK[3])
    y1 = depth1
    x2 = x1 + normal1[2]
    y2 = y1 - normal1[1]
    x4 = iK[2] * f32(row2) + iK[3]
    denom = x2 - x1 + x4 * (y1 - y2)
    nom = y1 * x2 - x1 * y2
    return np.where(np.abs(denom) < f32(1e-5), depth1, nom / denom).astype(f32)


def _dot3(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _rsqrt(x):
    return f32(1.0) / np.sqrt(x)


def viewing_angles(pose, point, normal):
    """ComputeViewingAngles :232-257 -> (cos_triangulation_angle, cos_incident_angle)."""
    SX = (pose[..., 16] - point[0], pose[..., 17] - point[1], pose[..., 18] - point[2])
    RX_inv_norm = _rsqrt(_dot3(point, point))
    SX_inv_norm = _rsqrt(_dot3(SX, SX))
    return _dot3(SX, point) * RX_inv_norm * SX_inv_norm, _dot3(SX, normal) * SX_inv_norm


def compose_homography(pose, iK, row, col, depth, normal):
    """ComposeHomography :259-315; row, col float32 (integers); normal = (n0, n1, n2) -> the nine entries of H."""
    K = [pose[..., i] for i in range(4)]
    R = [pose[..., 4 + i] for i in range(9)]
    T = [pose[..., 13 + i] for i in range(3)]
    dist = depth * (normal[0] * (iK[0] * col + iK[1]) + normal[1] * (iK[2] * row + iK[3]) + normal[2])
    inv_dist = f32(1.0) / dist
    N0, N1, N2 = inv_dist * normal[0], inv_dist * normal[1], inv_dist * normal[2]
    H = [None] * 9
    H[0] = iK[0] * (K[0] * (R[0] + N0 * T[0]) + K[1] * (R[6] + N0 * T[2]))
    H[1] = iK[2] * (K[0] * (R[1] + N1 * T[0]) + K[1] * (R[7] + N1 * T[2]))
    H[2] = (K[0] * (R[2] + N2 * T[0]) + K[1] * (R[8] + N2 * T[2]) +
            iK[1] * (K[0] * (R[0] + N0 * T[0]) + K[1] * (R[6] + N0 * T[2])) +
            iK[3] * (K[0] * (R[1] + N1 * T[0]) + K[1] * (R[7] + N1 * T[2])))
    H[3] = iK[0] * (K[2] * (R[3] + N0 * T[1]) + K[3] * (R[6] + N0 * T[2]))
    H[4] = iK[2] * (K[2] * (R[4] + N1 * T[1]) + K[3] * (R[7] + N1 * T[2]))
    H[5] = (K[2] * (R[5] + N2 * T[1]) + K[3] * (R[8] + N2 * T[2]) +
            iK[1] * (K[2] * (R[3] + N0 * T[1]) + K[3] * (R[6] + N0 * T[2])) +
            iK[3] * (K[2] * (R[4] + N1 * T[1]) + K[3] * (R[7] + N1 * T[2])))
    H[6] = iK[0] * (R[6] + N0 * T[2])
    H[7] = iK[2] * (R[7] + N1 * T[2])
    H[8] = R[8] + iK[1] * (R[6] + N0 * T[2]) + iK[3] * (R[7] + N1 * T[2]) + N2 * T[2]
    return H


def _hnorm(H, x, y):
    inv_z = f32(1.0) / (H[6] * x + H[7] * y + H[8])
    return inv_z * (H[0] * x + H[1] * y + H[2]), inv_z * (H[3] * x + H[4] * y + H[5])


def resolution_prob(H, row, col, radius):
    """ComputeResolutionProb :657-688."""
    r = f32(radius)
    s1, s2, s3, s4 = _hnorm(H, col - r, row - r), _hnorm(H, col - r, row + r), _hnorm(H, col + r, row + r), _hnorm(H, col + r, row - r)
    window = 2 * radius + 1
    ref_area = f32(window * window)
    src_area = np.abs(f32(0.5) * (s1[0] * s2[1] - s2[0] * s1[1] - s1[0] * s4[1] + s2[0] * s3[1] - s3[0] * s2[1] +
                                  s4[0] * s1[1] + s3[0] * s4[1] - s4[0] * s3[1]))
    return np.where(ref_area > src_area, src_area / ref_area, ref_area / src_area).astype(f32)


def geom_consistency_cost(c, sources, pose, K, iK, sidx, row, col, depth):
    """ComputeGeomConsistencyCost :451-514; K, iK of the reference image in the current rotation."""
    P = [pose[..., 19 + i] for i in range(12)]
    Q = [pose[..., 31 + i] for i in range(12)]
    max_cost = c["geom_max_cost"]
    fp = point_at_depth(iK, row, col, depth)
    inv_forward_z = f32(1.0) / (P[8] * fp[0] + P[9] * fp[1] + P[10] * fp[2] + P[11])
    src_col = inv_forward_z * (P[0] * fp[0] + P[1] * fp[1] + P[2] * fp[2] + P[3])
    src_row = inv_forward_z * (P[4] * fp[0] + P[5] * fp[1] + P[6] * fp[2] + P[7])
    src_depth = sources.sample_depth(sidx, src_col + f32(0.5), src_row + f32(0.5))
    src_col = src_col * src_depth
    src_row = src_row * src_depth
    bx = Q[0] * src_col + Q[1] * src_row + Q[2] * src_depth + Q[3]
    by = Q[4] * src_col + Q[5] * src_row + Q[6] * src_depth + Q[7]
    bz = Q[8] * src_col + Q[9] * src_row + Q[10] * src_depth + Q[11]
    inv_bz = f32(1.0) / bz
    backward_col = inv_bz * (K[0] * bx + K[1] * bz)
    backward_row = inv_bz * (K[2] * by + K[3] * bz)
    diff_col, diff_row = col - backward_col, row - backward_row
    cost = np.fmin(max_cost, np.sqrt(diff_col * diff_col + diff_row * diff_row))
    return np.where(src_depth == f32(0.0), max_cost, cost).astype(f32)


def photo_cost(c, sources, pose, iK, sidx, row, col, depth, normal, patch, center, ref_sum, ref_sq):
    """PhotoConsistencyCostComputer::Compute :348-445 for items of any leading shape L: pose [L, POSE], sidx, col, depth,
    center, ref_sum, ref_sq [L], normal three [L], patch [L, nt, nt] bytes of the window (already stepped); row a float32."""
    tform = compose_homography(pose, iK, row, col, depth, normal)
    step = f32(c["step"])
    ts = [step * t for t in tform]
    nt = len(c["offs"])
    col_start, row_start = col - f32(c["radius"]), row - f32(c["radius"])

    def walk(i0, i1, i2):
        start = tform[i0] * col_start + tform[i1] * row_start + tform[i2]
        lead = np.broadcast_arrays(start, ts[i1], ts[i0])
        base = np.cumsum(np.stack([lead[0]] + [lead[1]] * (nt - 1), axis=-1), axis=-1, dtype=f32)  # [L, nt]: one entry per window row
        return np.cumsum(np.stack([base] + [np.broadcast_to(lead[2][..., None], base.shape)] * (nt - 1), axis=-1), axis=-1, dtype=f32)

    col_src, row_src, z = walk(0, 1, 2), walk(3, 4, 5), walk(6, 7, 8)
    inv_z = f32(1.0) / z
    x = inv_z * col_src + f32(0.5)
    y = inv_z * row_src + f32(0.5)
    src_color = sources.sample(c["tex"], np.asarray(sidx)[..., None, None], x, y)
    ref_color = c["tex"][patch]
    diff = np.abs(patch.astype(np.int32) - np.asarray(center).astype(np.int32)[..., None, None])
    weight = c["w_spatial"].reshape(nt, nt) * c["w_color"][diff]
    weight_src = weight * src_color
    flat = lambda a: a.reshape(a.shape[:-2] + (nt * nt,))
    inv_w = f32(1.0) / seqsum(flat(weight))
    src_sum = seqsum(flat(weight_src)) * inv_w
    src_sq = seqsum(flat(weight_src * src_color)) * inv_w
    src_ref = seqsum(flat(weight_src * ref_color)) * inv_w
    ref_var = ref_sq - ref_sum * ref_sum
    src_var = src_sq - src_sum * src_sum
    covar = src_ref - ref_sum * src_sum
    cost = np.fmax(f32(0.0), np.fmin(f32(2.0), f32(1.0) - covar / np.sqrt(ref_var * src_var)))
    return np.where((ref_var < f32(1e-5)) | (src_var < f32(1e-5)), f32(2.0), cost).astype(f32)


# ---------------------------------------------------------------- LikelihoodComputer :595-729

def ncc_prob(c, cost):
    return exp32(cost * cost * c["inv_ncc"]) * c["ncc_norm"]


def forward_message(c, cost, prev):
    nc, un = f32(0.99999), f32(0.5)
    ch = f32(1.0) - nc
    emission = ncc_prob(c, cost)
    zn0 = (prev * ch + (f32(1.0) - prev) * nc) * un
    zn1 = (prev * nc + (f32(1.0) - prev) * ch) * emission
    return zn1 / (zn0 + zn1)


def backward_message(c, cost, prev):
    nc, un = f32(0.99999), f32(0.5)
    ch = f32(1.0) - nc
    emission = ncc_prob(c, cost)
    zn0 = prev * emission * ch + (f32(1.0) - prev) * un * nc
    zn1 = prev * emission * nc + (f32(1.0) - prev) * un * ch
    return zn1 / (zn0 + zn1)


def sel_prob(alpha, beta, prev, prev_weight):
    zn0 = (f32(1.0) - alpha) * (f32(1.0) - beta)
    zn1 = alpha * beta
    curr = zn1 / (zn0 + zn1)
    return prev_weight * prev + (f32(1.0) - prev_weight) * curr


def tri_prob(c, cos_tri):
    a = np.abs(cos_tri)
    scaled = f32(1.0) - (f32(1.0) - a) / (f32(1.0) - c["cos_min_tri"])
    likelihood = f32(1.0) - scaled * scaled
    return np.where(a > c["cos_min_tri"], np.fmin(f32(1.0), np.fmax(f32(0.0), likelihood)), f32(1.0)).astype(f32)


def inc_prob(c, cos_inc):
    x = f32(1.0) - np.fmax(f32(0.0), cos_inc)
    return exp32(x * x * c["inv_inc"])


# ---------------------------------------------------------------- initialisation

def init_random(c, key1, iK0, h, w, depth_min, depth_max):
    """FillWithRandomNumbers + InitNormalMap (:91-124, :732-743): stream (row, col, kind 0) per pixel."""
    rows, cols = np.meshgrid(np.arange(h, dtype=np.uint32), np.arange(w, dtype=np.uint32), indexing="ij")
    d = np.zeros((h, w), np.uint32)
    draw = lambda dd: uniform(c["seed"], key1, rows, cols, 0, dd)
    dmin, dmax = f32(depth_min), f32(depth_max)
    depth = draw(d) * (dmax - dmin) + dmin
    d = d + np.uint32(1)
    v1, v2, s = np.zeros((h, w), f32), np.zeros((h, w), f32), np.full((h, w), 2.0, f32)
    active = np.ones((h, w), bool)
    for _ in range(MAX_REJECT):
        if not active.any():
            break
        n1 = f32(2.0) * draw(d) - f32(1.0)
        n2 = f32(2.0) * draw(d + np.uint32(1)) - f32(1.0)
        ns = n1 * n1 + n2 * n2
        v1, v2, s = np.where(active, n1, v1), np.where(active, n2, v2), np.where(active, ns, s)
        d = np.where(active, d + np.uint32(2), d)
        active = active & ~(ns < f32(1.0))
    found = ~active
    s_norm = np.sqrt(np.where(found, f32(1.0) - s, f32(0.0)))
    normal = [np.where(found, f32(2.0) * v1 * s_norm, f32(0.0)), np.where(found, f32(2.0) * v2 * s_norm, f32(0.0)),
              np.where(found, f32(1.0) - f32(2.0) * s, f32(-1.0))]
    ray = (iK0[0] * cols.astype(f32) + iK0[1], iK0[2] * rows.astype(f32) + iK0[3], f32(1.0))
    flip = _dot3(normal, ray) > 0
    return depth.astype(f32), np.stack([np.where(flip, -n, n) for n in normal]).astype(f32)


def perturb_normal(c, rng, iK, row, colf, perturbation, normal):
    """PerturbNormal :134-190: the recursion as its four trials; only the columns still trying draw."""
    w = colf.shape[0]
    ray = (iK[0] * colf + iK[1], iK[2] * f32(row) + iK[3], f32(1.0))
    out = [n.copy() for n in normal]
    active = np.ones(w, bool)
    p = f32(perturbation)
    for _ in range(4):
        if not active.any():
            break
        a = [(rng.draw(active, k) - f32(0.5)) * p for k in range(3)]
        rng.advance(active, 3)
        s, co = [sin32(x) for x in a], [cos32(x) for x in a]
        s1, s2, s3 = s
        c1, c2, c3 = co
        R = [c2 * c3, -c2 * s3, s2,
             c1 * s3 + c3 * s1 * s2, c1 * c3 - s1 * s2 * s3, -c2 * s1,
             s1 * s3 - c1 * c3 * s2, c3 * s1 + c1 * s2 * s3, c1 * c2]
        pn = [R[0] * normal[0] + R[1] * normal[1] + R[2] * normal[2],
              R[3] * normal[0] + R[4] * normal[1] + R[5] * normal[2],
              R[6] * normal[0] + R[7] * normal[1] + R[8] * normal[2]]
        retry = _dot3(pn, ray) >= f32(0.0)
        inv_norm = _rsqrt(_dot3(pn, pn))
        done = active & ~retry
        for k in range(3):
            out[k] = np.where(done, pn[k] * inv_norm, out[k])
        active = active & retry
        p = f32(0.5) * p
    for k in range(3):  # four failed trials: the unperturbed normal
        out[k] = np.where(active, normal[k], out[k]).astype(f32)
    return out


class ColumnRng:
    """The stream (sweep number, column, kind 1) of every column of a sweep; a column's draw index counts up."""

    def __init__(self, c, key1, sweep_no, w):
        self.seed, self.key1, self.sweep_no = c["seed"], key1, sweep_no
        self.cols = np.arange(w, dtype=np.uint32)
        self.d = np.zeros(w, np.uint32)

    def draw(self, active=None, offset=0):
        return uniform(self.seed, self.key1, self.sweep_no, self.cols, 1, self.d + np.uint32(offset))

    def advance(self, active, count):
        self.d = np.where(active, self.d + np.uint32(count), self.d)


# ---------------------------------------------------------------- one sweep

def sweep(c, st, sources, K, iK, poses, sched, sweep_no, geom, filter_mode):
    """SweepFromTopToBottom :824-1133 on the state st of the current frame.  filter_mode: 0 none, 1 photometric, 2
    photometric and geometric.  poses [S][POSE], K / iK of this rotation."""
    perturbation, perturbation_normal, prev_weight = sched
    depth_map, normal_map, cost_map = st["depth"], st["normal"], st["cost"]
    h, w = depth_map.shape
    S = sources.S
    radius, offs = c["radius"], c["offs"]
    sel = np.zeros((S, h, w), f32)
    prev_sel = st["prev"]
    all_cols = np.ones(w, bool)

    beta = np.full((S, w), 0.5, f32)
    for row in range(h - 1, -1, -1):
        beta = backward_message(c, cost_map[:, row, :], beta)
        sel[:, row, :] = beta
    fwd = np.full((S, w), 0.5, f32)

    mask = np.zeros((S, h, w), np.uint8) if filter_mode else None
    rng = ColumnRng(c, st["key1"], sweep_no, w)
    colf = np.arange(w, dtype=f32)
    refp = np.pad(st["ref_img"], radius)
    prev_depth = depth_map[0].copy()
    prev_normal = [normal_map[k, 0].copy() for k in range(3)]
    pose_s = poses[:, None, :]          # [S, 1, POSE]
    sidx_s = np.arange(S)[:, None]      # [S, 1]

    for row in range(h):
        rowf = f32(row)
        band = refp[row:row + 2 * radius + 1:c["step"]]
        patch = np.lib.stride_tricks.sliding_window_view(band, 2 * radius + 1, axis=1)[:, :, ::c["step"]].transpose(1, 0, 2)  # [w, nt, nt]
        center = st["ref_img"][row]
        ref_sum, ref_sq = st["sum"][row], st["sq"][row]

        prev_depth = propagate_depth(iK, prev_depth, prev_normal, row - 1, row)
        curr_depth = depth_map[row].copy()
        curr_normal = [normal_map[k, row].copy() for k in range(3)]
        dmin, dmax = (f32(1.0) - perturbation) * curr_depth, (f32(1.0) + perturbation) * curr_depth
        rand_depth = rng.draw() * (dmax - dmin) + dmin
        rng.advance(all_cols, 1)
        rand_normal = perturb_normal(c, rng, iK, row, colf, perturbation_normal, curr_normal)

        if S:
            point = point_at_depth(iK, rowf, colf, curr_depth)
            alpha = forward_message(c, cost_map[:, row, :], fwd)
            sp = sel_prob(alpha, sel[:, row, :], prev_sel[:, row, :], prev_weight)
            cos_tri, cos_inc = viewing_angles(pose_s, point, curr_normal)
            H = compose_homography(pose_s, iK, rowf, colf, curr_depth, curr_normal)
            probs = sp * tri_prob(c, cos_tri) * inc_prob(c, cos_inc) * resolution_prob(H, rowf, colf, radius)
            inv_sum = f32(1.0) / seqsum(probs, axis=0)
            cdf = np.cumsum(np.concatenate([np.zeros((1, w), f32), probs * inv_sum], axis=0), axis=0, dtype=f32)[1:]

        depths = [curr_depth, prev_depth, rand_depth, curr_depth, rand_depth]
        normals = [curr_normal, prev_normal, rand_normal, rand_normal, curr_normal]
        costs = [np.zeros(w, f32) for _ in range(5)]
        ns = c["num_samples"]
        rand_prob = np.stack([rng.draw(None, k) for k in range(ns)]) - FLT_EPSILON  # [ns, w]
        rng.advance(all_cols, ns)
        if S:
            above = cdf[None, :, :] > rand_prob[:, None, :]  # [ns, S, w]
            valid = above.any(axis=1)
            src = np.where(valid, above.argmax(axis=1), 0)  # [ns, w]
            cols_i = np.arange(w)
            pose_i = poses[src]  # [ns, w, POSE]
            hyp_d = np.stack(depths[1:])[None]  # [1, 4, w]
            hyp_n = [np.stack([normals[k][j] for k in range(1, 5)])[None] for j in range(3)]
            if S <= ns:  # a cost depends on (source image, hypothesis, column) only: all of them once, then one per sample
                table = np.broadcast_to(photo_cost(c, sources, pose_s[:, None], iK, sidx_s[:, None], rowf, colf, hyp_d, hyp_n, patch, center,
                                                   ref_sum, ref_sq), (S, 4, w))
                pc = table[src[:, None, :], np.arange(4)[None, :, None], cols_i[None, None, :]]  # [ns, 4, w]
            else:
                pc = np.broadcast_to(photo_cost(c, sources, pose_i[:, None], iK, src[:, None, :], rowf, colf, hyp_d, hyp_n, patch, center,
                                                ref_sum, ref_sq), (ns, 4, w))
            if geom:
                gc = np.broadcast_to(geom_consistency_cost(c, sources, pose_i[:, None], K, iK, src[:, None, :], rowf, colf,
                                                           np.stack(depths)[None]), (ns, 5, w))
            for sample in range(ns):
                v = valid[sample]
                cur = costs[0] + cost_map[src[sample], row, cols_i]
                if geom:
                    cur = cur + c["geom_reg"] * gc[sample, 0]
                costs[0] = np.where(v, cur, costs[0])
                for k in range(1, 5):
                    cur = costs[k] + pc[sample, k - 1]
                    if geom:
                        cur = cur + c["geom_reg"] * gc[sample, k]
                    costs[k] = np.where(v, cur, costs[k])

        min_cost, min_idx = costs[0].copy(), np.zeros(w, np.int64)
        for k in range(1, 5):
            take = costs[k] <= min_cost
            min_cost, min_idx = np.where(take, costs[k], min_cost), np.where(take, k, min_idx)
        best_depth = np.choose(min_idx, depths).astype(f32)
        best_normal = [np.choose(min_idx, [normals[k][j] for k in range(5)]).astype(f32) for j in range(3)]
        depth_map[row] = best_depth
        for j in range(3):
            normal_map[j, row] = best_normal[j]

        if S:
            new_cost = photo_cost(c, sources, pose_s, iK, sidx_s, rowf, colf, best_depth, best_normal, patch, center, ref_sum, ref_sq)
            cost = np.where(min_idx == 0, cost_map[:, row, :], np.broadcast_to(new_cost, (S, w)))
            cost_map[:, row, :] = cost
            alpha = forward_message(c, cost, fwd)
            sel[:, row, :] = sel_prob(alpha, sel[:, row, :], prev_sel[:, row, :], prev_weight)
            fwd = alpha

        if filter_mode:
            if S:
                best_point = point_at_depth(iK, rowf, colf, best_depth)
                cos_tri, cos_inc = viewing_angles(pose_s, best_point, best_normal)
                skip = (cos_tri > c["filter_cos_min_tri"]) | (cos_inc <= f32(0.0))
                consistent = ~skip & (sel[:, row, :] >= c["filter_min_ncc_prob"])
                if filter_mode == 2:
                    gcost = geom_consistency_cost(c, sources, pose_s, K, iK, sidx_s, rowf, colf, best_depth)
                    consistent = consistent & (gcost <= c["filter_geom_max_cost"])
                mask[:, row, :] = consistent
                num_consistent = consistent.sum(axis=0)
            else:
                num_consistent = np.zeros(w, np.int64)
            filtered = num_consistent < c["filter_min_num_consistent"]
            depth_map[row] = np.where(filtered, f32(0.0), depth_map[row])
            for j in range(3):
                normal_map[j, row] = np.where(filtered, f32(0.0), normal_map[j, row])
            if S:
                mask[:, row, :] = np.where(filtered[None, :], 0, mask[:, row, :])

        prev_depth, prev_normal = best_depth, best_normal

    st["sel"] = sel
    return mask


# ---------------------------------------------------------------- PatchMatchCuda::Run

def patch_match(images, ref_idx, src_idxs, depth_min, depth_max, options):
    """One problem.  images: a list of dicts with data [h, w] uint8, K [9], R [9], T [3] float32 and, for geom_consistency,
    depth_map [h, w] / normal_map [3, h, w].  Returns depth [h, w], normal [3, h, w], sel_prob [S, h, w], mask [S, h, w] or None."""
    o = options
    assert o.check() is None, o.check()
    with np.errstate(all="ignore"):
        c = constants(o)
        src_idxs = list(src_idxs)
        geom = bool(o.geom_consistency)
        ref = images[ref_idx]
        h, w = ref["data"].shape
        S = len(src_idxs)
        K, iK, poses = init_transforms(images, ref_idx, src_idxs)
        sources = Sources(images, src_idxs, geom)
        ref_img, ref_sum, ref_sq = filter_ref_image(np.asarray(ref["data"], dtype=np.uint8), c)
        st = {"key1": int(ref_idx), "ref_img": ref_img, "sum": ref_sum.astype(f32), "sq": ref_sq.astype(f32)}
        if geom:
            st["depth"] = np.array(ref["depth_map"], dtype=f32)
            st["normal"] = np.array(ref["normal_map"], dtype=f32)
        else:
            st["depth"], st["normal"] = init_random(c, st["key1"], iK[0], h, w, depth_min, depth_max)
        st["prev"] = np.full((S, h, w), 0.5, f32)
        # ComputeInitialCost :760-803
        st["cost"] = np.zeros((S, h, w), f32)
        if S:
            colf = np.arange(w, dtype=f32)
            refp = np.pad(ref_img, c["radius"])
            for row in range(h):
                band = refp[row:row + 2 * c["radius"] + 1:c["step"]]
                patch = np.lib.stride_tricks.sliding_window_view(band, 2 * c["radius"] + 1, axis=1)[:, :, ::c["step"]].transpose(1, 0, 2)
                st["cost"][:, row, :] = photo_cost(c, sources, poses[0][:, None, :], iK[0], np.arange(S)[:, None], f32(row), colf, st["depth"][row],
                                                   [st["normal"][k, row] for k in range(3)], patch, ref_img[row], st["sum"][row], st["sq"][row])
        mask = None
        rot = 0
        for iteration in range(o.num_iterations):
            for sw in range(4):
                last = iteration == o.num_iterations - 1 and sw == 3
                mode = 0 if not (last and o.filter) else (2 if geom else 1)
                m = sweep(c, st, sources, K[rot], iK[rot], poses[rot], sweep_schedule(o, iteration, sw), iteration * 4 + sw, geom, mode)
                # Rotate :1659-1746
                rot = (rot + 1) % 4
                st["depth"] = rotate_map(st["depth"])
                st["normal"] = rotate_normal_map(st["normal"])
                st["ref_img"], st["sum"], st["sq"] = rotate_map(st["ref_img"]), rotate_map(st["sum"]), rotate_map(st["sq"])
                st["prev"] = rotate_map(st["sel"])
                st["cost"] = rotate_map(st["cost"])
                if m is not None:
                    mask = rotate_map(m)
        return {"depth": st["depth"], "normal": st["normal"], "sel_prob": st["prev"], "mask": mask}


def patch_match_stereo(images, problems, options):
    """The controller's two passes (patch_match.cc:201-215): the photometric pass of ALL problems with geom_consistency =
    filter = False, then, if geom_consistency is asked for, the geometric pass fed with those maps.  problems: a list of
    (ref_idx, src_idxs, depth_min, depth_max).  Returns the list of patch_match results of the last pass."""
    import copy
    o = options
    if not o.geom_consistency:
        return [patch_match(images, *p, o) for p in problems]
    photo = copy.copy(o)
    photo.geom_consistency, photo.filter = False, False
    first = [patch_match(images, *p, photo) for p in problems]
    fed = [dict(im) for im in images]
    for p, r in zip(problems, first):
        fed[p[0]]["depth_map"], fed[p[0]]["normal_map"] = r["depth"], r["normal"]
    return [patch_match(fed, *p, o) for p in problems]


def consistency_graph(mask, src_image_idxs):
    """GetConsistentImageIdxs :1217-1241: col, row, count, ids... of every pixel with a consistent source image, row-major."""
    out = []
    S, h, w = mask.shape
    for r in range(h):
        for cc in range(w):
            ids = [int(src_image_idxs[d]) for d in range(S) if mask[d, r, cc]]
            if ids:
                out += [cc, r, len(ids)] + ids
    return np.array(out, dtype=np.int32)
