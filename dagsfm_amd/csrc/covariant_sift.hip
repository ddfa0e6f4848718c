// covariant_sift.hip -- ExtractCovariantSiftFeaturesCPU (src/feature/sift.cc:428-598) on the device (DESIGN.md 21, and 27 for
// estimate_affine_shape): VLFeat's covdet (lib/VLFeat/covdet.c, DoG method) over its scalespace (scalespace.c), and
// vl_sift_calc_raw_descriptor (sift.c:1754-1903) on the warped patches, restated operation for operation in their own evaluation
// order, float where the source is float and double where it is double, plus COLMAP's loop around them.
//
//   k_sift_load / k_cov_upsample / k_sift_downsample   an octave's first level (scalespace.c:450-520, 699-801)
//   k_sift_conv_cols / k_sift_conv_rows   vl_imsmooth_f (imopv.c:644-679): vl_imconvcol_vf down the columns, then along the rows
//   k_cov_dog / k_sift_detect / k_sift_compact   the DoG response (covdet.c:1898-1907) and vl_find_local_extrema_3 (:1057-1126)
//   k_cov_refine      a lane per candidate: vl_refine_local_extreum_3 (:1206-1318), the elimination of mathop.c:905-1010 in double
//   k_cov_orient      a workgroup per feature: the 41 x 41 patch (vl_covdet_extract_patch_helper, :2362-2399), its smoothing, the
//                     polar gradient, the 36-bin histogram in double -- a lane per bin, walking all samples in order -- and its peaks
//                     (:2754-2838)
//   k_cov_affine_moments   a workgroup per feature and round of vl_covdet_extract_affine_shape_for_frame (:2462-2642): the 41 x 41
//                     patch, vl_imgradient_f, and the three masked sums of the second-moment matrix in double -- a lane per
//                     sum, walking all samples in order.  The loop around it (vl_svd2, the exits, the update of A) is the host's
//   k_cov_describe    THE HOT PATH: a workgroup of one wave per (feature, pooling scale).  The 31 x 31 patch is resampled from
//                     the level through L2 into LDS, its polar gradient stays in LDS, and a lane per (spatial cell, pair of
//                     orientation bins) walks that cell's samples in the reference's order from one constant table: no two
//                     lanes add to one bin, no atomics.  VLFeat's two normalisations follow (sift.c:1873-1902)
//   k_cov_pool        a workgroup per feature: the mean over the scales (an in-order float sum, one division), L1_ROOT / L2, the
//                     bytes and the UBC order (sift.cc:575-594, utils.cc:47-77)
// What the reference takes from the host libm is computed by the host libm here too, and all of it depends on the geometry or on
// one feature's frame, never on a pixel: the Gaussian taps, pow / log2 of the level choice, vl_svd2, atan2 / cos / sin of an
// orientation, the aaMask, the fast_expn window of the descriptor.  The non-extrema suppression (covdet.c:2104-2139, order
// dependent; over a grid) and std::sort run on the host.  The device does + - * / sqrt and comparisons only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ctx.h"
#include "sift_image_ops.h"

namespace {

constexpr int COV_WAVE = 64;          // lanes of k_cov_orient and k_cov_describe: one wave
constexpr int COV_OR_RES = 20;        // VL_COVDET_AA_PATCH_RESOLUTION
constexpr int COV_OR_SIDE = 2 * COV_OR_RES + 1;
constexpr int COV_OR_N = COV_OR_SIDE * COV_OR_SIDE;
constexpr double COV_OR_EXTENT = 9.0;  // VL_COVDET_AA_PATCH_EXTENT = 3 * VL_COVDET_AA_RELATIVE_INTEGRATION_SIGMA
constexpr int COV_OR_BINS = 36;       // VL_COVDET_OR_NUM_ORIENTATION_HISTOGAM_BINS
constexpr int COV_OR_MAX = 4;         // VL_COVDET_MAX_NUM_ORIENTATIONS
constexpr int COV_OR_TAPS = 16;       // deltaSigma <= 1 and stephat = 0.45: a half-width of at most ceil(3 / 0.45) = 7
constexpr int COV_D_RES = 15;         // kPatchResolution, sift.cc:519
constexpr int COV_D_SIDE = 2 * COV_D_RES + 1;
constexpr int COV_D_N = COV_D_SIDE * COV_D_SIDE;
constexpr double COV_D_EXTENT = 7.5;  // kPatchRelativeExtent
constexpr int COV_CELLS = 16;         // NBP x NBP
constexpr int COV_MAX_SCALES = 64;

struct CovCand {  // VlCovDetExtremum3 (its refined position and scores are floats) and the flag vl_refine_local_extreum_3 returns
  int32_t ok;
  float x, y, z, peak, edge;
};
struct CovFeature {  // VlCovDetFeature without laplacianScaleScore
  float x, y, a11, a12, a21, a22;
  int32_t o, s;
  float peak, edge, orient;
};
// one warped patch: the level (o, s) vl_covdet_extract_patch_helper chose, the map from the patch frame to it, and -- where the
// enclosing box leaves the level -- the geometry of the padded copy the source builds (covdet.c:2303-2359), which is read
// through cov_fetch instead of being built
struct CovPatch {
  double A[4], T[2];
  uint64_t level;          // the level's first sample in the scale space
  int32_t width, height;   // of the level
  int32_t padded;          // 0 the level itself, 1 the padded copy, 2 the zeroed buffer
  int32_t pw, ph;          // patchWidth, patchHeight
  int32_t y0i, c0, padx0, nadv, pady0, rmax;
  int32_t pad_;
};
struct CovOrientJob {
  CovPatch p;
  int32_t wx, wy;  // half-widths of filterx / filtery
  float tx[COV_OR_TAPS], ty[COV_OR_TAPS];
};
struct CovOrientOut {
  int32_t n, pad;
  double pos[COV_OR_MAX], score[COV_OR_MAX];  // i + di of a peak (covdet.c:2825-2826) and its height
};
struct CovSample {  // one addend of a spatial cell: the sample and what does not depend on the patch
  int32_t k;
  float win, ax, ay;
};

// ---- an octave's first level
// copy_and_upsample (scalespace.c:450-480): dst is 2 width x 2 height
__global__ void __launch_bounds__(SIFT_BLOCK) k_cov_upsample(float* __restrict__ dst, const float* __restrict__ src, uint32_t width, uint32_t height) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= width * height) return;
  const uint32_t y = i / width, x = i % width;
  const uint32_t ox = x + 1 < width ? 1u : 0u, oy = y + 1 < height ? width : 0u;
  const float v00 = src[i], v10 = src[i + ox], v01 = src[i + oy], v11 = src[i + ox + oy];
  float* d = dst + (size_t)(2 * y) * (2 * width) + 2 * x;
  d[0] = v00;
  d[1] = 0.5f * (v00 + v10);
  d[2 * width] = 0.5f * (v00 + v01);
  d[2 * width + 1] = 0.25f * (v00 + v01 + v10 + v11);
}

// _vl_dog_response as vl_covdet_detect calls it (covdet.c:1898-1907, 1966-1969): level s minus level s + 1
__global__ void __launch_bounds__(SIFT_BLOCK) k_cov_dog(float* __restrict__ dog, const float* __restrict__ oct, uint32_t nel, uint32_t n) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i < n) dog[i] = oct[i] - oct[(size_t)i + nel];
}

// vl_refine_local_extreum_3 (covdet.c:1206-1318) with vl_solve_linear_system_3 / vl_gaussian_elimination (mathop.c:839-1010)
__device__ __noinline__ void cov_refine_one(CovCand* out, const float* __restrict__ map, int w, int h, int depth, int x, int y, int z) {
  const int xo = 1, yo = w;
  const ptrdiff_t zo = (ptrdiff_t)w * h;
  double Dx = 0, Dy = 0, Dz = 0, Dxx = 0, Dyy = 0, Dzz = 0, Dxy = 0, Dxz = 0, Dyz = 0;
  double A[3 * 3], b[3];
  int dx = 0, dy = 0;
  bool err = false;
  const float* pt = map;
#define at(dx, dy, dz) (*(pt + (dx)*xo + (dy)*yo + (dz)*zo))
#define Aat(i, j) (A[(i) + (j)*3])
  #pragma unroll 1
  for (int iter = 0; iter < 5; ++iter) {
    x += dx;
    y += dy;
    pt = map + x * xo + y * yo + z * zo;
    Dx = 0.5 * (at(+1, 0, 0) - at(-1, 0, 0));
    Dy = 0.5 * (at(0, +1, 0) - at(0, -1, 0));
    Dz = 0.5 * (at(0, 0, +1) - at(0, 0, -1));
    Dxx = (at(+1, 0, 0) + at(-1, 0, 0) - 2.0 * at(0, 0, 0));
    Dyy = (at(0, +1, 0) + at(0, -1, 0) - 2.0 * at(0, 0, 0));
    Dzz = (at(0, 0, +1) + at(0, 0, -1) - 2.0 * at(0, 0, 0));
    Dxy = 0.25 * (at(+1, +1, 0) + at(-1, -1, 0) - at(-1, +1, 0) - at(+1, -1, 0));
    Dxz = 0.25 * (at(+1, 0, +1) + at(-1, 0, -1) - at(-1, 0, +1) - at(+1, 0, -1));
    Dyz = 0.25 * (at(0, +1, +1) + at(0, -1, -1) - at(0, -1, +1) - at(0, +1, -1));
    Aat(0, 0) = Dxx;
    Aat(1, 1) = Dyy;
    Aat(2, 2) = Dzz;
    Aat(0, 1) = Aat(1, 0) = Dxy;
    Aat(0, 2) = Aat(2, 0) = Dxz;
    Aat(1, 2) = Aat(2, 1) = Dyz;
    b[0] = -Dx;
    b[1] = -Dy;
    b[2] = -Dz;
    err = false;
    for (int j = 0; j < 3 && !err; ++j) {
      double maxa = 0, maxabsa = 0, tmp;
      int maxi = -1;
      for (int i = j; i < 3; ++i) {
        const double a = Aat(i, j), absa = fabs(a);
        if (absa > maxabsa) {
          maxa = a;
          maxabsa = absa;
          maxi = i;
        }
      }
      if (maxabsa < 1e-10) {
        err = true;
        break;
      }
      const int i = maxi;
      for (int jj = j; jj < 3; ++jj) {
        tmp = Aat(i, jj);
        Aat(i, jj) = Aat(j, jj);
        Aat(j, jj) = tmp;
        Aat(j, jj) /= maxa;
      }
      tmp = b[j];
      b[j] = b[i];
      b[i] = tmp;
      b[j] /= maxa;
      for (int ii = j + 1; ii < 3; ++ii) {
        const double f = Aat(ii, j);
        for (int jj = j; jj < 3; ++jj) Aat(ii, jj) -= f * Aat(j, jj);
        b[ii] -= f * b[j];
      }
    }
    if (err) {
      b[0] = 0;
      b[1] = 0;
      b[2] = 0;
      break;
    }
    for (int i = 2; i > 0; --i) {
      const double f = b[i];
      for (int ii = i - 1; ii >= 0; --ii) b[ii] -= f * Aat(ii, i);
    }
    dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
    dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
    if (dx == 0 && dy == 0) break;
  }
  const double peak = at(0, 0, 0) + 0.5 * (Dx * b[0] + Dy * b[1] + Dz * b[2]);
  const double alpha = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
  double edge;
  if (alpha < 0) {
    edge = (double)INFINITY;
  } else {
    const double q = 0.25 * alpha - 1;
    edge = (0.5 * alpha - 1) + sqrt((q > 0 ? q : 0) * alpha);  // VL_MAX(0.25 * alpha - 1, 0)
  }
#undef at
#undef Aat
  const float rx = (float)(x + b[0]), ry = (float)(y + b[1]), rz = (float)(z + b[2]);  // the range checks read the floats
  out->x = rx;
  out->y = ry;
  out->z = rz;
  out->peak = (float)peak;
  out->edge = (float)edge;
  out->ok = !err && fabs(b[0]) < 1.5 && fabs(b[1]) < 1.5 && fabs(b[2]) < 1.5 && 0 <= rx && rx <= w - 1 && 0 <= ry && ry <= h - 1 && 0 <= rz &&
            rz <= depth - 1;
}
__global__ void __launch_bounds__(SIFT_BLOCK) k_cov_refine(CovCand* __restrict__ out, const uint32_t* __restrict__ cand, uint32_t n,
                                                           const float* __restrict__ dog, int w, int h, int depth) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cand[i];  // flag index (s, y, x) of k_sift_detect: z = s + 1
  cov_refine_one(out + i, dog, w, h, depth, (int)(c % (uint32_t)w), (int)(c / (uint32_t)w % (uint32_t)h), (int)(c / ((uint32_t)w * (uint32_t)h)) + 1);
}

// ---- the warped patch
// sample (px, py) of what the resampling loop of vl_covdet_extract_patch_helper reads: the level, or the padded copy of
// covdet.c:2322-2345 -- its central band copies the level's columns from c0 on, padx0 times the first and every column from
// patchWidth - padx1 - 2 on the one the copy loop stopped at; the rows above and below repeat the band's first and last
__device__ inline float cov_fetch(const float* __restrict__ gss, const CovPatch& p, long px, long py) {
  const float* level = gss + p.level;
  if (p.padded == 0) {
    px = px < 0 ? 0 : (px > p.width - 1 ? p.width - 1 : px);  // in range by construction (covdet.c:2388-2389); never leave the level
    py = py < 0 ? 0 : (py > p.height - 1 ? p.height - 1 : py);
    return level[(size_t)py * p.width + px];
  }
  if (p.padded == 2) return 0.0f;
  const long re = py < p.pady0 ? p.pady0 : (py > p.rmax ? p.rmax : py);
  long yi = p.y0i + re;
  long adv = px - p.padx0;
  adv = adv < 0 ? 0 : (adv > p.nadv ? p.nadv : adv);
  long c = p.c0 + adv;
  yi = yi < 0 ? 0 : (yi > p.height - 1 ? p.height - 1 : yi);
  c = c < 0 ? 0 : (c > p.width - 1 ? p.width - 1 : c);
  return level[(size_t)yi * p.width + c];
}
// the bilinear resampling (covdet.c:2365-2399) of SIDE x SIDE samples into LDS, a sample per lane and step
template <int SIDE>
__device__ inline void cov_resample(float* __restrict__ patch, const float* __restrict__ gss, const CovPatch& p, const double* __restrict__ hat) {
  for (int k = (int)threadIdx.x; k < SIDE * SIDE; k += COV_WAVE) {
    const double yhat = hat[k / SIDE], xhat = hat[k % SIDE];
    const double rx = p.A[2] * yhat + p.T[0];
    const double ry = p.A[3] * yhat + p.T[1];
    const double x = p.A[0] * xhat + rx;
    const double y = p.A[1] * xhat + ry;
    const long xi = vl_floor_d(x), yi = vl_floor_d(y);
    const double i00 = cov_fetch(gss, p, xi, yi);
    const double i10 = cov_fetch(gss, p, xi + 1, yi);
    const double i01 = cov_fetch(gss, p, xi, yi + 1);
    const double i11 = cov_fetch(gss, p, xi + 1, yi + 1);
    const double wx = x - xi, wy = y - yi;
    patch[k] = (float)((1.0 - wy) * ((1.0 - wx) * i00 + wx * i10) + wy * ((1.0 - wx) * i01 + wx * i11));
  }
}
// one sample of vl_imgradient_polar_f (imopv.c:875-974): one-sided differences on the borders
template <int SIDE>
__device__ inline void cov_polar(const float* __restrict__ img, int k, float* mod, float* ang) {
  const int x = k % SIDE, y = k / SIDE;
  const float* src = img + k;
  float gx, gy;
  if (x == 0)
    gx = src[1] - src[0];
  else if (x == SIDE - 1)
    gx = src[0] - src[-1];
  else
    gx = 0.5f * (src[1] - src[-1]);
  if (y == 0)
    gy = src[SIDE] - src[0];
  else if (y == SIDE - 1)
    gy = src[0] - src[-SIDE];
  else
    gy = 0.5f * (src[SIDE] - src[-SIDE]);
  *mod = vl_fast_sqrt(gx * gx + gy * gy);
  *ang = vl_mod_2pi((float)(vl_fast_atan2(gy, gx) + 2 * kVlPi));
}

// vl_covdet_extract_orientations_for_frame (covdet.c:2754-2838) up to the peaks; the host adds theta0 and sorts
__global__ void __launch_bounds__(COV_WAVE) k_cov_orient(const CovOrientJob* __restrict__ jobs, const float* __restrict__ gss,
                                                         const double* __restrict__ hat, const float* __restrict__ mask,
                                                         CovOrientOut* __restrict__ out) {
  __shared__ float a[COV_OR_N], b[COV_OR_N];
  __shared__ int32_t bins[COV_OR_N];
  __shared__ double add1[COV_OR_N], add2[COV_OR_N];
  __shared__ double hist[COV_OR_BINS];
  const CovOrientJob& job = jobs[blockIdx.x];
  const int lane = (int)threadIdx.x;
  cov_resample<COV_OR_SIDE>(a, gss, job.p, hat);
  __syncthreads();
  // vl_imsmooth_f on the patch: filtery down the columns, filterx along the rows; out(p) = sum_j in(clamp(p - W + j)) taps[2 W - j]
  for (int k = lane; k < COV_OR_N; k += COV_WAVE) {
    const int x = k % COV_OR_SIDE, y = k / COV_OR_SIDE, W = job.wy;
    float acc = 0;
    #pragma unroll 1
    for (int j = 0; j <= 2 * W; ++j) {
      int q = y - W + j;
      q = q < 0 ? 0 : (q > COV_OR_SIDE - 1 ? COV_OR_SIDE - 1 : q);
      acc += a[q * COV_OR_SIDE + x] * job.ty[2 * W - j];
    }
    b[k] = acc;
  }
  __syncthreads();
  for (int k = lane; k < COV_OR_N; k += COV_WAVE) {
    const int x = k % COV_OR_SIDE, y = k / COV_OR_SIDE, W = job.wx;
    float acc = 0;
    #pragma unroll 1
    for (int j = 0; j <= 2 * W; ++j) {
      int q = x - W + j;
      q = q < 0 ? 0 : (q > COV_OR_SIDE - 1 ? COV_OR_SIDE - 1 : q);
      acc += b[y * COV_OR_SIDE + q] * job.tx[2 * W - j];
    }
    a[k] = acc;
  }
  __syncthreads();
  const double binExtent = 2 * kVlPi / COV_OR_BINS;
  for (int k = lane; k < COV_OR_N; k += COV_WAVE) {
    float m, an;
    cov_polar<COV_OR_SIDE>(a, k, &m, &an);
    const double modulus = m, angle = an, weight = mask[k];
    const double x = angle / binExtent;
    const long bin = vl_floor_d(x);
    const double w2 = x - bin;
    const double w1 = 1.0 - w2;
    bins[k] = (int32_t)((bin + COV_OR_BINS) % COV_OR_BINS);
    add1[k] = w1 * (modulus * weight);
    add2[k] = w2 * (modulus * weight);
  }
  __syncthreads();
  if (lane < COV_OR_BINS) {  // bin `lane` receives its addends in sample order
    double hsum = 0;
    const int prev = (lane + COV_OR_BINS - 1) % COV_OR_BINS;
    #pragma unroll 1
    for (int k = 0; k < COV_OR_N; ++k) {
      const int b0 = bins[k];
      if (b0 == lane) hsum += add1[k];
      if (b0 == prev) hsum += add2[k];
    }
    hist[lane] = hsum;
  }
  __syncthreads();
  if (lane != 0) return;
  enum { nb = COV_OR_BINS };
  #pragma unroll 1
  for (int iter = 0; iter < 6; iter++) {
    double prev = hist[nb - 1];
    const double first = hist[0];
    int i;
    #pragma unroll 1
    for (i = 0; i < nb - 1; ++i) {
      const double curr = (prev + hist[i] + hist[(i + 1) % nb]) / 3.0;
      prev = hist[i];
      hist[i] = curr;
    }
    hist[i] = (prev + hist[i] + first) / 3.0;
  }
  double maxPeak = 0;
  #pragma unroll 1
  for (int i = 0; i < nb; ++i) maxPeak = maxPeak > hist[i] ? maxPeak : hist[i];  // VL_MAX
  CovOrientOut r;
  r.n = 0;
  r.pad = 0;
  for (int i = 0; i < COV_OR_MAX; ++i) r.pos[i] = r.score[i] = 0;
  #pragma unroll 1
  for (int i = 0; i < nb; ++i) {
    const double h0 = hist[i], hm = hist[(i - 1 + nb) % nb], hp = hist[(i + 1 + nb) % nb];
    if (h0 > 0.8 * maxPeak && h0 > hm && h0 > hp) {
      const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
      r.pos[r.n] = i + di;
      r.score[r.n] = h0;
      r.n += 1;
      if (r.n >= COV_OR_MAX) break;
    }
  }
  out[blockIdx.x] = r;
}

// One pass of vl_covdet_extract_affine_shape_for_frame between its two vl_svd2 (covdet.c:2530-2562) for one feature: the patch
// (aaAccurateSmoothing is off: no smoothing), vl_imgradient_f (imopv.c:722-829) and lxx, lyy, lxy -- out[3 f .. 3 f + 2] in that
// order.  Each sum is one lane's chain over the 1681 addends in sample order; the products lx * lx * mask (left to right, the
// floats widened) do not depend on the chain, so the chain costs one FP64 addition an addend.  A zeroed patch (padded == 2)
// gives three exact zeros: every addend is + 0.
__global__ void __launch_bounds__(COV_WAVE) k_cov_affine_moments(const CovPatch* __restrict__ jobs, const float* __restrict__ gss,
                                                                 const double* __restrict__ hat, const float* __restrict__ mask,
                                                                 double* __restrict__ out) {
  __shared__ float patch[COV_OR_N], gx[COV_OR_N], gy[COV_OR_N];
  const CovPatch& p = jobs[blockIdx.x];
  const int lane = (int)threadIdx.x;
  cov_resample<COV_OR_SIDE>(patch, gss, p, hat);
  __syncthreads();
  for (int k = lane; k < COV_OR_N; k += COV_WAVE) {
    const int x = k % COV_OR_SIDE, y = k / COV_OR_SIDE;
    const float* src = patch + k;
    float dx, dy;
    if (x == 0)
      dx = src[1] - src[0];
    else if (x == COV_OR_SIDE - 1)
      dx = src[0] - src[-1];
    else
      dx = (float)(0.5 * (src[1] - src[-1]));
    if (y == 0)
      dy = src[COV_OR_SIDE] - src[0];
    else if (y == COV_OR_SIDE - 1)
      dy = src[0] - src[-COV_OR_SIDE];
    else
      dy = (float)(0.5 * (src[COV_OR_SIDE] - src[-COV_OR_SIDE]));
    gx[k] = dx;
    gy[k] = dy;
  }
  __syncthreads();
  if (lane >= 3) return;
  const float* u = lane == 1 ? gy : gx;  // lane 0: lx lx, lane 1: ly ly, lane 2: lx ly
  const float* v = lane == 0 ? gx : gy;
  double acc = 0;
  #pragma unroll 8
  for (int k = 0; k < COV_OR_N; ++k) {
    const double a = u[k], b = v[k], m = mask[k];
    acc += a * b * m;
  }
  out[3 * (size_t)blockIdx.x + lane] = acc;
}

// normalize_histogram (sift.c:1702-1718): the sum of squares left to right by one lane, the division by all
__device__ inline void cov_normalize(float* descr, float* norm_slot) {
  if (threadIdx.x == 0) {
    float norm = 0.0f;
    #pragma unroll 1
    for (int i = 0; i < 128; ++i) norm += descr[i] * descr[i];
    *norm_slot = vl_fast_sqrt(norm) + kVlEpsF;
  }
  __syncthreads();
  const float norm = *norm_slot;
  for (int i = (int)threadIdx.x; i < 128; i += COV_WAVE) descr[i] /= norm;
  __syncthreads();
}

// One (feature, pooling scale): vl_covdet_extract_patch_for_frame + vl_imgradient_polar_f + vl_sift_calc_raw_descriptor at the
// patch centre with sigma = 2, angle0 = 0, magnif = 3 (sift.cc:551-573).  W = 21 covers the 31 x 31 patch, so every sample is
// visited, row by row; nx, ny, the window, the spatial bins and weights are the same for every patch (table), only the modulus
// and the angle vary.  Lane l owns the cell l / 4 and the orientation bins 2 (l % 4), 2 (l % 4) + 1 and walks the cell's
// samples in the table's (= the source's) order.
__global__ void __launch_bounds__(COV_WAVE) k_cov_describe(const CovPatch* __restrict__ items, const float* __restrict__ gss,
                                                           const double* __restrict__ hat, const CovSample* __restrict__ table,
                                                           const int32_t* __restrict__ counts, float* __restrict__ raw) {
  __shared__ float patch[COV_D_N], mod[COV_D_N], nts[COV_D_N];
  __shared__ float descr[128];
  __shared__ float norm_slot;
  const CovPatch& p = items[blockIdx.x];
  const int lane = (int)threadIdx.x;
  cov_resample<COV_D_SIDE>(patch, gss, p, hat);
  __syncthreads();
  for (int k = lane; k < COV_D_N; k += COV_WAVE) {
    float m, an;
    cov_polar<COV_D_SIDE>(patch, k, &m, &an);
    const float theta = vl_mod_2pi(an);  // angle - angle0 with angle0 = 0 (sift.c:1818)
    mod[k] = m;
    nts[k] = (float)(8 * theta / (2 * kVlPi));  // NBO * theta / (2 * VL_PI)
  }
  __syncthreads();
  {
    const int cell = lane >> 2, t0 = 2 * (lane & 3), t1 = t0 + 1;
    const int n = counts[cell];
    float acc0 = 0.0f, acc1 = 0.0f;
    #pragma unroll 1
    for (int j = 0; j < n; ++j) {
      const CovSample e = table[j * COV_CELLS + cell];
      const float nt = nts[e.k];
      const int bint = (int)vl_floor_f(nt);
      const float rbint = nt - bint;
      const float w = e.win * mod[e.k] * e.ax * e.ay;
      const float w0 = w * fabsf(1 - rbint), w1 = w * fabsf(0 - rbint);
      const int b0 = bint % 8, b1 = (bint + 1) % 8;
      if (b0 == t0) acc0 += w0;
      if (b0 == t1) acc1 += w0;
      if (b1 == t0) acc0 += w1;
      if (b1 == t1) acc1 += w1;
    }
    descr[cell * 8 + t0] = acc0;
    descr[cell * 8 + t1] = acc1;
  }
  __syncthreads();
  cov_normalize(descr, &norm_slot);
  for (int i = lane; i < 128; i += COV_WAVE)
    if (descr[i] > 0.2) descr[i] = (float)0.2;
  __syncthreads();
  cov_normalize(descr, &norm_slot);
  for (int i = lane; i < 128; i += COV_WAVE) raw[128 * (size_t)blockIdx.x + i] = descr[i];
}

// colwise().mean() over the scales of a feature (sift.cc:577), L1RootNormalize / L2Normalize, FeatureDescriptorsToUnsignedByte
// (utils.cc:47-77; the sums left to right) and the UBC bin order (sift.cc:58-74)
__global__ void __launch_bounds__(128) k_cov_pool(const float* __restrict__ raw, int scales, int pooled, int l2, uint8_t* __restrict__ out) {
  __shared__ float d[128];
  __shared__ float norm_slot;
  const int i = (int)threadIdx.x;
  const float* r = raw + (size_t)blockIdx.x * scales * 128;
  float v = r[i];
  if (pooled) {
    #pragma unroll 1
    for (int s = 1; s < scales; ++s) v += r[s * 128 + i];
    v /= (float)scales;
  }
  d[i] = v;
  __syncthreads();
  if (i == 0) {
    float norm = 0.0f;
    if (l2) {
      #pragma unroll 1
      for (int k = 0; k < 128; ++k) norm += d[k] * d[k];
    } else {
      #pragma unroll 1
      for (int k = 0; k < 128; ++k) norm += fabsf(d[k]);
    }
    norm_slot = norm;
  }
  __syncthreads();
  float norm = norm_slot;
  const bool scale = !l2 || norm > 0.0f;  // Eigen's normalized() leaves a zero row as it is
  if (l2) norm = sqrtf(norm);
  v = scale ? v / norm : v;
  if (!l2) v = sqrtf(v);
  const float rr = roundf(512.0f * v);
  const float lo = (0.0f < rr) ? rr : 0.0f;        // std::max(0, r): 0 for a NaN
  const float cl = (lo < 255.0f) ? lo : 255.0f;    // std::min(255, .)
  const int t = i & 7;
  out[128 * (size_t)blockIdx.x + (i & ~7) + (t ? 8 - t : 0)] = (uint8_t)cl;
}

// ---- host half
inline long cov_floor(double x) {  // vl_floor_d
  const long xi = (long)x;
  if (x >= 0 || (double)xi == x) return xi;
  return xi - 1;
}
inline int cov_shift(int x, int n) { return n >= 0 ? x << n : x >> -n; }  // VL_SHIFT_LEFT

// _vl_new_gaussian_fitler_f (imopv.c:620-642), by the host libm as the reference's; appended to taps, returns the half-width
int cov_taps(double sigma, std::vector<float>* taps) {
  const size_t W = (size_t)std::ceil(sigma * 3.0), at = taps->size();
  taps->resize(at + 2 * W + 1);
  float* filter = taps->data() + at;
  float mass = (float)1.0;
  filter[W] = 1.0;
  for (size_t i = 1; i <= W; ++i) {
    const double x = (double)i / sigma;
    const double g = std::exp(-0.5 * x * x);
    mass += g + g;
    filter[W - i] = g;
    filter[W + i] = g;
  }
  for (size_t i = 0; i < 2 * W + 1; ++i) filter[i] /= mass;
  return (int)W;
}

// vl_lapack_dlasv2 and vl_svd2 (mathop.c:640-826): the singular values S[0], S[3] and the rotations of a 2 x 2 matrix
inline int cov_sign(double x) { return x < 0.0 ? -1 : +1; }
void cov_dlasv2(double* smin, double* smax, double* sv, double* cv, double* su, double* cu, double f, double g, double h) {
  double svt = 0, cvt = 0, sut = 0, cut = 0;
  double ft = f, gt = g, ht = h;
  double fa = std::fabs(f), ga = std::fabs(g), ha = std::fabs(h);
  int pmax = 1, swap = 0, glarge = 0, tsign = 1;
  double tmp;
  if (fa < ha) {
    pmax = 3;
    tmp = ft, ft = ht, ht = tmp;
    tmp = fa, fa = ha, ha = tmp;
    swap = 1;
  }
  if (ga == 0.0) {
    *smin = ha;
    *smax = fa;
    cut = 1.0, sut = 0.0;
    cvt = 1.0, svt = 0.0;
  } else {
    if (ga > fa) {
      pmax = 2;
      if ((fa / ga) < kVlEpsD) {
        glarge = 1;
        *smax = ga;
        if (ha > 1.0)
          *smin = fa / (ga / ha);
        else
          *smin = (fa / ga) * ha;
        cut = 1.0, sut = ht / gt;
        cvt = 1.0, svt = ft / gt;
      }
    }
    if (glarge == 0) {
      const double fmh = fa - ha;
      const double d = fmh == fa ? 1.0 : fmh / fa;
      const double q = gt / ft;
      const double s = 2.0 - d;
      const double dd = d * d, qq = q * q, ss = s * s;
      const double spq = std::sqrt(ss + qq);
      const double dpq = d == 0.0 ? std::fabs(q) : std::sqrt(dd + qq);
      const double a = 0.5 * (spq + dpq);
      *smin = ha / a;
      *smax = fa * a;
      if (qq == 0.0) {
        if (d == 0.0)
          tmp = cov_sign(ft) * 2 * cov_sign(gt);
        else
          tmp = gt / (cov_sign(ft) * fmh) + q / s;
      } else {
        tmp = (q / (spq + s) + q / (dpq + d)) * (1.0 + a);
      }
      const double tt = std::sqrt(tmp * tmp + 4.0);
      cvt = 2.0 / tt;
      svt = tmp / tt;
      cut = (cvt + svt * q) / a;
      sut = (ht / ft) * svt / a;
    }
  }
  if (swap == 1) {
    *cu = svt, *su = cvt;
    *cv = sut, *sv = cut;
  } else {
    *cu = cut, *su = sut;
    *cv = cvt, *sv = svt;
  }
  if (pmax == 1) tsign = cov_sign(*cv) * cov_sign(*cu) * cov_sign(f);
  if (pmax == 2) tsign = cov_sign(*sv) * cov_sign(*cu) * cov_sign(g);
  if (pmax == 3) tsign = cov_sign(*sv) * cov_sign(*su) * cov_sign(h);
  *smax = (tsign < 0 ? -1 : +1) * (*smax);
  *smin = (tsign * cov_sign(f) * cov_sign(h) < 0 ? -1 : +1) * (*smin);
}
void cov_svd2(double* S, double* U, double* V, const double* M) {
  const double m11 = M[0], m21 = M[1], m12 = M[2], m22 = M[3];
  double cu1 = m11, su1 = m21;
  const double norm = std::sqrt(cu1 * cu1 + su1 * su1);
  double cu2, su2, cv2, sv2, smin, smax;
  cu1 /= norm;
  su1 /= norm;
  const double f = cu1 * m11 + su1 * m21;
  const double g = cu1 * m12 + su1 * m22;
  const double h = -su1 * m12 + cu1 * m22;
  cov_dlasv2(&smin, &smax, &sv2, &cv2, &su2, &cu2, f, g, h);
  S[0] = smax, S[1] = 0, S[2] = 0, S[3] = smin;
  U[0] = cu2 * cu1 - su2 * su1;
  U[1] = su2 * cu1 + cu2 * su1;
  U[2] = -cu2 * su1 - su2 * cu1;
  U[3] = -su2 * su1 + cu2 * cu1;
  V[0] = cv2, V[1] = sv2, V[2] = -sv2, V[3] = cv2;
}

// vl_solve_linear_system_2 over vl_gaussian_elimination (mathop.c:872-1016) for a 2 x 3 system, column major: a singular
// matrix leaves x with what stands in the last column when the elimination gives up
void cov_solve2(double* x, const double* A, const double* b) {
  double M[2 * 3] = {A[0], A[1], A[2], A[3], b[0], b[1]};
  const int numRows = 2, numColumns = 3;
#define Mat(i, j) M[(i) + (j)*numRows]
  bool ok = true;
  for (int j = 0; j < numRows && ok; ++j) {
    double maxa = 0, maxabsa = 0, tmp;
    int maxi = -1;
    for (int i = j; i < numRows; ++i) {
      const double a = Mat(i, j), absa = std::fabs(a);
      if (absa > maxabsa) {
        maxa = a;
        maxabsa = absa;
        maxi = i;
      }
    }
    if (maxabsa < 1e-10) {
      ok = false;
      break;
    }
    const int i = maxi;
    for (int jj = j; jj < numColumns; ++jj) {
      tmp = Mat(i, jj);
      Mat(i, jj) = Mat(j, jj);
      Mat(j, jj) = tmp;
      Mat(j, jj) /= maxa;
    }
    for (int ii = j + 1; ii < numRows; ++ii) {
      const double f = Mat(ii, j);
      for (int jj = j; jj < numColumns; ++jj) Mat(ii, jj) -= f * Mat(j, jj);
    }
  }
  if (ok)
    for (int i = numRows - 1; i > 0; --i)
      for (int ii = i - 1; ii >= 0; --ii) {
        const double f = Mat(ii, i);
        for (int j = numRows; j < numColumns; ++j) Mat(ii, j) -= f * Mat(i, j);
      }
#undef Mat
  x[0] = M[4];
  x[1] = M[5];
}

struct CovGeom {  // VlScaleSpaceGeometry of the detector's scale space (covdet.c:1699-1718)
  int width = 0, height = 0, first = 0, last = 0, R = 0, smin = -1, smax = 0;
  double base = 0;
  std::vector<uint64_t> oct;  // an octave's first sample
  int ow(int o) const { return cov_shift(width, -o); }
  int oh(int o) const { return cov_shift(height, -o); }
  uint64_t level(int o, int s) const { return oct[o - first] + (uint64_t)ow(o) * oh(o) * (uint64_t)(s - smin); }
};

// vl_covdet_extract_patch_helper up to the resampling loop (covdet.c:2222-2359): the level and the patch-to-level map
void cov_plan_patch(const CovGeom& g, CovPatch* p, double* sigma1, double* sigma2, double extent, double sigma, const double A_[4],
                    const double T_[2], double d1, double d2) {
  double A[4] = {A_[0], A_[1], A_[2], A_[3]};
  double T[2] = {T_[0], T_[1]};
  const double factor = 1.0 / (d1 < d2 ? d1 : d2);
  long o, s = 0;
  double sigma_ = 0;
  auto pick = [&](long oo) {
    long ss = cov_floor(std::log2(sigma / (factor * g.base)) - oo);
    ss = ss > g.smin ? ss : g.smin;
    ss = ss < g.smax ? ss : g.smax;
    return ss;
  };
  for (o = g.first + 1; o <= g.last; ++o) {
    s = pick(o);
    sigma_ = g.base * std::pow(2.0, o + (double)s / g.R);
    if (factor * sigma_ > sigma) {
      o--;
      break;
    }
  }
  o = o < g.last ? o : g.last;
  s = pick(o);
  sigma_ = g.base * std::pow(2.0, o + (double)s / g.R);
  if (sigma1) *sigma1 = sigma_ / d1;
  if (sigma2) *sigma2 = sigma_ / d2;
  const long width = g.ow((int)o), height = g.oh((int)o);
  const double step = std::pow(2.0, (double)o);
  for (double& a : A) a /= step;
  T[0] /= step;
  T[1] /= step;
  memset(p, 0, sizeof(*p));
  p->level = g.level((int)o, (int)s);
  p->width = (int32_t)width;
  p->height = (int32_t)height;
  double x0 = +INFINITY, x1 = -INFINITY, y0 = +INFINITY, y1 = -INFINITY;
  const double boxx[4] = {extent, extent, -extent, -extent};
  const double boxy[4] = {-extent, extent, extent, -extent};
  for (int i = 0; i < 4; ++i) {
    const double x = A[0] * boxx[i] + A[2] * boxy[i] + T[0];
    const double y = A[1] * boxx[i] + A[3] * boxy[i] + T[1];
    x0 = x0 < x ? x0 : x;  // VL_MIN / VL_MAX
    x1 = x1 > x ? x1 : x;
    y0 = y0 < y ? y0 : y;
    y1 = y1 > y ? y1 : y;
  }
  auto to_index = [](double v) {  // a frame far outside the image: keep the conversion defined
    return (long)(v < -1e8 ? -1e8 : (v > 1e8 ? 1e8 : v));
  };
  const long x0i = to_index(std::floor(x0) - 1), y0i = to_index(std::floor(y0) - 1);
  const long x1i = to_index(std::ceil(x1) + 1), y1i = to_index(std::ceil(y1) + 1);
  if (x0i < 0 || x1i > width - 1 || y0i < 0 || y1i > height - 1) {
    const long padx0 = std::max(0l, -x0i), pady0 = std::max(0l, -y0i);
    const long padx1 = std::max(0l, x1i - (width - 1)), pady1 = std::max(0l, y1i - (height - 1));
    const long patchWidth = x1i - x0i + 1, patchHeight = y1i - y0i + 1;
    p->pw = (int32_t)patchWidth;
    p->ph = (int32_t)patchHeight;
    if (pady0 < patchHeight - pady1) {
      p->padded = 1;
      p->y0i = (int32_t)y0i;
      p->c0 = (int32_t)std::min(std::max(0l, x0i), width - 1);
      p->padx0 = (int32_t)padx0;
      p->nadv = (int32_t)std::max(0l, patchWidth - padx1 - 2 - padx0);  // the samples the copy loop of :2328 advances over
      p->pady0 = (int32_t)pady0;
      p->rmax = (int32_t)(patchHeight - pady1 - 1);
    } else {
      p->padded = 2;
    }
    T[0] -= x0i;
    T[1] -= y0i;
  }
  for (int i = 0; i < 4; ++i) p->A[i] = A[i];
  p->T[0] = T[0];
  p->T[1] = T[1];
}

}  // namespace

struct CovSiftState {
  enum { img, fimg, gss, tmp, dog, flags, counts, offs, cand, refined, taps, consts, table, ojobs, oout, items, raw, desc8, COUNT };
  DevBuf buf[COUNT];
  bool consts_ready = false;
  int32_t cell_counts[COV_CELLS] = {0};
  size_t at_hat31 = 0, at_hat41 = 0, at_mask = 0, at_counts = 0;  // byte offsets in consts
  DevEvent ev[8];
  double stage_ms[DSM_COVARIANT_SIFT_STAGES] = {0};
  // the last successful call of either entry
  bool valid = false, have_raw = false;
  uint32_t n = 0, scales = 0;
  std::vector<int32_t> os;
  std::vector<float> scores;
  // the shape adaptation of the last successful dsm_extract_covariant_sift_affine
  bool affine_valid = false;
  uint32_t affine_rounds = 0, affine_exits[4] = {0}, affine_active[DSM_AFFINE_SHAPE_MAX_ROUNDS] = {0};
};

void dsm_covariant_sift_destroy(dsm_ctx* ctx) {
  delete ctx->covsift;
  ctx->covsift = nullptr;
}

extern "C" void dsm_covariant_sift_default_options(dsm_covariant_sift_options* o) {  // SiftExtractionOptions, src/feature/sift.h:78-100
  o->octave_resolution = 3;
  o->first_octave = -1;
  o->max_num_features = 8192;
  o->upright = 0;
  o->normalization = DSM_SIFT_L1_ROOT;
  o->estimate_affine_shape = 0;
  o->domain_size_pooling = 1;  // the extractor this entry restates is the one the option selects
  o->dsp_num_scales = 10;
  o->peak_threshold = 0.02 / 3;  // 0.02 / octave_resolution
  o->edge_threshold = 10.0;
  o->dsp_min_scale = 1.0 / 6.0;
  o->dsp_max_scale = 3.0;
}

namespace {

// the constants of the two patch stages, once per context: the accumulated sample positions of the resampling loops
// (covdet.c:2367-2397), the aaMask (covdet.c:1545-1557) and the descriptor's sample table (sift.c:1809-1869 at the patch centre)
int cov_upload_consts(dsm_ctx* ctx, CovSiftState& d, hipStream_t st) {
  std::vector<double> hat31(COV_D_SIDE), hat41(COV_OR_SIDE);
  {
    const double stephat = COV_D_EXTENT / COV_D_RES;
    double v = -COV_D_EXTENT;
    for (int i = 0; i < COV_D_SIDE; ++i, v += stephat) hat31[i] = v;
  }
  {
    const double stephat = COV_OR_EXTENT / COV_OR_RES;
    double v = -COV_OR_EXTENT;
    for (int i = 0; i < COV_OR_SIDE; ++i, v += stephat) hat41[i] = v;
  }
  std::vector<float> mask(COV_OR_N);
  {
    const long w = COV_OR_RES;
    const double step = (2.0 * COV_OR_EXTENT) / (2 * w + 1);
    const double sigma = 3;  // VL_COVDET_AA_RELATIVE_INTEGRATION_SIGMA
    for (long j = -w; j <= w; ++j)
      for (long i = -w; i <= w; ++i) {
        const double dx = i * step / sigma, dy = j * step / sigma;
        mask[(i + w) + (2 * w + 1) * (j + w)] = std::exp(-0.5 * (dx * dx + dy * dy));
      }
  }
  // vl_sift_calc_raw_descriptor(x = y = 15, sigma = kSigma = 2, angle0 = 0) on a 31 x 31 patch, magnif = 3, windowSize = 2
  std::vector<CovSample> cells[COV_CELLS];
  {
    double expn[SIFT_EXPN_SZ + 2];  // fast_expn_init, sift.c:713-720
    for (int k = 0; k < SIFT_EXPN_SZ + 1; ++k) expn[k] = std::exp(-(double)k * (25.0 / SIFT_EXPN_SZ));
    expn[SIFT_EXPN_SZ + 1] = 0.0;
    auto fast_expn = [&](double x) {  // sift.c:691-706
      if (x > 25.0) return 0.0;
      x *= SIFT_EXPN_SZ / 25.0;
      const int i = (int)cov_floor(x);
      const double r = x - i;
      const double a = expn[i], b = expn[i + 1];
      return a + r * (b - a);
    };
    auto floor_f = [](float x) {  // vl_floor_f
      const long xi = (long)x;
      if (x >= 0 || (float)xi == x) return xi;
      return xi - 1;
    };
    const double kPatchStep = COV_D_EXTENT / COV_D_RES;
    const double kSigma = COV_D_EXTENT / (3.0 * (4 + 1) / 2) / kPatchStep;  // sift.cc:524-525
    const double x = COV_D_RES, y = COV_D_RES, magnif = 3.0, angle0 = 0;
    const int w = COV_D_SIDE, h = COV_D_SIDE, NBP = 4;
    const int xi = (int)(x + 0.5), yi = (int)(y + 0.5);
    const double st0 = std::sin(angle0), ct0 = std::cos(angle0);
    const double SBP = magnif * kSigma + kVlEpsD;
    const int W = (int)std::floor(std::sqrt(2.0) * SBP * (NBP + 1) / 2.0 + 0.5);
    for (int dyi = std::max(-W, -yi); dyi <= std::min(+W, h - yi - 1); ++dyi)
      for (int dxi = std::max(-W, -xi); dxi <= std::min(+W, w - xi - 1); ++dxi) {
        const float dx = (float)(xi + dxi - x), dy = (float)(yi + dyi - y);
        const float nx = (float)((ct0 * dx + st0 * dy) / SBP);
        const float ny = (float)((-st0 * dx + ct0 * dy) / SBP);
        const float wsigma = 2.0f;  // f->windowSize = NBP / 2 (vl_sift_new)
        const float win = (float)fast_expn((nx * nx + ny * ny) / (2.0 * wsigma * wsigma));
        const int binx = (int)floor_f((float)(nx - 0.5)), biny = (int)floor_f((float)(ny - 0.5));
        const float rbinx = (float)(nx - (binx + 0.5)), rbiny = (float)(ny - (biny + 0.5));
        for (int dbinx = 0; dbinx < 2; ++dbinx)
          for (int dbiny = 0; dbiny < 2; ++dbiny)
            if (binx + dbinx >= -(NBP / 2) && binx + dbinx < (NBP / 2) && biny + dbiny >= -(NBP / 2) && biny + dbiny < (NBP / 2)) {
              CovSample e;
              e.k = (yi + dyi) * w + (xi + dxi);
              e.win = win;
              e.ax = std::fabs(1 - dbinx - rbinx);
              e.ay = std::fabs(1 - dbiny - rbiny);
              cells[(biny + dbiny + NBP / 2) * NBP + (binx + dbinx + NBP / 2)].push_back(e);
            }
      }
  }
  size_t longest = 0;
  for (int c = 0; c < COV_CELLS; ++c) {
    d.cell_counts[c] = (int32_t)cells[c].size();
    longest = std::max(longest, cells[c].size());
  }
  std::vector<CovSample> table(longest * COV_CELLS, CovSample{0, 0.0f, 0.0f, 0.0f});  // [j][cell]: a step of the walk is one row
  for (int c = 0; c < COV_CELLS; ++c)
    for (size_t j = 0; j < cells[c].size(); ++j) table[j * COV_CELLS + c] = cells[c][j];
  d.at_hat31 = 0;
  d.at_hat41 = d.at_hat31 + sizeof(double) * COV_D_SIDE;
  d.at_mask = d.at_hat41 + sizeof(double) * COV_OR_SIDE;
  d.at_counts = d.at_mask + sizeof(float) * COV_OR_N;
  std::vector<uint8_t> blob(d.at_counts + sizeof(d.cell_counts));
  memcpy(blob.data() + d.at_hat31, hat31.data(), sizeof(double) * COV_D_SIDE);
  memcpy(blob.data() + d.at_hat41, hat41.data(), sizeof(double) * COV_OR_SIDE);
  memcpy(blob.data() + d.at_mask, mask.data(), sizeof(float) * COV_OR_N);
  memcpy(blob.data() + d.at_counts, d.cell_counts, sizeof(d.cell_counts));
  HIPCHK(ctx, d.buf[CovSiftState::consts].reserve(blob.size()));
  HIPCHK(ctx, d.buf[CovSiftState::table].reserve(table.size() * sizeof(CovSample)));
  HIPCHK(ctx, hipMemcpyAsync(d.buf[CovSiftState::consts].p, blob.data(), blob.size(), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d.buf[CovSiftState::table].p, table.data(), table.size() * sizeof(CovSample), hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  d.consts_ready = true;
  return DSM_OK;
}

}  // namespace

// both entries: dsm_extract_covariant_sift refuses estimate_affine_shape, dsm_extract_covariant_sift_affine (affine_entry) honours it
static int cov_extract(dsm_ctx* ctx, const dsm_covariant_sift_options* options, const uint8_t* gray_u8, uint32_t width, uint32_t height,
                       uint32_t row_stride, uint32_t capacity, float* keypoints_out, uint8_t* descriptors_out, uint32_t* num_features_out,
                       bool affine_entry) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [&](int code, const char* msg) { return dsm_fail(ctx, code, msg); };
  dsm_covariant_sift_options o;
  if (options)
    o = *options;
  else
    dsm_covariant_sift_default_options(&o);
  if (num_features_out) *num_features_out = 0;
  if (!gray_u8 || !num_features_out || (capacity && !keypoints_out)) return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (width == 0 || height == 0 || row_stride < width) return fail(DSM_ERR_INVALID_ARGUMENT, "an empty image or row_stride below width");
  if (o.estimate_affine_shape && !affine_entry)
    return fail(DSM_ERR_INVALID_ARGUMENT, "estimate_affine_shape is not covered: vl_covdet_extract_affine_shape stays with the reference");
  // SiftExtractionOptions::Check (sift.cc:218-234)
  if (!(o.max_num_features > 0) || !(o.octave_resolution > 0) || !(o.peak_threshold > 0.0) || !(o.edge_threshold > 0.0) ||
      (o.domain_size_pooling && (!(o.dsp_min_scale > 0) || !(o.dsp_max_scale >= o.dsp_min_scale) || !(o.dsp_num_scales > 0))))
    return fail(DSM_ERR_INVALID_ARGUMENT, "options that SiftExtractionOptions::Check rejects");
  if (o.normalization != DSM_SIFT_L1_ROOT && o.normalization != DSM_SIFT_L2) return fail(DSM_ERR_INVALID_ARGUMENT, "an unknown normalization");
  if (o.first_octave < -4 || o.first_octave > 16 || o.octave_resolution > 64 || (o.domain_size_pooling && o.dsp_num_scales > COV_MAX_SCALES))
    return fail(DSM_ERR_OUT_OF_RANGE, "first_octave outside -4 .. 16, octave_resolution or dsp_num_scales above 64");
  if (width > 0x3fffffffu || height > 0x3fffffffu) return fail(DSM_ERR_OUT_OF_RANGE, "an image side of 2^30 or more");

  CovGeom g;
  g.width = (int)width;
  g.height = (int)height;
  g.first = o.first_octave;
  g.R = o.octave_resolution;
  g.smin = -1;
  g.smax = g.R + 1;
  // vl_scalespace_get_default_geometry (scalespace.c:318) computes the base scale for ITS octaveResolution, 3, and
  // vl_covdet_put_image (covdet.c:1712-1718) replaces the resolution and leaves the base scale
  g.base = 1.6 * std::pow(2.0, 1.0 / 3);
  const double nominal = 0.5;
  {
    // covdet.c:1699; what the reference aborts on: no octave at all, or a negative first octave without octave 0 (scalespace.c:396)
    const double side = std::min((double)width - 1, (double)height - 1);
    if (!(side >= 15.0 * std::pow(2.0, (double)std::max(g.first, 0))))
      return fail(DSM_ERR_OUT_OF_RANGE, "the image is too small for this first_octave: the reference aborts (min(width, height) - 1 < 15 * 2^max(first_octave, 0))");
    g.last = (int)cov_floor(std::log2(side / 15.0));
    if (g.last < std::max(g.first, 0)) return fail(DSM_ERR_OUT_OF_RANGE, "the image is too small for this first_octave: the reference aborts");
  }
  const int levels = g.R + 3;
  uint64_t total = 0;
  for (int oc = g.first; oc <= g.last; ++oc) {
    g.oct.push_back(total);
    total += (uint64_t)g.ow(oc) * g.oh(oc) * levels;
  }
  const uint64_t w0 = g.ow(g.first), h0 = g.oh(g.first), nel0 = std::max<uint64_t>(w0 * h0, (uint64_t)width * height);
  if (w0 > 0x3fffffffu || h0 > 65535 || nel0 * (uint64_t)levels >= 0x80000000ull)
    return fail(DSM_ERR_OUT_OF_RANGE, "the first octave has 2^31 or more samples or more than 65535 rows");
  const uint64_t chunks0 = (nel0 * g.R + SIFT_CHUNK - 1) / SIFT_CHUNK;
  const uint64_t scratch = (uint64_t)row_stride * height + 4 * ((uint64_t)width * height + total + nel0 + nel0 * (g.R + 2)) + nel0 * g.R + chunks0 * 8;
  if (ctx->memory_budget && scratch > ctx->memory_budget) return fail(DSM_ERR_OUT_OF_RANGE, "the scale space's scratch exceeds the memory budget");

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  if (!ctx->covsift) ctx->covsift = new CovSiftState();
  CovSiftState& d = *ctx->covsift;
  typedef CovSiftState B;
  d.valid = false;
  d.have_raw = false;
  uint32_t aff_rounds = 0, aff_exits[4] = {0, 0, 0, 0}, aff_active[DSM_AFFINE_SHAPE_MAX_ROUNDS] = {0};
  if (affine_entry) d.affine_valid = false;
  if (!d.consts_ready) {
    const int rc = cov_upload_consts(ctx, d, st);
    if (rc != DSM_OK) return rc;
  }
  for (DevEvent& e : d.ev)
    if (!e.e) HIPCHK(ctx, hipEventCreate(&e.e));
  for (double& v : d.stage_ms) v = 0.0;
  auto mark = [&](int i) { return hipEventRecord(d.ev[i], st); };
  auto took = [&](int stage, int a) {  // events a, a + 1 have completed
    float ms = 0;
    const hipError_t e = hipEventElapsedTime(&ms, d.ev[a], d.ev[a + 1]);
    d.stage_ms[stage] += ms;
    return e;
  };
  HIPCHK(ctx, d.buf[B::img].reserve((size_t)row_stride * height));
  HIPCHK(ctx, d.buf[B::fimg].reserve((size_t)width * height * 4));
  HIPCHK(ctx, d.buf[B::gss].reserve(total * 4));
  HIPCHK(ctx, d.buf[B::tmp].reserve(nel0 * 4));
  HIPCHK(ctx, d.buf[B::dog].reserve(nel0 * 4 * (g.R + 2)));
  HIPCHK(ctx, d.buf[B::flags].reserve(nel0 * g.R));
  HIPCHK(ctx, d.buf[B::counts].reserve(chunks0 * 4));
  HIPCHK(ctx, d.buf[B::offs].reserve(chunks0 * 4));
  HIPCHK(ctx, hipMemcpyAsync(d.buf[B::img].p, gray_u8, (size_t)row_stride * height, hipMemcpyHostToDevice, st));
  float* gss = d.buf[B::gss].as<float>();
  float* tmp = d.buf[B::tmp].as<float>();
  float* fimg = d.buf[B::fimg].as<float>();
  const double* hat31 = reinterpret_cast<const double*>(static_cast<const uint8_t*>(d.buf[B::consts].p) + d.at_hat31);
  const double* hat41 = reinterpret_cast<const double*>(static_cast<const uint8_t*>(d.buf[B::consts].p) + d.at_hat41);
  const float* mask = reinterpret_cast<const float*>(static_cast<const uint8_t*>(d.buf[B::consts].p) + d.at_mask);
  const int32_t* cell_counts = reinterpret_cast<const int32_t*>(static_cast<const uint8_t*>(d.buf[B::consts].p) + d.at_counts);

  // ---- vl_scalespace_put_image (scalespace.c:811-821).  Pass 0 collects the taps of every smoothing in call order, pass 1
  // launches; the sigmas depend on the geometry alone.
  auto sigma_of = [&](int oc, int s) { return g.base * std::pow(2.0, oc + (double)s / g.R); };  // vl_scalespace_get_level_sigma
  std::vector<float> all_taps;
  std::vector<size_t> tap_at;
  std::vector<int> tap_w;
  size_t next_smooth = 0;
  for (int pass = 0; pass < 2; ++pass) {
    auto smooth = [&](uint64_t dst, uint64_t src, int w, int h, double sigma) {  // vl_imsmooth_f with sigmax = sigmay = sigma
      if (pass == 0) {
        tap_at.push_back(all_taps.size());
        tap_w.push_back(cov_taps(sigma, &all_taps));
        return;
      }
      const float* taps = d.buf[B::taps].as<float>() + tap_at[next_smooth];
      const int W = tap_w[next_smooth++];
      hipLaunchKernelGGL(k_sift_conv_cols, dim3((w + SIFT_TILE - 1) / SIFT_TILE, (h + SIFT_TILE - 1) / SIFT_TILE), dim3(SIFT_BLOCK),
                         (size_t)((SIFT_TILE + 2 * W) * SIFT_TILE + 2 * W + 1) * 4, st, tmp, (const float*)(gss + src), w, h, taps, W);
      hipLaunchKernelGGL(k_sift_conv_rows, dim3((w + SIFT_BLOCK - 1) / SIFT_BLOCK, h), dim3(SIFT_BLOCK), (size_t)(SIFT_BLOCK + 4 * W + 1) * 4, st,
                         gss + dst, (const float*)tmp, w, h, taps, W);
    };
    auto fill_octave = [&](int oc) {  // _vl_scalespace_fill_octave, :669-686
      const double step = std::pow(2.0, (double)oc);
      for (int s = g.smin + 1; s <= g.smax; ++s) {
        const double sigma = sigma_of(oc, s), previousSigma = sigma_of(oc, s - 1);
        const double deltaSigma = sqrtf(sigma * sigma - previousSigma * previousSigma);
        smooth(g.level(oc, s), g.level(oc, s - 1), g.ow(oc), g.oh(oc), deltaSigma / step);
      }
    };
    if (pass == 1) {
      for (int w : tap_w)
        if (w > 256) return fail(DSM_ERR_OUT_OF_RANGE, "a smoothing half-width above 256 samples");
      HIPCHK(ctx, d.buf[B::taps].reserve(all_taps.size() * 4));
      HIPCHK(ctx, hipMemcpyAsync(d.buf[B::taps].p, all_taps.data(), all_taps.size() * 4, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, mark(0));
      hipLaunchKernelGGL(k_sift_load, dim3(dsm_grid((uint64_t)width * height, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, fimg, d.buf[B::img].as<uint8_t>(), width, height,
                         row_stride);
      // _vl_scalespace_start_octave_from_image, :699-745: down to octave max(0, first), then up from octave 0
      const int top = std::max(0, g.first);
      hipLaunchKernelGGL(k_sift_downsample, dim3(dsm_grid((uint64_t)g.ow(top) * g.oh(top), SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, gss + g.level(top, g.smin),
                         (const float*)fimg, width, 1u << top, (uint32_t)g.ow(top), (uint32_t)g.oh(top));
      for (int op = -1; op >= g.first; --op)
        hipLaunchKernelGGL(k_cov_upsample, dim3(dsm_grid((uint64_t)g.ow(op + 1) * g.oh(op + 1), SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, gss + g.level(op, g.smin),
                           (const float*)(gss + g.level(op + 1, g.smin)), (uint32_t)g.ow(op + 1), (uint32_t)g.oh(op + 1));
    }
    {
      const double sigma = sigma_of(g.first, g.smin), imageSigma = nominal;
      if (sigma > imageSigma) {
        const double deltaSigma = std::sqrt(sigma * sigma - imageSigma * imageSigma);
        smooth(g.level(g.first, g.smin), g.level(g.first, g.smin), g.ow(g.first), g.oh(g.first), deltaSigma / std::pow(2.0, (double)g.first));
      }
    }
    fill_octave(g.first);
    for (int oc = g.first + 1; oc <= g.last; ++oc) {  // _vl_scalespace_start_octave_from_previous_octave, :755-801
      const int prevLevelIndex = std::min(g.smin + g.R, g.smax);
      if (pass == 1)
        hipLaunchKernelGGL(k_sift_downsample, dim3(dsm_grid((uint64_t)g.ow(oc) * g.oh(oc), SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, gss + g.level(oc, g.smin),
                           (const float*)(gss + g.level(oc - 1, prevLevelIndex)), (uint32_t)g.ow(oc - 1), 2u, (uint32_t)g.ow(oc), (uint32_t)g.oh(oc));
      const double sigma = sigma_of(oc, g.smin), prevSigma = sigma_of(oc - 1, prevLevelIndex);
      if (sigma > prevSigma) {
        const double deltaSigma = std::sqrt(sigma * sigma - prevSigma * prevSigma);
        smooth(g.level(oc, g.smin), g.level(oc, g.smin), g.ow(oc), g.oh(oc), deltaSigma / std::pow(2.0, (double)oc));
      }
      fill_octave(oc);
    }
  }
  HIPCHK(ctx, mark(1));
  HIPCHK(ctx, hipGetLastError());

  // ---- vl_covdet_detect (covdet.c:1991-2089): the octaves from the last to the first, COLMAP's early end at :2086
  std::vector<CovFeature> features;
  std::vector<uint32_t> counts;
  std::vector<CovCand> refined;
  const int depth = g.R + 2;  // the levels of the DoG scale space: s = -1 .. R
  for (int oc = g.last; oc >= g.first; --oc) {
    const uint32_t w = (uint32_t)g.ow(oc), h = (uint32_t)g.oh(oc), nel = w * h;
    const double step = std::pow(2.0, (double)oc);
    const uint32_t ndog = nel * (uint32_t)depth, nflag = nel * (uint32_t)g.R, chunks = (nflag + SIFT_CHUNK - 1) / SIFT_CHUNK;
    float* dog = d.buf[B::dog].as<float>();
    HIPCHK(ctx, mark(2));
    hipLaunchKernelGGL(k_cov_dog, dim3(dsm_grid(ndog, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, dog, (const float*)(gss + g.level(oc, g.smin)), nel, ndog);
    hipLaunchKernelGGL(k_sift_detect, dim3(dsm_grid(nflag, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[B::flags].as<uint8_t>(), (const float*)dog, (int)w, (int)h, nflag,
                       0.8 * o.peak_threshold);
    auto compact = [&](const uint32_t* offs, uint32_t* out) {
      hipLaunchKernelGGL(k_sift_compact, dim3(dsm_grid(chunks, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, (const uint8_t*)d.buf[B::flags].as<uint8_t>(), nflag, chunks, offs, out);
    };
    compact(nullptr, d.buf[B::counts].as<uint32_t>());
    HIPCHK(ctx, mark(3));
    HIPCHK(ctx, hipGetLastError());
    counts.resize(chunks);
    HIPCHK(ctx, hipMemcpyAsync(counts.data(), d.buf[B::counts].p, (size_t)chunks * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, took(1, 2));
    uint32_t ncand = 0;
    for (uint32_t c = 0; c < chunks; ++c) {  // exclusive scan in place
      const uint32_t k = counts[c];
      counts[c] = ncand;
      ncand += k;
    }
    if (ncand) {
      if (ctx->memory_budget && scratch + (uint64_t)ncand * (4 + sizeof(CovCand)) > ctx->memory_budget)
        return fail(DSM_ERR_OUT_OF_RANGE, "the candidates' scratch exceeds the memory budget");
      HIPCHK(ctx, mark(2));
      HIPCHK(ctx, hipMemcpyAsync(d.buf[B::offs].p, counts.data(), (size_t)chunks * 4, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, d.buf[B::cand].reserve((size_t)ncand * 4));
      HIPCHK(ctx, d.buf[B::refined].reserve((size_t)ncand * sizeof(CovCand)));
      compact(d.buf[B::offs].as<uint32_t>(), d.buf[B::cand].as<uint32_t>());
      hipLaunchKernelGGL(k_cov_refine, dim3(dsm_grid(ncand, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[B::refined].as<CovCand>(), (const uint32_t*)d.buf[B::cand].as<uint32_t>(),
                         ncand, (const float*)dog, (int)w, (int)h, depth);
      HIPCHK(ctx, mark(3));
      HIPCHK(ctx, hipGetLastError());
      refined.resize(ncand);
      HIPCHK(ctx, hipMemcpyAsync(refined.data(), d.buf[B::refined].p, (size_t)ncand * sizeof(CovCand), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, took(1, 2));
      for (const CovCand& c : refined) {  // covdet.c:2024-2041
        bool ok = c.ok != 0;
        ok &= std::fabs(c.peak) > o.peak_threshold;
        ok &= c.edge < o.edge_threshold;
        if (!ok) continue;
        // the exponent is float arithmetic: refined.z is a float, and the integers beside it convert to float
        const double sigma = g.base * std::pow(2.0, (float)oc + (c.z + (float)g.smin) / (float)g.R);
        CovFeature f;
        f.x = c.x * step;
        f.y = c.y * step;
        f.a11 = sigma;
        f.a12 = 0.0;
        f.a21 = 0.0;
        f.a22 = sigma;
        f.o = oc;
        f.s = (int32_t)std::round(c.z);
        f.peak = c.peak;
        f.edge = c.edge;
        f.orient = 0;
        features.push_back(f);
      }
    }
    if (features.size() >= (size_t)o.max_num_features) break;
  }
  {  // the non-extrema suppression, covdet.c:2104-2139 (tolerance 0.5, covdet.c:1536): a feature zeroed earlier no longer suppresses.
    // Within one i the set of zeroed j does not depend on the order of j, and a j outside the box |dx|, |dy| < tol sigma fails the
    // test: so the inner loop visits the cells of a grid that the box touches instead of all features -- the same tests on the
    // same values, the same result (47 785 detections at 3200 x 2400 are 2.3 x 10^9 pair tests otherwise).
    const double tol = 0.5, cell = 8.0;
    const long n = (long)features.size();
    const long gx = (long)(width / cell) + 2, gy = (long)(height / cell) + 2;
    auto cell_of = [&](double v, long hi) {
      const long c = (long)std::floor(v / cell);
      return c < 0 ? 0l : (c > hi - 1 ? hi - 1 : c);
    };
    std::vector<uint32_t> first((size_t)(gx * gy) + 1, 0), members((size_t)n);
    for (long i = 0; i < n; ++i) first[(size_t)(cell_of(features[i].y, gy) * gx + cell_of(features[i].x, gx)) + 1] += 1;
    for (size_t c = 0; c < (size_t)(gx * gy); ++c) first[c + 1] += first[c];
    {
      std::vector<uint32_t> fill(first.begin(), first.end() - 1);
      for (long i = 0; i < n; ++i) members[fill[(size_t)(cell_of(features[i].y, gy) * gx + cell_of(features[i].x, gx))]++] = (uint32_t)i;
    }
    for (long i = 0; i < n; ++i) {
      const double x = features[i].x, y = features[i].y, sigma = features[i].a11, score = features[i].peak;
      if (score == 0) continue;
      const long cx0 = cell_of(x - tol * sigma, gx), cx1 = cell_of(x + tol * sigma, gx);
      const long cy0 = cell_of(y - tol * sigma, gy), cy1 = cell_of(y + tol * sigma, gy);
      for (long cy = cy0; cy <= cy1; ++cy)
        for (long cx = cx0; cx <= cx1; ++cx)
          for (uint32_t m = first[(size_t)(cy * gx + cx)]; m < first[(size_t)(cy * gx + cx) + 1]; ++m) {
            const long j = members[m];
            const double dx_ = features[j].x - x, dy_ = features[j].y - y, sigma_ = features[j].a11, score_ = features[j].peak;
            if (score_ == 0) continue;
            if (sigma < (1 + tol) * sigma_ && sigma_ < (1 + tol) * sigma && std::fabs(dx_) < tol * sigma && std::fabs(dy_) < tol * sigma &&
                std::fabs(score) > std::fabs(score_))
              features[j].peak = 0;
          }
    }
    size_t j = 0;
    for (size_t i = 0; i < features.size(); ++i)
      if (features[i].peak != 0) features[j++] = features[i];
    features.resize(j);
  }

  // ---- sift.cc:467-473: vl_covdet_extract_affine_shape (covdet.c:2462-2668) in the place of the orientations.  The loop of
  // every feature advances in rounds: the host runs a pass's head (vl_svd2, the anisotropy test, the rescaling, the iteration
  // limit) and plans the patch, one launch computes the three sums of every active feature, the host reads them and runs the
  // pass's tail (the zero test, vl_svd2, the convergence test, the update of A).  At most 14 rounds: the 15th head leaves.
  if (o.estimate_affine_shape && !o.upright && !features.empty()) {
    enum { DIVERGED = 0, MAX_ITER = 1, ZERO_MOMENT = 2, CONVERGED = 3 };
    struct Shape {
      double A[4], T[2], D0, D3, referenceScale;
      int iter;
      CovFeature adapted;
    };
    const size_t nf = features.size();
    if (ctx->memory_budget && scratch + nf * (sizeof(CovPatch) + 24) > ctx->memory_budget)
      return fail(DSM_ERR_OUT_OF_RANGE, "the shape adaptation's scratch exceeds the memory budget");
    std::vector<Shape> shapes(nf);
    std::vector<uint32_t> active, next;
    auto head = [&](uint32_t i) {  // covdet.c:2495-2528; true: the pass goes on to the patch
      Shape& h = shapes[i];
      double U[4], V[4], D[4], factor;
      cov_svd2(D, U, V, h.A);
      const double r0 = D[0] / D[3], r1 = D[3] / D[0];
      const double anisotropy = r0 > r1 ? r0 : r1;  // VL_MAX
      if (anisotropy > 5.0) {  // VL_COVDET_AA_MAX_ANISOTROPY
        aff_exits[DIVERGED] += 1;
        return false;
      }
      if (h.iter == 0) {
        h.referenceScale = D[0] < D[3] ? D[0] : D[3];  // VL_MIN
        factor = 1.0;
      } else {
        factor = h.referenceScale / (D[0] < D[3] ? D[0] : D[3]);
      }
      D[0] *= factor;
      D[3] *= factor;
      h.A[0] = U[0] * D[0];
      h.A[1] = U[1] * D[0];
      h.A[2] = U[2] * D[3];
      h.A[3] = U[3] * D[3];
      h.adapted.a11 = h.A[0];
      h.adapted.a21 = h.A[1];
      h.adapted.a12 = h.A[2];
      h.adapted.a22 = h.A[3];
      h.D0 = D[0];
      h.D3 = D[3];
      if (++h.iter >= 15) {  // VL_COVDET_AA_MAX_NUM_ITERATIONS
        aff_exits[MAX_ITER] += 1;
        return false;
      }
      return true;
    };
    for (size_t i = 0; i < nf; ++i) {
      const CovFeature& f = features[i];
      Shape& h = shapes[i];
      h.A[0] = f.a11, h.A[1] = f.a21, h.A[2] = f.a12, h.A[3] = f.a22;
      h.T[0] = f.x, h.T[1] = f.y;
      h.D0 = h.D3 = h.referenceScale = 0;
      h.iter = 0;
      h.adapted = f;
      if (head((uint32_t)i)) active.push_back((uint32_t)i);
    }
    std::vector<CovPatch> jobs;
    std::vector<double> sums;
    HIPCHK(ctx, d.buf[B::ojobs].reserve(active.size() * sizeof(CovPatch)));
    HIPCHK(ctx, d.buf[B::oout].reserve(active.size() * 24));
    while (!active.empty()) {
      if (aff_rounds >= DSM_AFFINE_SHAPE_MAX_ROUNDS) return fail(DSM_ERR_OUT_OF_RANGE, "the shape adaptation ran past its 14 rounds");
      const size_t na = active.size();
      aff_active[aff_rounds++] = (uint32_t)na;
      jobs.resize(na);
      sums.resize(3 * na);
      for (size_t j = 0; j < na; ++j) {
        const Shape& h = shapes[active[j]];
        cov_plan_patch(g, &jobs[j], nullptr, nullptr, COV_OR_EXTENT, 1.0 /* VL_COVDET_AA_RELATIVE_DERIVATIVE_SIGMA */, h.A, h.T, h.D0, h.D3);
      }
      HIPCHK(ctx, hipMemcpyAsync(d.buf[B::ojobs].p, jobs.data(), na * sizeof(CovPatch), hipMemcpyHostToDevice, st));
      HIPCHK(ctx, mark(4));
      hipLaunchKernelGGL(k_cov_affine_moments, dim3((uint32_t)na), dim3(COV_WAVE), 0, st, (const CovPatch*)d.buf[B::ojobs].as<CovPatch>(), (const float*)gss, hat41,
                         mask, d.buf[B::oout].as<double>());
      HIPCHK(ctx, mark(5));
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(sums.data(), d.buf[B::oout].p, na * 24, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, took(2, 4));
      next.clear();
      for (size_t j = 0; j < na; ++j) {  // covdet.c:2559-2598
        const uint32_t i = active[j];
        Shape& h = shapes[i];
        const double lxx = sums[3 * j], lyy = sums[3 * j + 1], lxy = sums[3 * j + 2];
        const double M[4] = {lxx, lxy, lxy, lyy};
        if (lxx == 0 || lyy == 0) {
          h.adapted = features[i];
          aff_exits[ZERO_MOMENT] += 1;
          continue;
        }
        double Q[4], P[4], P_[4];
        cov_svd2(Q, P, P_, M);
        if (Q[3] / Q[0] < 1.001 && Q[0] / Q[3] < 1.001) {  // VL_COVDET_AA_CONVERGENCE_THRESHOLD
          aff_exits[CONVERGED] += 1;
          continue;
        }
        double Ap[4];
        const double q0 = std::sqrt(Q[0]), q1 = std::sqrt(Q[3]);
        Ap[0] = (h.A[0] * P[0] + h.A[2] * P[1]) / q0;
        Ap[1] = (h.A[1] * P[0] + h.A[3] * P[1]) / q0;
        Ap[2] = (h.A[0] * P[2] + h.A[2] * P[3]) / q1;
        Ap[3] = (h.A[1] * P[2] + h.A[3] * P[3]) / q1;
        memcpy(h.A, Ap, sizeof(Ap));
        if (head(i)) next.push_back(i);
      }
      active.swap(next);
    }
    for (size_t i = 0; i < nf; ++i) {  // make upright, covdet.c:2610-2639 (transposed is false): reads the adapted frame's floats
      const CovFeature& ad = shapes[i].adapted;
      const double A[4] = {ad.a11, ad.a21, ad.a12, ad.a22};
      const double ref[2] = {0, 1};
      double ref_[2];
      cov_solve2(ref_, A, ref);
      const double angle = std::atan2(ref[1], ref[0]);
      const double angle_ = std::atan2(ref_[1], ref_[0]);
      const double dangle = angle_ - angle;
      // one sincos call, as the reference's compiler emits for cos and sin of one argument (gcc -O2): glibc's sincos and its sin
      // differ in the last bit of the sine for some arguments, and a12 is the residual of a cancellation that shows it
      double r1, r2;
      ::sincos(dangle, &r2, &r1);
      CovFeature& f = features[i];
      f = ad;
      f.a11 = +A[0] * r1 + A[2] * r2;
      f.a21 = +A[1] * r1 + A[3] * r2;
      f.a12 = -A[0] * r2 + A[2] * r1;
      f.a22 = -A[1] * r2 + A[3] * r1;
    }
  }

  // ---- vl_covdet_extract_orientations (covdet.c:2857-2892) unless upright (sift.cc:467-473)
  if (!o.estimate_affine_shape && !o.upright && !features.empty()) {
    const size_t nf = features.size();
    std::vector<CovOrientJob> jobs(nf);
    std::vector<double> theta0(nf);
    std::vector<float> taps;
    for (size_t i = 0; i < nf; ++i) {  // covdet.c:2716-2773
      const CovFeature& f = features[i];
      double A[4] = {f.a11, f.a21, f.a12, f.a22};
      const double T[2] = {f.x, f.y};
      double U[4], V[4], D[4], sigma1, sigma2;
      const double sigmaD = 1.0;
      cov_svd2(D, U, V, A);
      A[0] = U[0] * D[0];
      A[1] = U[1] * D[0];
      A[2] = U[2] * D[3];
      A[3] = U[3] * D[3];
      theta0[i] = std::atan2(V[1], V[0]);
      cov_plan_patch(g, &jobs[i].p, &sigma1, &sigma2, COV_OR_EXTENT, sigmaD, A, T, D[0], D[3]);
      const double deltaSigma1 = std::sqrt(std::max(sigmaD * sigmaD - sigma1 * sigma1, 0.0));
      const double deltaSigma2 = std::sqrt(std::max(sigmaD * sigmaD - sigma2 * sigma2, 0.0));
      const double stephat = COV_OR_EXTENT / COV_OR_RES;
      taps.clear();
      jobs[i].wx = cov_taps(deltaSigma1 / stephat, &taps);
      if (2 * jobs[i].wx + 1 > COV_OR_TAPS) return fail(DSM_ERR_OUT_OF_RANGE, "an orientation patch's smoothing is wider than 15 taps");
      memset(jobs[i].tx, 0, sizeof(jobs[i].tx));
      memcpy(jobs[i].tx, taps.data(), taps.size() * 4);
      taps.clear();
      jobs[i].wy = cov_taps(deltaSigma2 / stephat, &taps);
      if (2 * jobs[i].wy + 1 > COV_OR_TAPS) return fail(DSM_ERR_OUT_OF_RANGE, "an orientation patch's smoothing is wider than 15 taps");
      memset(jobs[i].ty, 0, sizeof(jobs[i].ty));
      memcpy(jobs[i].ty, taps.data(), taps.size() * 4);
    }
    HIPCHK(ctx, d.buf[B::ojobs].reserve(nf * sizeof(CovOrientJob)));
    HIPCHK(ctx, d.buf[B::oout].reserve(nf * sizeof(CovOrientOut)));
    HIPCHK(ctx, hipMemcpyAsync(d.buf[B::ojobs].p, jobs.data(), nf * sizeof(CovOrientJob), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, mark(4));
    hipLaunchKernelGGL(k_cov_orient, dim3((uint32_t)nf), dim3(COV_WAVE), 0, st, (const CovOrientJob*)d.buf[B::ojobs].as<CovOrientJob>(), (const float*)gss, hat41, mask,
                       d.buf[B::oout].as<CovOrientOut>());
    HIPCHK(ctx, mark(5));
    HIPCHK(ctx, hipGetLastError());
    std::vector<CovOrientOut> outs(nf);
    HIPCHK(ctx, hipMemcpyAsync(outs.data(), d.buf[B::oout].p, nf * sizeof(CovOrientOut), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, took(2, 4));
    const double binExtent = 2 * kVlPi / COV_OR_BINS;
    for (size_t i = 0; i < nf; ++i) {
      const CovFeature feature = features[i];
      struct Orientation {
        double angle, score;
      } ors[COV_OR_MAX];
      const int n = std::min(std::max(outs[i].n, 0), (int)COV_OR_MAX);
      for (int k = 0; k < n; ++k) {
        ors[k].angle = binExtent * outs[i].pos[k] + theta0[i];
        ors[k].score = outs[i].score[k];
      }
      // qsort by descending score (covdet.c:2841-2844): glibc's merge sort keeps equal scores in index order
      std::stable_sort(ors, ors + n, [](const Orientation& a, const Orientation& b) { return a.score > b.score; });
      for (int j = 0; j < n; ++j) {
        const double A[4] = {feature.a11, feature.a21, feature.a12, feature.a22};
        const double r1 = std::cos(ors[j].angle), r2 = std::sin(ors[j].angle);
        if (j > 0) features.push_back(feature);
        CovFeature& oriented = j == 0 ? features[i] : features.back();
        oriented.orient = ors[j].score;
        oriented.a11 = +A[0] * r1 + A[2] * r2;
        oriented.a21 = +A[1] * r1 + A[3] * r2;
        oriented.a12 = -A[0] * r2 + A[2] * r1;
        oriented.a22 = -A[1] * r2 + A[3] * r1;
      }
    }
  }

  // ---- COLMAP's half: the sort (sift.cc:479-487; the same std::sort on the same sequence) and the cut (:489-513)
  std::sort(features.begin(), features.end(), [](const CovFeature& feature1, const CovFeature& feature2) {
    if (feature1.o == feature2.o) {
      return feature1.s > feature2.s;
    } else {
      return feature1.o > feature2.o;
    }
  });
  size_t kept = 0;
  {
    const int kMaxOctaveResolution = 1000;
    int prev_octave_scale_idx = std::numeric_limits<int>::max();
    for (size_t i = 0; i < features.size(); ++i) {
      ++kept;
      const int octave_scale_idx = features[i].o * kMaxOctaveResolution + features[i].s;
      if (octave_scale_idx != prev_octave_scale_idx && kept >= (size_t)o.max_num_features) break;
      prev_octave_scale_idx = octave_scale_idx;
    }
  }
  *num_features_out = (uint32_t)kept;
  if (kept > capacity) return fail(DSM_ERR_OUT_OF_RANGE, "capacity below the number of features found (see num_features_out)");

  // ---- the descriptors (sift.cc:515-594)
  float dsp_min_scale = 1;
  float dsp_scale_step = 0;
  int dsp_num_scales = 1;
  if (o.domain_size_pooling) {
    dsp_min_scale = o.dsp_min_scale;
    dsp_scale_step = (o.dsp_max_scale - o.dsp_min_scale) / o.dsp_num_scales;
    dsp_num_scales = o.dsp_num_scales;
  }
  std::vector<uint8_t> desc_host;
  if (descriptors_out && kept) {
    const size_t nitems = kept * (size_t)dsp_num_scales;
    if (ctx->memory_budget && scratch + nitems * (sizeof(CovPatch) + 512) + kept * 128 > ctx->memory_budget)
      return fail(DSM_ERR_OUT_OF_RANGE, "the descriptors' scratch exceeds the memory budget");
    std::vector<CovPatch> items(nitems);
    for (size_t i = 0; i < kept; ++i)
      for (int s = 0; s < dsp_num_scales; ++s) {
        const double dsp_scale = dsp_min_scale + s * dsp_scale_step;
        CovFeature f = features[i];
        f.a11 *= dsp_scale;
        f.a12 *= dsp_scale;
        f.a21 *= dsp_scale;
        f.a22 *= dsp_scale;
        double A[4] = {f.a11, f.a21, f.a12, f.a22};  // vl_covdet_extract_patch_for_frame, covdet.c:2438-2445
        const double T[2] = {f.x, f.y};
        double D[4], U[4], V[4];
        cov_svd2(D, U, V, A);
        cov_plan_patch(g, &items[i * dsp_num_scales + s], nullptr, nullptr, COV_D_EXTENT, 1.0 /* kPatchRelativeSmoothing */, A, T, D[0], D[3]);
      }
    HIPCHK(ctx, d.buf[B::items].reserve(nitems * sizeof(CovPatch)));
    HIPCHK(ctx, d.buf[B::raw].reserve(nitems * 512));
    HIPCHK(ctx, d.buf[B::desc8].reserve(kept * 128));
    HIPCHK(ctx, hipMemcpyAsync(d.buf[B::items].p, items.data(), nitems * sizeof(CovPatch), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, mark(4));
    hipLaunchKernelGGL(k_cov_describe, dim3((uint32_t)nitems), dim3(COV_WAVE), 0, st, (const CovPatch*)d.buf[B::items].as<CovPatch>(), (const float*)gss, hat31,
                       (const CovSample*)d.buf[B::table].as<CovSample>(), cell_counts, d.buf[B::raw].as<float>());
    HIPCHK(ctx, mark(5));
    hipLaunchKernelGGL(k_cov_pool, dim3((uint32_t)kept), dim3(128), 0, st, (const float*)d.buf[B::raw].as<float>(), dsp_num_scales, (int)(o.domain_size_pooling != 0),
                       (int)(o.normalization == DSM_SIFT_L2), d.buf[B::desc8].as<uint8_t>());
    HIPCHK(ctx, mark(6));
    HIPCHK(ctx, hipGetLastError());
    desc_host.resize(kept * 128);
    HIPCHK(ctx, hipMemcpyAsync(desc_host.data(), d.buf[B::desc8].p, kept * 128, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, took(3, 4));
    HIPCHK(ctx, took(4, 5));
    d.have_raw = true;
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, took(0, 0));

  d.n = (uint32_t)kept;
  d.scales = (uint32_t)dsp_num_scales;
  d.os.resize(kept * 2);
  d.scores.resize(kept * 3);
  for (size_t i = 0; i < kept; ++i) {
    const CovFeature& f = features[i];
    float* kp = keypoints_out + 6 * i;  // sift.cc:494-501
    kp[0] = f.x + 0.5;
    kp[1] = f.y + 0.5;
    kp[2] = f.a11;
    kp[3] = f.a12;
    kp[4] = f.a21;
    kp[5] = f.a22;
    d.os[2 * i] = f.o;
    d.os[2 * i + 1] = f.s;
    d.scores[3 * i] = f.peak;
    d.scores[3 * i + 1] = f.edge;
    d.scores[3 * i + 2] = f.orient;
  }
  if (kept && descriptors_out) memcpy(descriptors_out, desc_host.data(), kept * 128);
  d.valid = true;
  if (affine_entry) {
    d.affine_rounds = aff_rounds;
    memcpy(d.affine_exits, aff_exits, sizeof(aff_exits));
    memcpy(d.affine_active, aff_active, sizeof(aff_active));
    d.affine_valid = true;
  }
  return DSM_OK;
}

extern "C" int dsm_extract_covariant_sift(dsm_ctx* ctx, const dsm_covariant_sift_options* options, const uint8_t* gray_u8, uint32_t width,
                                          uint32_t height, uint32_t row_stride, uint32_t capacity, float* keypoints_out,
                                          uint8_t* descriptors_out, uint32_t* num_features_out) {
  return cov_extract(ctx, options, gray_u8, width, height, row_stride, capacity, keypoints_out, descriptors_out, num_features_out, false);
}

extern "C" int dsm_extract_covariant_sift_affine(dsm_ctx* ctx, const dsm_covariant_sift_options* options, const uint8_t* gray_u8,
                                                 uint32_t width, uint32_t height, uint32_t row_stride, uint32_t capacity,
                                                 float* keypoints_out, uint8_t* descriptors_out, uint32_t* num_features_out) {
  return cov_extract(ctx, options, gray_u8, width, height, row_stride, capacity, keypoints_out, descriptors_out, num_features_out, true);
}

extern "C" int dsm_get_affine_shape_stats(dsm_ctx* ctx, uint32_t* rounds, uint32_t exits[4], uint32_t active[DSM_AFFINE_SHAPE_MAX_ROUNDS]) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->covsift || !ctx->covsift->affine_valid)
    return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_affine_shape_stats: no successful dsm_extract_covariant_sift_affine call yet");
  const CovSiftState& d = *ctx->covsift;
  if (rounds) *rounds = d.affine_rounds;
  if (exits) memcpy(exits, d.affine_exits, sizeof(d.affine_exits));
  if (active) memcpy(active, d.affine_active, sizeof(d.affine_active));
  return DSM_OK;
}

extern "C" int dsm_get_covariant_sift_raw(dsm_ctx* ctx, uint32_t capacity, int32_t* octave_scale, float* scores, float* raw_descriptors,
                                          uint32_t* n_out) {
  if (!ctx || !n_out) return DSM_ERR_INVALID_ARGUMENT;
  *n_out = 0;
  if (!ctx->covsift || !ctx->covsift->valid)
    return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_covariant_sift_raw: no successful dsm_extract_covariant_sift or dsm_extract_covariant_sift_affine call yet");
  CovSiftState& d = *ctx->covsift;
  *n_out = d.n;
  if (raw_descriptors && !d.have_raw && d.n)
    return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_covariant_sift_raw: the last call computed no descriptors (descriptors_out was NULL)");
  if (d.n > capacity) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "capacity below the number of features (see n_out)");
  if (octave_scale && d.n) memcpy(octave_scale, d.os.data(), d.os.size() * 4);
  if (scores && d.n) memcpy(scores, d.scores.data(), d.scores.size() * 4);
  if (raw_descriptors && d.n) {
    hipError_t he = hipSetDevice(ctx->device);
    if (he == hipSuccess) he = hipMemcpy(raw_descriptors, d.buf[CovSiftState::raw].p, (size_t)d.n * d.scales * 512, hipMemcpyDeviceToHost);
    HIPCHK(ctx, he);
  }
  return DSM_OK;
}

extern "C" int dsm_get_covariant_sift_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->covsift) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_covariant_sift_time: no dsm_extract_covariant_sift call yet");
  memcpy(stage_ms, ctx->covsift->stage_ms, sizeof(ctx->covsift->stage_ms));
  return DSM_OK;
}
