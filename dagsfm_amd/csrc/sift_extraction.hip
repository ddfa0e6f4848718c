// sift_extraction.hip -- ExtractSiftFeaturesCPU (src/feature/sift.cc:252-426) on the device: VLFeat's vl_sift
// (lib/VLFeat/sift.c) restated operation for operation in its own evaluation order, float where the source is float and double
// where it is double, plus COLMAP's loop around it.
//
// (the image-sized kernels below live in sift_image_ops.h, shared with covariant_sift.hip)
//   k_sift_load / k_sift_upsample_rows / k_sift_downsample   the octave's base (sift.c:738-758, 835-851, 1017-1037, 1113)
//   k_sift_conv_cols / k_sift_conv_rows   the two passes of _vl_sift_smooth (sift.c:773-816): vl_imconvcol_vf with
//                     VL_PAD_BY_CONTINUITY (imopv.c:119-212), a pixel per lane, tile plus halo in LDS, the taps in the source's order
//   k_sift_dog        the differences of adjacent levels (:1176-1185)
//   k_sift_detect     the 26-neighbour extremum test (:1194-1258) into a flag per (s, y, x)
//   k_sift_compact    the flags compacted in scan order (s, y, x): a lane counts a fixed chunk of SIFT_CHUNK flags, the
//                     host (which needs the total anyway to size the next launch) scans the chunk counts, a lane emits its chunk
//   k_sift_refine     a lane per candidate: the five-step loop with the pivoted 3 x 3 elimination in double (:1267-1427)
//   k_sift_grad       modulus and angle of levels 0 .. S - 1 (update_gradient, :1447-1530)
//   k_sift_orient     a lane per keypoint: the 36-bin histogram in the window's pixel order, its peaks (:1559-1692)
//   k_sift_describe   a lane per (keypoint, kept orientation): the 4 x 4 x 8 histogram in the window's pixel order, VLFeat's two
//                     normalisations (:1923-2093), then COLMAP's L1_ROOT / L2, the bytes and the UBC order (utils.cc:47-77,
//                     sift.cc:58-74)
// What the reference takes from the host libm is computed by the host libm here too: the Gaussian taps, the fast_expn table,
// pow(2, s / S) of a keypoint's sigma and sin / cos of its orientation.  The device does + - * / sqrt and comparisons only.
// No atomics; no result depends on the launch geometry.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"
#include "sift_image_ops.h"

namespace {

struct SiftCand {  // a refined candidate: the host keeps the good ones and fills sigma (pow)
  int32_t ix, iy, is, good;
  double xn, yn, sn;
};
struct SiftKey {  // VlSiftKeypoint's fields the later stages read
  float x, y, sigma;
  int32_t is;
};
struct SiftJob {  // one descriptor: a keypoint and one kept orientation with its host sin / cos
  float x, y, sigma;
  int32_t is;
  double angle0, st0, ct0;
};

// the quadratic refinement of one candidate (sift.c:1267-1427)
__device__ __noinline__ void sift_refine_one(SiftCand* out, const float* __restrict__ dog, int w, int h, int S, int x, int y, int s, double tp,
                                             double te) {
  const int xo = 1, yo = w;
  const ptrdiff_t so = (ptrdiff_t)w * h;
  const int s_min = -1, s_max = S + 1;
  double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dss = 0, Dxy = 0, Dxs = 0, Dys = 0;
  double A[3 * 3], b[3];
  int dx = 0, dy = 0;
  const float* pt = dog;
#define at(dx, dy, ds) (*(pt + (dx)*xo + (dy)*yo + (ds)*so))
#define Aat(i, j) (A[(i) + (j)*3])
  #pragma unroll 1
  for (int iter = 0; iter < 5; ++iter) {
    x += dx;
    y += dy;
    pt = dog + xo * x + yo * y + so * (s - s_min);
    Dx = 0.5 * (at(+1, 0, 0) - at(-1, 0, 0));
    Dy = 0.5 * (at(0, +1, 0) - at(0, -1, 0));
    Ds = 0.5 * (at(0, 0, +1) - at(0, 0, -1));
    Dxx = (at(+1, 0, 0) + at(-1, 0, 0) - 2.0 * at(0, 0, 0));
    Dyy = (at(0, +1, 0) + at(0, -1, 0) - 2.0 * at(0, 0, 0));
    Dss = (at(0, 0, +1) + at(0, 0, -1) - 2.0 * at(0, 0, 0));
    Dxy = 0.25 * (at(+1, +1, 0) + at(-1, -1, 0) - at(-1, +1, 0) - at(+1, -1, 0));
    Dxs = 0.25 * (at(+1, 0, +1) + at(-1, 0, -1) - at(-1, 0, +1) - at(+1, 0, -1));
    Dys = 0.25 * (at(0, +1, +1) + at(0, -1, -1) - at(0, -1, +1) - at(0, +1, -1));
    Aat(0, 0) = Dxx;
    Aat(1, 1) = Dyy;
    Aat(2, 2) = Dss;
    Aat(0, 1) = Aat(1, 0) = Dxy;
    Aat(0, 2) = Aat(2, 0) = Dxs;
    Aat(1, 2) = Aat(2, 1) = Dys;
    b[0] = -Dx;
    b[1] = -Dy;
    b[2] = -Ds;
    for (int j = 0; j < 3; ++j) {
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
      if (maxabsa < 1e-10f) {
        b[0] = 0;
        b[1] = 0;
        b[2] = 0;
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
    for (int i = 2; i > 0; --i) {
      const double f = b[i];
      for (int ii = i - 1; ii >= 0; --ii) b[ii] -= f * Aat(ii, i);
    }
    dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
    dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
    if (dx == 0 && dy == 0) break;
  }
  const double val = at(0, 0, 0) + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
  const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
  const double xn = x + b[0], yn = y + b[1], sn = s + b[2];
  const bool good = fabs(val) > tp && score < (te + 1) * (te + 1) / te && score >= 0 && fabs(b[0]) < 1.5 && fabs(b[1]) < 1.5 &&
                    fabs(b[2]) < 1.5 && xn >= 0 && xn <= w - 1 && yn >= 0 && yn <= h - 1 && sn >= s_min && sn <= s_max;
#undef at
#undef Aat
  out->ix = x;
  out->iy = y;
  out->is = s;
  out->good = good;
  out->xn = xn;
  out->yn = yn;
  out->sn = sn;
}
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_refine(SiftCand* __restrict__ out, const uint32_t* __restrict__ cand, uint32_t n,
                                                            const float* __restrict__ dog, int w, int h, int S, double tp, double te) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cand[i];
  sift_refine_one(out + i, dog, w, h, S, (int)(c % (uint32_t)w), (int)(c / (uint32_t)w % (uint32_t)h), (int)(c / ((uint32_t)w * (uint32_t)h)), tp, te);
}

// update_gradient (sift.c:1447-1530): one-sided differences on the borders; w, h >= 2
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_grad(float* __restrict__ grad, const float* __restrict__ oct, int w, int h, uint32_t n) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % (uint32_t)w), y = (int)(i / (uint32_t)w % (uint32_t)h);
  const float* src = oct + (size_t)w * h + i;  // level s - s_min = s + 1
  float gx, gy;
  if (x == 0)
    gx = src[1] - src[0];
  else if (x == w - 1)
    gx = src[0] - src[-1];
  else
    gx = 0.5f * (src[1] - src[-1]);
  if (y == 0)
    gy = src[w] - src[0];
  else if (y == h - 1)
    gy = src[0] - src[-w];
  else
    gy = 0.5f * (src[w] - src[-w]);
  grad[2 * (size_t)i] = vl_fast_sqrt(gx * gx + gy * gy);
  grad[2 * (size_t)i + 1] = vl_mod_2pi((float)(vl_fast_atan2(gy, gx) + 2 * kVlPi));
}

// vl_sift_calc_keypoint_orientations (sift.c:1559-1692)
__global__ void __launch_bounds__(64) k_sift_orient(const SiftKey* __restrict__ keys, uint32_t n, const float* __restrict__ grad,
                                                    const double* __restrict__ expn, int w, int h, double xper, double* __restrict__ angles,
                                                    int32_t* __restrict__ nangles) {
  const uint32_t ki = blockIdx.x * 64 + threadIdx.x;
  if (ki >= n) return;
  const SiftKey k = keys[ki];
  const double winf = 1.5;
  const int xo = 2, yo = 2 * w;
  const size_t so = (size_t)2 * w * h;
  const double x = k.x / xper, y = k.y / xper, sigma = k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double sigmaw = winf * sigma;
  const double Wd = floor(3.0 * sigmaw);
  const int W = (int)(Wd > 1 ? Wd : 1);
  enum { nbins = 36 };
  double hist[nbins];
  nangles[ki] = 0;
  if (xi < 0 || xi > w - 1 || yi < 0 || yi > h - 1) return;
  #pragma unroll 1
  for (int i = 0; i < nbins; ++i) hist[i] = 0;
  const float* pt = grad + xo * xi + (size_t)yo * yi + so * si;
  for (int ys = max(-W, -yi); ys <= min(+W, h - 1 - yi); ++ys) {
    for (int xs = max(-W, -xi); xs <= min(+W, w - 1 - xi); ++xs) {
      const double dx = (double)(xi + xs) - x, dy = (double)(yi + ys) - y;
      const double r2 = dx * dx + dy * dy;
      if (r2 >= W * W + 0.6) continue;
      const double wgt = sift_fast_expn(expn, r2 / (2 * sigmaw * sigmaw));
      const double mod = *(pt + xs * xo + (ptrdiff_t)ys * yo);
      const double ang = *(pt + xs * xo + (ptrdiff_t)ys * yo + 1);
      const double fbin = nbins * ang / (2 * kVlPi);
      const int bin = (int)vl_floor_d(fbin - 0.5);  // VL_SIFT_BILINEAR_ORIENTATIONS is defined (sift.c:669)
      const double rbin = fbin - bin - 0.5;
      hist[(bin + nbins) % nbins] += (1 - rbin) * mod * wgt;
      hist[(bin + 1) % nbins] += (rbin)*mod * wgt;
    }
  }
  #pragma unroll 1
  for (int iter = 0; iter < 6; iter++) {
    double prev = hist[nbins - 1];
    const double first = hist[0];
    int i;
    #pragma unroll 1
    for (i = 0; i < nbins - 1; i++) {
      const double newh = (prev + hist[i] + hist[(i + 1) % nbins]) / 3.0;
      prev = hist[i];
      hist[i] = newh;
    }
    hist[i] = (prev + hist[i] + first) / 3.0;
  }
  double maxh = 0;
  #pragma unroll 1
  for (int i = 0; i < nbins; ++i) maxh = maxh > hist[i] ? maxh : hist[i];  // VL_MAX
  int na = 0;
  #pragma unroll 1
  for (int i = 0; i < nbins && na < 4; ++i) {
    const double h0 = hist[i], hm = hist[(i - 1 + nbins) % nbins], hp = hist[(i + 1 + nbins) % nbins];
    if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
      const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
      angles[4 * (size_t)ki + na++] = 2 * kVlPi * (i + di + 0.5) / nbins;
    }
  }
  nangles[ki] = na;
}

// normalize_histogram (sift.c:1702-1718) over the 128 bins
__device__ inline void sift_normalize(float* d) {
  float norm = 0.0f;
  #pragma unroll 1
  for (int i = 0; i < 128; ++i) norm += d[i] * d[i];
  norm = vl_fast_sqrt(norm) + kVlEpsF;
  #pragma unroll 1
  for (int i = 0; i < 128; ++i) d[i] /= norm;
}

// vl_sift_calc_keypoint_descriptor (sift.c:1923-2093) into descr[128 * job], then L1RootNormalize / L2Normalize,
// FeatureDescriptorsToUnsignedByte (utils.cc:47-77; the sums left to right) and the UBC bin order (sift.cc:58-74) into out
__global__ void __launch_bounds__(64) k_sift_describe(const SiftJob* __restrict__ jobs, uint32_t n, const float* __restrict__ grad,
                                                      const double* __restrict__ expn, int w, int h, double xper, int l2,
                                                      float* __restrict__ descr_all, uint8_t* __restrict__ out) {
  const uint32_t ji = blockIdx.x * 64 + threadIdx.x;
  if (ji >= n) return;
  const SiftJob k = jobs[ji];
  float* descr = descr_all + 128 * (size_t)ji;
  enum { NBO = 8, NBP = 4 };
  const double magnif = 3.0;
  const int xo = 2, yo = 2 * w;
  const size_t so = (size_t)2 * w * h;
  const double x = k.x / xper, y = k.y / xper, sigma = k.sigma / xper;
  const int xi = (int)(x + 0.5), yi = (int)(y + 0.5), si = k.is;
  const double angle0 = k.angle0, st0 = k.st0, ct0 = k.ct0;
  const double SBP = magnif * sigma + kVlEpsD;
  const int W = (int)floor(1.4142135623730951 * SBP * (NBP + 1) / 2.0 + 0.5);
  const int binyo = NBO * NBP, binxo = NBO;
  #pragma unroll 1
  for (int i = 0; i < 128; ++i) descr[i] = 0;
  // out of bounds: the reference leaves the caller's row as it is (uninitialised in sift.cc:359); here it is zero
  if (!(xi < 0 || xi >= w || yi < 0 || yi >= h - 1)) {
    const float* pt = grad + xi * xo + (size_t)yi * yo + si * so;
    float* dpt = descr + (NBP / 2) * binyo + (NBP / 2) * binxo;
    for (int dyi = max(-W, 1 - yi); dyi <= min(+W, h - yi - 2); ++dyi) {
      for (int dxi = max(-W, 1 - xi); dxi <= min(+W, w - xi - 2); ++dxi) {
        const float mod = *(pt + dxi * xo + (ptrdiff_t)dyi * yo + 0);
        const float angle = *(pt + dxi * xo + (ptrdiff_t)dyi * yo + 1);
        const float theta = vl_mod_2pi((float)(angle - angle0));
        const float dx = (float)(xi + dxi - x), dy = (float)(yi + dyi - y);
        const float nx = (float)((ct0 * dx + st0 * dy) / SBP);
        const float ny = (float)((-st0 * dx + ct0 * dy) / SBP);
        const float nt = (float)(NBO * theta / (2 * kVlPi));
        const float wsigma = 2.0f;  // windowSize = NBP / 2
        const float win = (float)sift_fast_expn(expn, (nx * nx + ny * ny) / (2.0 * wsigma * wsigma));
        const int binx = (int)vl_floor_f((float)(nx - 0.5)), biny = (int)vl_floor_f((float)(ny - 0.5)), bint = (int)vl_floor_f(nt);
        const float rbinx = (float)(nx - (binx + 0.5)), rbiny = (float)(ny - (biny + 0.5)), rbint = nt - bint;
        for (int dbinx = 0; dbinx < 2; ++dbinx)
          for (int dbiny = 0; dbiny < 2; ++dbiny)
            for (int dbint = 0; dbint < 2; ++dbint)
              if (binx + dbinx >= -(NBP / 2) && binx + dbinx < (NBP / 2) && biny + dbiny >= -(NBP / 2) && biny + dbiny < (NBP / 2)) {
                const float weight = win * mod * fabsf(1 - dbinx - rbinx) * fabsf(1 - dbiny - rbiny) * fabsf(1 - dbint - rbint);
                dpt[(bint + dbint) % NBO + (biny + dbiny) * binyo + (binx + dbinx) * binxo] += weight;
              }
      }
    }
    sift_normalize(descr);
    #pragma unroll 1
    for (int i = 0; i < 128; ++i)
      if (descr[i] > 0.2) descr[i] = (float)0.2;
    sift_normalize(descr);
  }
  if (!out) return;
  float norm = 0.0f;
  if (l2) {
    #pragma unroll 1
    for (int i = 0; i < 128; ++i) norm += descr[i] * descr[i];
  } else {
    #pragma unroll 1
    for (int i = 0; i < 128; ++i) norm += fabsf(descr[i]);
  }
  const bool scale = !l2 || norm > 0.0f;  // Eigen's normalized() leaves a zero row as it is
  if (l2) norm = sqrtf(norm);
  #pragma unroll 1
  for (int i = 0; i < 128; ++i) {
    float v = scale ? descr[i] / norm : descr[i];
    if (!l2) v = sqrtf(v);
    const float r = roundf(512.0f * v);
    const float lo = (0.0f < r) ? r : 0.0f;         // std::max(0, r): 0 for a NaN
    const float cl = (lo < 255.0f) ? lo : 255.0f;   // std::min(255, .)
    const int t = i & 7;
    out[128 * (size_t)ji + (i & ~7) + (t ? 8 - t : 0)] = (uint8_t)cl;
  }
}

inline int sift_shift(int x, int n) { return n >= 0 ? x << n : x >> -n; }  // VL_SHIFT_LEFT

// the Gaussian of _vl_sift_smooth (sift.c:782-798), by the host libm as the reference's
// appended to taps; returns the half-width
int sift_taps(double sigma, std::vector<float>* taps) {
  const double cw = std::ceil(4.0 * sigma);
  const size_t W = (size_t)(cw > 1 ? cw : 1), at = taps->size();
  taps->resize(at + 2 * W + 1);
  float* g = taps->data() + at;
  float acc = 0;
  for (size_t j = 0; j < 2 * W + 1; ++j) {
    const float d = ((float)((int)j - (int)W)) / ((float)sigma);
    g[j] = (float)std::exp(-0.5 * (d * d));
    acc += g[j];
  }
  for (size_t j = 0; j < 2 * W + 1; ++j) g[j] /= acc;
  return (int)W;
}

}  // namespace

struct SiftState {
  enum { img, oct, tmp, dog, grad, flags, counts, offs, cand, refined, keys, angles, nangles, jobs, descf, desc8, taps, expn, COUNT };
  DevBuf buf[COUNT];
  bool expn_ready = false;
  DevEvent ev[10];
  double stage_ms[DSM_SIFT_STAGES] = {0};  // of the last call (dsm_get_sift_time)
};

void dsm_sift_destroy(dsm_ctx* ctx) {
  delete ctx->sift;
  ctx->sift = nullptr;
}

extern "C" void dsm_sift_default_options(dsm_sift_options* o) {  // SiftExtractionOptions, src/feature/sift.h
  o->num_octaves = 4;
  o->octave_resolution = 3;
  o->first_octave = -1;
  o->max_num_orientations = 2;
  o->max_num_features = 8192;
  o->upright = 0;
  o->normalization = DSM_SIFT_L1_ROOT;
  o->reserved = 0;
  o->peak_threshold = 0.02 / 3;  // 0.02 / octave_resolution
  o->edge_threshold = 10.0;
}

extern "C" int dsm_extract_sift(dsm_ctx* ctx, const dsm_sift_options* options, const uint8_t* gray_u8, uint32_t width, uint32_t height,
                                uint32_t row_stride, uint32_t capacity, float* keypoints_out, uint8_t* descriptors_out,
                                uint32_t* num_features_out) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [&](int code, const char* msg) { return dsm_fail(ctx, code, msg); };
  dsm_sift_options o;
  if (options)
    o = *options;
  else
    dsm_sift_default_options(&o);
  if (num_features_out) *num_features_out = 0;
  if (!gray_u8 || !num_features_out || (capacity && !keypoints_out)) return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  if (width == 0 || height == 0 || row_stride < width) return fail(DSM_ERR_INVALID_ARGUMENT, "an empty image or row_stride below width");
  // SiftExtractionOptions::Check (sift.cc:218-234)
  if (!(o.max_num_features > 0) || !(o.octave_resolution > 0) || !(o.peak_threshold > 0.0) || !(o.edge_threshold > 0.0) ||
      !(o.max_num_orientations > 0))
    return fail(DSM_ERR_INVALID_ARGUMENT, "options that SiftExtractionOptions::Check rejects");
  if (o.normalization != DSM_SIFT_L1_ROOT && o.normalization != DSM_SIFT_L2) return fail(DSM_ERR_INVALID_ARGUMENT, "an unknown normalization");
  if (o.first_octave < -4 || o.first_octave > 16 || o.octave_resolution > 64 || o.num_octaves > 64)
    return fail(DSM_ERR_OUT_OF_RANGE, "first_octave outside -4 .. 16, octave_resolution or num_octaves above 64");
  const int S = o.octave_resolution, o_min = o.first_octave, s_min = -1, s_max = S + 1;
  int O = o.num_octaves;
  if (O < 0) {  // vl_sift_new, sift.c:885-887
    const double v = std::floor(std::log2((double)std::min(width, height))) - o_min - 3;
    O = (int)(v > 1 ? v : 1);
  }
  const uint64_t w0 = o_min >= 0 ? (uint64_t)width >> o_min : (uint64_t)width << -o_min;
  const uint64_t h0 = o_min >= 0 ? (uint64_t)height >> o_min : (uint64_t)height << -o_min;
  const uint64_t nel0 = std::max<uint64_t>(w0 * h0, (uint64_t)width * height);
  if (w0 > 0x3fffffffu || h0 > 65535 || nel0 * (uint64_t)(S + 3) >= 0x80000000ull)
    return fail(DSM_ERR_OUT_OF_RANGE, "the first octave has 2^31 or more samples or more than 65535 rows");
  // the scratch of the whole call, known from (width, height, first_octave, S): the levels, the DoG, the gradient, the flags
  const uint64_t chunks0 = (nel0 * S + SIFT_CHUNK - 1) / SIFT_CHUNK;
  const uint64_t scratch = (uint64_t)row_stride * height + nel0 * 4 * (uint64_t)((S + 3) + 1 + (S + 2) + 2 * S) + nel0 * S + chunks0 * 8;
  if (ctx->memory_budget && scratch > ctx->memory_budget)
    return fail(DSM_ERR_OUT_OF_RANGE, "the first octave's scratch exceeds the memory budget");

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  if (!ctx->sift) ctx->sift = new SiftState();
  SiftState& d = *ctx->sift;
  if (!d.expn_ready) {  // fast_expn_init, sift.c:713-720 (one entry more: fast_expn reads tab[i + 1] at x = EXPN_MAX)
    double tab[SIFT_EXPN_SZ + 2];
    for (int k = 0; k < SIFT_EXPN_SZ + 1; ++k) tab[k] = std::exp(-(double)k * (25.0 / SIFT_EXPN_SZ));
    tab[SIFT_EXPN_SZ + 1] = 0.0;
    HIPCHK(ctx, d.buf[SiftState::expn].reserve(sizeof(tab)));
    HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::expn].p, tab, sizeof(tab), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    d.expn_ready = true;
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
  HIPCHK(ctx, d.buf[SiftState::img].reserve((size_t)row_stride * height));
  HIPCHK(ctx, d.buf[SiftState::oct].reserve(nel0 * 4 * (S + 3)));
  HIPCHK(ctx, d.buf[SiftState::tmp].reserve(nel0 * 4));
  HIPCHK(ctx, d.buf[SiftState::dog].reserve(nel0 * 4 * (S + 2)));
  HIPCHK(ctx, d.buf[SiftState::grad].reserve(nel0 * 8 * S));
  HIPCHK(ctx, d.buf[SiftState::flags].reserve(nel0 * S));
  HIPCHK(ctx, d.buf[SiftState::counts].reserve(chunks0 * 4));
  HIPCHK(ctx, d.buf[SiftState::offs].reserve(chunks0 * 4));
  HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::img].p, gray_u8, (size_t)row_stride * height, hipMemcpyHostToDevice, st));
  float* oct = d.buf[SiftState::oct].as<float>();
  float* tmp = d.buf[SiftState::tmp].as<float>();

  // the filter geometry (vl_sift_new, sift.c:906-909) and every smoothing's taps, back to back
  const double sigman = 0.5, sigmak = std::pow(2.0, 1.0 / S), sigma0 = 1.6 * sigmak;
  const double dsigma0 = sigma0 * std::sqrt(1.0 - 1.0 / (sigmak * sigmak));
  std::vector<float> all_taps;
  size_t tap_at[64 + 4] = {0};
  int tap_w[64 + 4] = {0};
  auto add_taps = [&](int slot, double sigma) {
    tap_at[slot] = all_taps.size();
    tap_w[slot] = sift_taps(sigma, &all_taps);
  };
  {  // slot 0: the first octave's base (:1045-1051); slot 1: a next octave's base (:1120-1126); slot 2 + k: level s_min + 1 + k
    const double sa = sigma0 * std::pow(sigmak, s_min), sb = sigman * std::pow(2.0, -o_min);
    if (sa > sb) add_taps(0, std::sqrt(sa * sa - sb * sb));
    const int s_best = std::min(s_min + S, s_max);
    const double na = sigma0 * powf((float)sigmak, (float)s_min), nb = sigma0 * powf((float)sigmak, (float)(s_best - S));
    if (na > nb) add_taps(1, std::sqrt(na * na - nb * nb));
    for (int s = s_min + 1; s <= s_max; ++s) add_taps(2 + (s - s_min - 1), dsigma0 * std::pow(sigmak, s));
  }
  for (int k = 0; k < S + 4; ++k)
    if (tap_w[k] > 256) return fail(DSM_ERR_OUT_OF_RANGE, "a smoothing half-width above 256 samples");
  HIPCHK(ctx, d.buf[SiftState::taps].reserve(all_taps.size() * 4));
  HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::taps].p, all_taps.data(), all_taps.size() * 4, hipMemcpyHostToDevice, st));
  auto smooth = [&](float* out, const float* in, uint32_t w, uint32_t h, int slot) {  // _vl_sift_smooth: columns into tmp, rows into out
    const float* taps = d.buf[SiftState::taps].as<float>() + tap_at[slot];
    const int W = tap_w[slot];
    hipLaunchKernelGGL(k_sift_conv_cols, dim3((w + SIFT_TILE - 1) / SIFT_TILE, (h + SIFT_TILE - 1) / SIFT_TILE), dim3(SIFT_BLOCK),
                       (size_t)((SIFT_TILE + 2 * W) * SIFT_TILE + 2 * W + 1) * 4, st, tmp, in, (int)w, (int)h, taps, W);
    hipLaunchKernelGGL(k_sift_conv_rows, dim3((w + SIFT_BLOCK - 1) / SIFT_BLOCK, h), dim3(SIFT_BLOCK), (size_t)(SIFT_BLOCK + 4 * W + 1) * 4, st, out,
                       (const float*)tmp, (int)w, (int)h, taps, W);
  };

  // COLMAP's containers (sift.cc:279-385): a group per DoG level of every octave
  // (flat: level l holds level_keys[l] keypoints and the features level_first[l] .. level_first[l + 1] of kp_all / desc_all)
  std::vector<uint32_t> level_keys, level_first, counts;
  std::vector<float> kp_all;
  std::vector<uint8_t> desc_all, host;  // host: the octave's records, raw -- no container type of their own in the library
  level_first.push_back(0);
  const double tp = o.peak_threshold, te = o.edge_threshold;
  uint32_t pw = 0, ph = 0;  // the previous octave's size
  for (int oc = o_min; oc < o_min + O; ++oc) {
    const int wi = sift_shift((int)width, -oc), hi = sift_shift((int)height, -oc);
    // below 2 x 2 update_gradient is undefined, below 3 x 3 nothing is detected, and every later octave is smaller still
    if (wi < 2 || hi < 2) break;
    const uint32_t w = (uint32_t)wi, h = (uint32_t)hi, nel = w * h;
    HIPCHK(ctx, mark(0));
    if (oc == o_min) {  // vl_sift_process_first_octave, sift.c:1015-1052
      float* fimg = o_min == 0 ? oct : d.buf[SiftState::dog].as<float>();  // the float image: a buffer that is free until the DoG
      hipLaunchKernelGGL(k_sift_load, dim3(dsm_grid((uint64_t)width * height, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, fimg, d.buf[SiftState::img].as<uint8_t>(), width, height, row_stride);
      if (o_min < 0) {
        auto up = [&](float* dst, const float* src, uint32_t ww, uint32_t hh) {
          hipLaunchKernelGGL(k_sift_upsample_rows, dim3(dsm_grid((uint64_t)ww * hh, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, dst, src, ww, hh);
        };
        up(tmp, fimg, width, height);
        up(oct, tmp, height, 2 * width);
        for (int q = -1; q > o_min; --q) {  // the source's arguments as they are (:1023-1028)
          up(tmp, oct, width << -q, height << -q);
          up(oct, tmp, width << -q, 2 * (height << -q));
        }
      } else if (o_min > 0) {
        hipLaunchKernelGGL(k_sift_downsample, dim3(dsm_grid(nel, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, oct, (const float*)fimg, width, 1u << o_min, w, h);
      }
      if (tap_w[0]) smooth(oct, oct, w, h, 0);
    } else {  // vl_sift_process_next_octave, sift.c:1105-1126: level min(s_min + S, s_max) of the previous octave, every second sample
      const int s_best = std::min(s_min + S, s_max);
      // (the source level starts at (s_best - s_min) pw ph >= 4 nel: the new base does not reach it)
      hipLaunchKernelGGL(k_sift_downsample, dim3(dsm_grid(nel, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, oct, (const float*)(oct + (size_t)(s_best - s_min) * pw * ph), pw,
                         2u, w, h);
      if (tap_w[1]) smooth(oct, oct, w, h, 1);
    }
    pw = w;
    ph = h;
    HIPCHK(ctx, mark(1));
    for (int s = s_min + 1; s <= s_max; ++s)
      smooth(oct + (size_t)(s - s_min) * nel, oct + (size_t)(s - s_min - 1) * nel, w, h, 2 + (s - s_min - 1));
    HIPCHK(ctx, mark(2));
    HIPCHK(ctx, hipGetLastError());
    if (w < 3 || h < 3) continue;  // no interior sample: nothing to detect (its smoothing is not in the stage times)

    // vl_sift_detect
    const uint32_t ndog = nel * (uint32_t)(S + 2), nflag = nel * (uint32_t)S, chunks = (nflag + SIFT_CHUNK - 1) / SIFT_CHUNK;
    hipLaunchKernelGGL(k_sift_dog, dim3(dsm_grid(ndog, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[SiftState::dog].as<float>(), (const float*)oct, nel, ndog);
    hipLaunchKernelGGL(k_sift_detect, dim3(dsm_grid(nflag, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[SiftState::flags].as<uint8_t>(), (const float*)d.buf[SiftState::dog].as<float>(), (int)w, (int)h,
                       nflag, 0.8 * tp);
    auto compact = [&](const uint32_t* offs, uint32_t* out) {
      hipLaunchKernelGGL(k_sift_compact, dim3(dsm_grid(chunks, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, (const uint8_t*)d.buf[SiftState::flags].as<uint8_t>(), nflag, chunks, offs, out);
    };
    compact(nullptr, d.buf[SiftState::counts].as<uint32_t>());
    HIPCHK(ctx, mark(3));
    HIPCHK(ctx, hipGetLastError());
    counts.resize(chunks);
    HIPCHK(ctx, hipMemcpyAsync(counts.data(), d.buf[SiftState::counts].p, (size_t)chunks * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    uint32_t ncand = 0;
    for (uint32_t c = 0; c < chunks; ++c) {  // exclusive scan in place
      const uint32_t k = counts[c];
      counts[c] = ncand;
      ncand += k;
    }
    for (int k = 0; k < 3; ++k) HIPCHK(ctx, took(k, k));
    if (ncand == 0) continue;
    // what depends on the image: the candidates' records, and at most 4 orientations of each with a float and a byte descriptor
    if (ctx->memory_budget && scratch + (uint64_t)ncand * (4 + sizeof(SiftCand) + sizeof(SiftKey) + 36 + 4 * (sizeof(SiftJob) + 640)) > ctx->memory_budget)
      return fail(DSM_ERR_OUT_OF_RANGE, "the candidates' scratch exceeds the memory budget");
    HIPCHK(ctx, mark(4));
    HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::offs].p, counts.data(), (size_t)chunks * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, d.buf[SiftState::cand].reserve((size_t)ncand * 4));
    HIPCHK(ctx, d.buf[SiftState::refined].reserve((size_t)ncand * sizeof(SiftCand)));
    compact(d.buf[SiftState::offs].as<uint32_t>(), d.buf[SiftState::cand].as<uint32_t>());
    hipLaunchKernelGGL(k_sift_refine, dim3(dsm_grid(ncand, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[SiftState::refined].as<SiftCand>(), (const uint32_t*)d.buf[SiftState::cand].as<uint32_t>(), ncand,
                       (const float*)d.buf[SiftState::dog].as<float>(), (int)w, (int)h, S, tp, te);
    HIPCHK(ctx, mark(5));
    HIPCHK(ctx, hipGetLastError());
    // host layout: ncand SiftCand | ncand SiftKey | ncand x 4 angles | ncand counts | 4 ncand SiftJob
    const size_t at_keys = (size_t)ncand * sizeof(SiftCand), at_ang = at_keys + (size_t)ncand * sizeof(SiftKey), at_nang = at_ang + (size_t)ncand * 32,
                 at_jobs = (at_nang + (size_t)ncand * 4 + 7) / 8 * 8;
    host.resize(at_jobs + (size_t)ncand * 4 * sizeof(SiftJob));
    const SiftCand* refined = reinterpret_cast<const SiftCand*>(host.data());
    SiftKey* keys = reinterpret_cast<SiftKey*>(host.data() + at_keys);
    double* angles = reinterpret_cast<double*>(host.data() + at_ang);
    int32_t* nangles = reinterpret_cast<int32_t*>(host.data() + at_nang);
    SiftJob* jobs = reinterpret_cast<SiftJob*>(host.data() + at_jobs);
    HIPCHK(ctx, hipMemcpyAsync(host.data(), d.buf[SiftState::refined].p, (size_t)ncand * sizeof(SiftCand), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    // the good ones in order, with the host's pow (sift.c:1414-1424)
    const double xper = std::pow(2.0, oc);
    uint32_t nk = 0;
    for (uint32_t i = 0; i < ncand; ++i) {
      const SiftCand& c = refined[i];
      if (!c.good) continue;
      SiftKey& k = keys[nk++];
      k.is = c.is;
      k.x = (float)(c.xn * xper);
      k.y = (float)(c.yn * xper);
      k.sigma = (float)(sigma0 * std::pow(2.0, c.sn / S) * xper);
    }
    HIPCHK(ctx, took(3, 4));
    if (nk == 0) continue;  // sift.cc:306-308

    // orientations
    const uint32_t ngrad = nel * (uint32_t)S;
    HIPCHK(ctx, mark(6));
    hipLaunchKernelGGL(k_sift_grad, dim3(dsm_grid(ngrad, SIFT_BLOCK)), dim3(SIFT_BLOCK), 0, st, d.buf[SiftState::grad].as<float>(), (const float*)oct, (int)w, (int)h, ngrad);
    HIPCHK(ctx, mark(7));
    for (uint32_t i = 0; i < nk; ++i) {  // upright: one orientation of 0 (sift.cc:340-342)
      angles[4 * (size_t)i] = 0.0;
      nangles[i] = 1;
    }
    if (!o.upright) {
      HIPCHK(ctx, d.buf[SiftState::keys].reserve((size_t)nk * sizeof(SiftKey)));
      HIPCHK(ctx, d.buf[SiftState::angles].reserve((size_t)nk * 32));
      HIPCHK(ctx, d.buf[SiftState::nangles].reserve((size_t)nk * 4));
      HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::keys].p, keys, (size_t)nk * sizeof(SiftKey), hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_sift_orient, dim3(dsm_grid(nk, 64)), dim3(64), 0, st, (const SiftKey*)d.buf[SiftState::keys].as<SiftKey>(), nk, (const float*)d.buf[SiftState::grad].as<float>(),
                         (const double*)d.buf[SiftState::expn].as<double>(), (int)w, (int)h, xper, d.buf[SiftState::angles].as<double>(), d.buf[SiftState::nangles].as<int32_t>());
      HIPCHK(ctx, mark(8));
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(angles, d.buf[SiftState::angles].p, (size_t)nk * 32, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(nangles, d.buf[SiftState::nangles].p, (size_t)nk * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, took(5, 7));
    }
    HIPCHK(ctx, hipEventSynchronize(d.ev[7]));
    HIPCHK(ctx, took(4, 6));
    // the first max_num_orientations of every keypoint (sift.cc:351-352), sin / cos by the host libm (sift.c:1961-1962)
    uint32_t nj = 0;
    for (uint32_t i = 0; i < nk; ++i) {
      const int used = std::min<int>(nangles[i], o.max_num_orientations);
      for (int a = 0; a < used; ++a) {
        SiftJob& j = jobs[nj++];
        j.x = keys[i].x;
        j.y = keys[i].y;
        j.sigma = keys[i].sigma;
        j.is = keys[i].is;
        j.angle0 = angles[(size_t)i * 4 + a];
        j.st0 = std::sin(j.angle0);
        j.ct0 = std::cos(j.angle0);
      }
    }
    const size_t f0 = kp_all.size() / 4;  // the octave's first feature
    kp_all.resize((f0 + nj) * 4);
    if (descriptors_out) desc_all.resize((f0 + nj) * 128);
    if (descriptors_out && nj) {
      HIPCHK(ctx, d.buf[SiftState::jobs].reserve((size_t)nj * sizeof(SiftJob)));
      HIPCHK(ctx, d.buf[SiftState::descf].reserve((size_t)nj * 512));
      HIPCHK(ctx, d.buf[SiftState::desc8].reserve((size_t)nj * 128));
      HIPCHK(ctx, hipMemcpyAsync(d.buf[SiftState::jobs].p, jobs, (size_t)nj * sizeof(SiftJob), hipMemcpyHostToDevice, st));
      HIPCHK(ctx, mark(8));
      hipLaunchKernelGGL(k_sift_describe, dim3(dsm_grid(nj, 64)), dim3(64), 0, st, (const SiftJob*)d.buf[SiftState::jobs].as<SiftJob>(), nj, (const float*)d.buf[SiftState::grad].as<float>(),
                         (const double*)d.buf[SiftState::expn].as<double>(), (int)w, (int)h, xper, (int)(o.normalization == DSM_SIFT_L2), d.buf[SiftState::descf].as<float>(),
                         d.buf[SiftState::desc8].as<uint8_t>());
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, mark(9));
      HIPCHK(ctx, hipMemcpyAsync(desc_all.data() + f0 * 128, d.buf[SiftState::desc8].p, (size_t)nj * 128, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, took(6, 8));
    }
    // the groups per DoG level (sift.cc:310-384)
    int prev_level = -1;
    uint32_t j = 0;
    for (uint32_t i = 0; i < nk; ++i) {
      if (keys[i].is != prev_level) {
        level_keys.push_back(0);
        level_first.push_back((uint32_t)(f0 + j));
      }
      level_keys.back() += 1;
      prev_level = keys[i].is;
      const int used = std::min<int>(nangles[i], o.max_num_orientations);
      for (int a = 0; a < used; ++a, ++j) {
        float* kp = kp_all.data() + 4 * (f0 + j);
        kp[0] = keys[i].x + 0.5f;
        kp[1] = keys[i].y + 0.5f;
        kp[2] = keys[i].sigma;
        kp[3] = (float)jobs[j].angle0;
      }
      level_first.back() = (uint32_t)(f0 + j);
    }
  }
  HIPCHK(ctx, hipStreamSynchronize(st));

  // max_num_features (sift.cc:387-398): the coarsest levels until the count of keypoints exceeds it, the crossing level kept whole
  size_t first_level_to_keep = 0;
  int64_t num_features = 0;
  for (size_t i = level_keys.size(); i-- > 0;) {
    num_features += (int64_t)level_keys[i];
    if (num_features > o.max_num_features) {
      first_level_to_keep = i;
      break;
    }
  }
  // level_first[l + 1] is the end of level l: level_first = {0, end of level 0, end of level 1, ...}
  const size_t begin = level_first[first_level_to_keep], total = kp_all.size() / 4 - begin;
  *num_features_out = (uint32_t)total;
  if (total > capacity) return fail(DSM_ERR_OUT_OF_RANGE, "capacity below the number of features found (see num_features_out)");
  if (total) memcpy(keypoints_out, kp_all.data() + 4 * begin, total * 16);
  if (total && descriptors_out) memcpy(descriptors_out, desc_all.data() + 128 * begin, total * 128);
  return DSM_OK;
}

extern "C" int dsm_get_sift_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->sift) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_sift_time: no dsm_extract_sift call yet");
  memcpy(stage_ms, ctx->sift->stage_ms, sizeof(ctx->sift->stage_ms));
  return DSM_OK;
}
