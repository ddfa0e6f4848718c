// sift_image_ops.h -- what VLFeat's two extractors share on the device: mathop.h's fast float functions, the image-sized
// passes of a Gaussian scale space (load, downsampling, vl_imconvcol_vf with continuity padding in both directions, the DoG, the
// 26-neighbour extremum test and the compaction of its flags).  sift_extraction.hip (vl_sift) and
// covariant_sift.hip (covdet + scalespace) include it; every kernel is internal to the including file.
#ifndef DAGSFM_AMD_CSRC_SIFT_IMAGE_OPS_H_
#define DAGSFM_AMD_CSRC_SIFT_IMAGE_OPS_H_
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace {

constexpr int SIFT_BLOCK = 256;
constexpr uint32_t SIFT_CHUNK = 256;  // flags one lane of the compaction walks
constexpr double kVlPi = 3.141592653589793;      // VL_PI, mathop.h:28
constexpr double kVlEpsD = 2.220446049250313e-16;  // VL_EPSILON_D
constexpr float kVlEpsF = 1.19209290E-07F;         // VL_EPSILON_F
constexpr int SIFT_EXPN_SZ = 256;                  // EXPN_SZ, EXPN_MAX = 25.0 (sift.c:671-672)

// ---- mathop.h, operation for operation
__device__ inline float vl_fast_resqrt(float x) {  // mathop.h:479-501
  union {
    float x;
    int32_t i;
  } u;
  const float xhalf = 0.5f * x;
  u.x = x;
  u.i = 0x5f3759df - (u.i >> 1);
  u.x = u.x * (1.5f - xhalf * u.x * u.x);
  u.x = u.x * (1.5f - xhalf * u.x * u.x);
  return u.x;
}
__device__ inline float vl_fast_sqrt(float x) { return ((double)x < 1e-8) ? 0.0f : x * vl_fast_resqrt(x); }  // :544-548
__device__ inline float vl_fast_atan2(float y, float x) {  // :407-424
  float angle, r;
  const float c3 = 0.1821F, c1 = 0.9675F;
  const float abs_y = fabsf(y) + kVlEpsF;
  if (x >= 0) {
    r = (x - abs_y) / (x + abs_y);
    angle = (float)(kVlPi / 4);
  } else {
    r = (x + abs_y) / (abs_y - x);
    angle = (float)(3 * kVlPi / 4);
  }
  angle += (c3 * r * r - c1) * r;
  return (y < 0) ? -angle : angle;
}
__device__ inline float vl_mod_2pi(float x) {  // :109-115
  while (x > (float)(2 * kVlPi)) x -= (float)(2 * kVlPi);
  while (x < 0.0F) x += (float)(2 * kVlPi);
  return x;
}
__device__ inline long vl_floor_f(float x) {  // :134-140
  const long xi = (long)x;
  if (x >= 0 || (float)xi == x) return xi;
  return xi - 1;
}
__device__ inline long vl_floor_d(double x) {  // :146-152
  const long xi = (long)x;
  if (x >= 0 || (double)xi == x) return xi;
  return xi - 1;
}
__device__ inline double sift_fast_expn(const double* __restrict__ tab, double x) {  // sift.c:691-706
  if (x > 25.0) return 0.0;
  x *= SIFT_EXPN_SZ / 25.0;
  const int i = (int)vl_floor_d(x);
  const double r = x - i;
  const double a = tab[i], b = tab[i + 1];
  return a + r * (b - a);
}

// ---- the octave's base
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_load(float* __restrict__ dst, const uint8_t* __restrict__ src, uint32_t w, uint32_t h,
                                                          uint32_t stride) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= w * h) return;
  dst[i] = (float)src[(size_t)(i / w) * stride + i % w] / 255.0f;  // sift.cc:288
}
// copy_and_upsample_rows (sift.c:738-758): dst is the transpose, 2 width rows of height
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_upsample_rows(float* __restrict__ dst, const float* __restrict__ src, uint32_t width,
                                                                   uint32_t height) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= width * height) return;
  const uint32_t y = i / width, x = i % width;
  const float a = src[i];
  const float b = x + 1 < width ? src[i + 1] : a;
  dst[(size_t)(2 * x) * height + y] = a;
  dst[(size_t)(2 * x + 1) * height + y] = x + 1 < width ? 0.5f * (a + b) : a;
}
// copy_and_downsample (sift.c:835-851) by d = 2^k: the dw x dh pixels the next octave reads
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_downsample(float* __restrict__ dst, const float* __restrict__ src, uint32_t width, uint32_t d,
                                                                uint32_t dw, uint32_t dh) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= dw * dh) return;
  dst[i] = src[(size_t)(i / dw) * d * width + (size_t)(i % dw) * d];
}

// vl_imconvcol_vf, VL_PAD_BY_CONTINUITY: out(p) = sum_j in(clamp(p - W + j)) * taps[2 W - j], j ascending, one float product and
// one float sum per tap -- a pixel per lane, the block's tile plus a halo of W on either side in LDS, the taps behind it.  The
// halo is loaded with clamped coordinates, which is the source's padding; a half-width above the tile or the image only makes
// the load loop longer.  The transposes of the source cancel: k_sift_conv_cols is the first call of _vl_sift_smooth (down the
// columns, a 16 x 16 tile), k_sift_conv_rows the second (along the rows, a 256 x 1 tile).
constexpr int SIFT_TILE = 16;
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_conv_cols(float* __restrict__ dst, const float* __restrict__ src, int w, int h,
                                                               const float* __restrict__ taps, int W) {
  extern __shared__ float sift_lds[];
  const int rows = SIFT_TILE + 2 * W;
  float* tp = sift_lds + rows * SIFT_TILE;
  const int x0 = (int)blockIdx.x * SIFT_TILE, y0 = (int)blockIdx.y * SIFT_TILE;
  for (int k = (int)threadIdx.x; k < rows * SIFT_TILE; k += SIFT_BLOCK) {
    int q = y0 - W + k / SIFT_TILE;
    q = q < 0 ? 0 : (q > h - 1 ? h - 1 : q);
    const int xx = min(x0 + k % SIFT_TILE, w - 1);
    sift_lds[k] = src[(size_t)q * w + xx];
  }
  for (int k = (int)threadIdx.x; k <= 2 * W; k += SIFT_BLOCK) tp[k] = taps[k];
  __syncthreads();
  const int tx = (int)threadIdx.x % SIFT_TILE, ty = (int)threadIdx.x / SIFT_TILE;
  const int x = x0 + tx, y = y0 + ty;
  if (x >= w || y >= h) return;
  float acc = 0;
#pragma unroll 1
  for (int j = 0; j <= 2 * W; ++j) acc += sift_lds[(ty + j) * SIFT_TILE + tx] * tp[2 * W - j];
  dst[(size_t)y * w + x] = acc;
}
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_conv_rows(float* __restrict__ dst, const float* __restrict__ src, int w, int h,
                                                               const float* __restrict__ taps, int W) {
  extern __shared__ float sift_lds[];
  const int span = SIFT_BLOCK + 2 * W;
  float* tp = sift_lds + span;
  const int x0 = (int)blockIdx.x * SIFT_BLOCK, y = (int)blockIdx.y;
  const float* row = src + (size_t)y * w;
  for (int k = (int)threadIdx.x; k < span; k += SIFT_BLOCK) {
    int q = x0 - W + k;
    q = q < 0 ? 0 : (q > w - 1 ? w - 1 : q);
    sift_lds[k] = row[q];
  }
  for (int k = (int)threadIdx.x; k <= 2 * W; k += SIFT_BLOCK) tp[k] = taps[k];
  __syncthreads();
  const int x = x0 + (int)threadIdx.x;
  if (x >= w) return;
  float acc = 0;
#pragma unroll 1
  for (int j = 0; j <= 2 * W; ++j) acc += sift_lds[(int)threadIdx.x + j] * tp[2 * W - j];
  dst[(size_t)y * w + x] = acc;
}

__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_dog(float* __restrict__ dog, const float* __restrict__ oct, uint32_t nel, uint32_t n) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i < n) dog[i] = oct[(size_t)i + nel] - oct[i];
}

// the strict 26-neighbour test with the 0.8 tp gate (sift.c:1199-1232); flag index = (s * h + y) * w + x, the reference's scan order
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_detect(uint8_t* __restrict__ flags, const float* __restrict__ dog, int w, int h, uint32_t n,
                                                            double gate) {
  const uint32_t i = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int x = (int)(i % (uint32_t)w), y = (int)(i / (uint32_t)w % (uint32_t)h);
  uint8_t f = 0;
  if (x >= 1 && x < w - 1 && y >= 1 && y < h - 1) {
    const size_t so = (size_t)w * h;
    const float* pt = dog + so + i;  // DoG level s - s_min = s + 1
    const float v = *pt;
    bool mx = (double)v >= gate, mn = (double)v <= -gate;
    for (int ds = -1; ds <= 1 && (mx || mn); ++ds)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          if (!ds && !dy && !dx) continue;
          const float u = pt[(ptrdiff_t)ds * (ptrdiff_t)so + dy * w + dx];
          mx = mx && v > u;
          mn = mn && v < u;
        }
    f = mx || mn;
  }
  flags[i] = f;
}

// offs == NULL: out[c] = the number of flags in chunk c; else the set flags' indices to out[offs[c] ...], in order
__global__ void __launch_bounds__(SIFT_BLOCK) k_sift_compact(const uint8_t* __restrict__ flags, uint32_t n, uint32_t chunks, const uint32_t* __restrict__ offs,
                                                             uint32_t* __restrict__ out) {
  const uint32_t c = blockIdx.x * SIFT_BLOCK + threadIdx.x;
  if (c >= chunks) return;
  const uint32_t lo = c * SIFT_CHUNK, hi = min(n, lo + SIFT_CHUNK);
  uint32_t k = offs ? offs[c] : 0u;
  for (uint32_t i = lo; i < hi; ++i)
    if (flags[i]) {
      if (offs) out[k] = i;
      ++k;
    }
  if (!offs) out[c] = k;
}

}  // namespace

#endif  // DAGSFM_AMD_CSRC_SIFT_IMAGE_OPS_H_
