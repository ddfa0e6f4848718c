// patch_match.hip -- PatchMatch multi-view stereo: PatchMatchCuda of src/mvs/patch_match_cuda.cu restated for
// gfx950, operation for operation in IEEE float and in the reference's evaluation order (-ffp-contract=off; / and sqrt are
// correctly rounded; rsqrt(x) is 1.0f / sqrtf(x)).
//
//   k_pm_filter        GpuMatRefImage::Filter (gpu_mat_ref_image.cu:44-83): a thread per pixel, the bilaterally weighted sum and
//                      squared sum of the window and the re-quantised reference image uint8(255.0f * (b / 255.0f))
//   k_pm_init          FillWithRandomNumbers (gpu_mat.h:140-152) and InitNormalMap (:732-743) with GenerateRandomDepth /
//                      GenerateRandomNormal (:91-124); the 0.5 of prev_sel_prob_map (:1635)
//   k_pm_initial_cost  ComputeInitialCost (:760-803)
//   k_pm_sweep_wave, k_pm_backward (product), k_pm_sweep (check build)
//                      SweepFromTopToBottom (:824-1133) with PropagateDepth (:202-227), PerturbDepth / PerturbNormal (:126-190),
//                      ComputeViewingAngles (:232-257), ComposeHomography (:259-315), PhotoConsistencyCostComputer::Compute
//                      (:348-445), ComputeGeomConsistencyCost (:451-514), FindMinCost (:518-528, `<=`: the last minimum wins),
//                      TransformPDFToCDF (:580-593) and LikelihoodComputer (:595-729)
//   k_pm_rotate        Rotate (:1659-1746) with RotateNormalMap (:746-758) and CudaRotate (cuda_rotate.h:56-72): every map of a
//                      problem a quarter turn counter-clockwise, physically, as the reference does
// The host: InitTransforms (:1500-1608) with mvs/image.cc:92-140 in float, the schedule of RunWithWindowSizeAndStep
// (:1283-1294), the tables and constants of DESIGN.md 24.
//
// Schedule: a batch of problems per launch (blockIdx.y).  The product's sweep is k_pm_sweep_wave, a wave per column of the
// rotated frame (see there), with k_pm_backward for the backward messages; the check build also has k_pm_sweep, the
// reference's own schedule -- a lane per column, the rows walked serially, a wave per 64 columns -- as the independently
// written cross-check (DSM_PATCH_MATCH_LANES).  k_pm_initial_cost is a lane per column in both.  The window rows of the
// reference image are staged in LDS as bytes -- 3 x 64 columns wide as ReadRefImageIntoSharedMemory (:530-578) has them for a
// wave of columns, the 2 * radius + 1 columns of its window for a wave of one -- in a ring of 2 * radius + 1 rows of which
// one is replaced per row.  window_radius, window_step, num_samples and the source count are run-time values; the sweep is
// instantiated on the geometric term and the filter only (four kernels).  No atomics; every loop has a bound that does not depend on data
// (GenerateRandomNormal's rejection loop ends after 64 rejected pairs with the normal (0, 0, -1)).
//
// Where the reference leaves the result to the hardware, the contract is (tests/patch_match_ref.py):
//   random numbers   Philox4x32-10, key (seed, reference image index), counter (draw index, a, b, stream kind): kind 0 is the
//                    pixel (a, b) = (row, col) of the initialisation, kind 1 the column b of the rotated frame in sweep number a;
//                    u = ((word0 >> 8) + 1) * 2^-24, in (0, 1] like curand_uniform
//   source images    software bilinear interpolation in float over the bytes, texel b / 255.0f, zero border; depth maps
//                    nearest, zero border; a coordinate that is not finite or lies outside [-1, width] x [-1, height] gives 0
//                    before any index is formed
//   min / max        fminf / fmaxf
//   bilateral weight the product of a per-tap table and a per-byte-difference table, both the host libm's double exp rounded to float
//   exp, sin, cos    the double value of the float argument rounded to float: exact_exp.h, exact_trig.h
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ctx.h"

#define DSM_XT static __device__ __noinline__
#define DSM_XT_CONST __device__ const
#include "exact_trig.h"
#define DSM_XE static __host__ __device__ inline
#include "exact_exp.h"

namespace {

constexpr int PM_LANES = 64;              // columns of one wave; the LDS stripe is 3 * PM_LANES columns wide
constexpr int PM_POSE = 4 + 9 + 3 + 3 + 12 + 12;  // K, R, T, C, P, inv_P of one source image (:1557)
constexpr uint32_t PM_MAX_SIDE = 32768;
constexpr int PM_MAX_RADIUS = 32;         // kMaxPatchMatchWindowRadius
constexpr int PM_MAX_REJECT = 64;
constexpr uint64_t PM_DEFAULT_CHUNK_BYTES = 4ull << 30;
constexpr int PM_BLOCK = 256;

struct PmImage {
  uint64_t px_off;     // first byte in the pixel blob, rows of `w` bytes
  uint64_t depth_off;  // first float in the depth blob, rows of `w` floats
  uint32_t w, h;
};

struct PmProb {
  int32_t w0, h0, S, ref;
  float dmin, dmax;
  uint32_t key1, pad;
  const uint32_t* src;  // [S] indices into the image table
  const float* poses;   // [4 rotations][S][PM_POSE]
  float K[4][4];        // {fx, cx, fy, cy} of the reference image per rotation
  float iK[4][4];       // {1/fx, -cx/fx, 1/fy, -cy/fy}
  uint8_t* ref_img[2];
  float* sum[2];
  float* sq[2];
  float* depth[2];
  float* normal[2];
  float* cost[2];
  float* sel;
  float* prev;
  uint8_t* mask[2];
  float* fwd;    // [S][max(w0, h0)]
  float* probs;  // [S][max(w0, h0)]
};

struct PmParams {
  const PmProb* probs;
  const PmImage* images;
  const uint8_t* pixels;
  const float* depths;
  const float* w_spatial;  // [taps], in the order of the window loops
  const float* w_color;    // [256]
  const float* tex;        // [256]: b / 255.0f
  int32_t radius, step, num_samples, filter_min_num_consistent;
  uint32_t seed, sweep_no;
  int32_t rot, cur;
  float perturbation, perturbation_normal, prev_weight;
  float cos_min_tri, inv_inc_sigma_sq, inv_ncc_sigma_sq, ncc_norm;
  float geom_reg, geom_max_cost;
  float filter_min_ncc_prob, filter_cos_min_tri, filter_geom_max_cost;
};

// ---- random numbers ----
__device__ inline uint32_t pm_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0;
    c1 = n1;
    c2 = n2;
    c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}
struct PmRand {
  uint32_t k0, k1, a, b, kind, d;
  __device__ inline float at(uint32_t index) const {  // draw `index` of the stream, without advancing
    const uint32_t r = pm_philox(k0, k1, index, a, b, kind);
    return (float)((r >> 8) + 1u) * 5.9604644775390625e-08f;
  }
  __device__ inline float uniform() {
    const uint32_t r = pm_philox(k0, k1, d++, a, b, kind);
    return (float)((r >> 8) + 1u) * 5.9604644775390625e-08f;  // 2^-24
  }
};

__device__ inline float pm_exp(float x) { return (float)dsm_exp((double)x); }
__device__ inline float pm_dot3(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ inline float pm_rsqrt(float x) { return 1.0f / sqrtf(x); }

// ---- the source images ----
__device__ inline float pm_texel(const uint8_t* px, const float* tex, int w, int h, int x, int y) {
  if (x < 0 || y < 0 || x >= w || y >= h) return 0.0f;
  return tex[px[(size_t)y * w + x]];
}
// tex2DLayered with linear filtering at the unnormalised coordinate (x, y)
__device__ inline float pm_sample(const uint8_t* px, const float* tex, int w, int h, float x, float y) {
  if (!(x >= -1.0f && x <= (float)w && y >= -1.0f && y <= (float)h)) return 0.0f;
  const float xb = x - 0.5f, yb = y - 0.5f;
  const float fx = floorf(xb), fy = floorf(yb);
  const float a = xb - fx, b = yb - fy;
  const float a1 = 1.0f - a, b1 = 1.0f - b;
  const int ix = (int)fx, iy = (int)fy;  // -2 .. w - 1, -2 .. h - 1
  float v = (a1 * b1) * pm_texel(px, tex, w, h, ix, iy);
  v = v + (a * b1) * pm_texel(px, tex, w, h, ix + 1, iy);
  v = v + (a1 * b) * pm_texel(px, tex, w, h, ix, iy + 1);
  v = v + (a * b) * pm_texel(px, tex, w, h, ix + 1, iy + 1);
  return v;
}
// tex2DLayered with point filtering
__device__ inline float pm_sample_depth(const float* dm, int w, int h, float x, float y) {
  if (!(x >= -1.0f && x <= (float)w && y >= -1.0f && y <= (float)h)) return 0.0f;
  const int ix = (int)floorf(x), iy = (int)floorf(y);
  if (ix < 0 || iy < 0 || ix >= w || iy >= h) return 0.0f;
  return dm[(size_t)iy * w + ix];
}

// ---- geometry ----
__device__ inline void pm_point_at_depth(const float* iK, float row, float col, float depth, float* point) {
  point[0] = depth * (iK[0] * col + iK[1]);
  point[1] = depth * (iK[2] * row + iK[3]);
  point[2] = depth;
}

__device__ inline float pm_propagate_depth(const float* iK, float depth1, const float* normal1, float row1, float row2) {
  const float x1 = depth1 * (iK[2] * row1 + iK[3]);
  const float y1 = depth1;
  const float x2 = x1 + normal1[2];
  const float y2 = y1 - normal1[1];
  const float x4 = iK[2] * row2 + iK[3];
  const float denom = x2 - x1 + x4 * (y1 - y2);
  const float kEps = 1e-5f;
  if (fabsf(denom) < kEps) return depth1;
  const float nom = y1 * x2 - x1 * y2;
  return nom / denom;
}

__device__ inline void pm_viewing_angles(const float* pose, const float* point, const float* normal, float* cos_tri, float* cos_inc) {
  const float* C = pose + 16;
  const float SX[3] = {C[0] - point[0], C[1] - point[1], C[2] - point[2]};
  const float RX_inv_norm = pm_rsqrt(pm_dot3(point, point));
  const float SX_inv_norm = pm_rsqrt(pm_dot3(SX, SX));
  *cos_inc = pm_dot3(SX, normal) * SX_inv_norm;
  *cos_tri = pm_dot3(SX, point) * RX_inv_norm * SX_inv_norm;
}

__device__ inline void pm_compose_homography(const float* pose, const float* iK, int row, int col, float depth, const float* normal, float* H) {
  const float* K = pose;
  const float* R = pose + 4;
  const float* T = pose + 13;
  const float dist = depth * (normal[0] * (iK[0] * col + iK[1]) + normal[1] * (iK[2] * row + iK[3]) + normal[2]);
  const float inv_dist = 1.0f / dist;
  const float inv_dist_N0 = inv_dist * normal[0];
  const float inv_dist_N1 = inv_dist * normal[1];
  const float inv_dist_N2 = inv_dist * normal[2];
  H[0] = iK[0] * (K[0] * (R[0] + inv_dist_N0 * T[0]) + K[1] * (R[6] + inv_dist_N0 * T[2]));
  H[1] = iK[2] * (K[0] * (R[1] + inv_dist_N1 * T[0]) + K[1] * (R[7] + inv_dist_N1 * T[2]));
  H[2] = K[0] * (R[2] + inv_dist_N2 * T[0]) + K[1] * (R[8] + inv_dist_N2 * T[2]) +
         iK[1] * (K[0] * (R[0] + inv_dist_N0 * T[0]) + K[1] * (R[6] + inv_dist_N0 * T[2])) +
         iK[3] * (K[0] * (R[1] + inv_dist_N1 * T[0]) + K[1] * (R[7] + inv_dist_N1 * T[2]));
  H[3] = iK[0] * (K[2] * (R[3] + inv_dist_N0 * T[1]) + K[3] * (R[6] + inv_dist_N0 * T[2]));
  H[4] = iK[2] * (K[2] * (R[4] + inv_dist_N1 * T[1]) + K[3] * (R[7] + inv_dist_N1 * T[2]));
  H[5] = K[2] * (R[5] + inv_dist_N2 * T[1]) + K[3] * (R[8] + inv_dist_N2 * T[2]) +
         iK[1] * (K[2] * (R[3] + inv_dist_N0 * T[1]) + K[3] * (R[6] + inv_dist_N0 * T[2])) +
         iK[3] * (K[2] * (R[4] + inv_dist_N1 * T[1]) + K[3] * (R[7] + inv_dist_N1 * T[2]));
  H[6] = iK[0] * (R[6] + inv_dist_N0 * T[2]);
  H[7] = iK[2] * (R[7] + inv_dist_N1 * T[2]);
  H[8] = R[8] + iK[1] * (R[6] + inv_dist_N0 * T[2]) + iK[3] * (R[7] + inv_dist_N1 * T[2]) + inv_dist_N2 * T[2];
}

__device__ inline void pm_hnorm(const float* H, float x, float y, float* out) {  // Mat33DotVec3Homogeneous
  const float inv_z = 1.0f / (H[6] * x + H[7] * y + H[8]);
  out[0] = inv_z * (H[0] * x + H[1] * y + H[2]);
  out[1] = inv_z * (H[3] * x + H[4] * y + H[5]);
}

__device__ inline float pm_resolution_prob(const float* H, float row, float col, int radius) {
  float src1[2], src2[2], src3[2], src4[2];
  pm_hnorm(H, col - radius, row - radius, src1);
  pm_hnorm(H, col - radius, row + radius, src2);
  pm_hnorm(H, col + radius, row + radius, src3);
  pm_hnorm(H, col + radius, row - radius, src4);
  const int window = 2 * radius + 1;
  const float ref_area = (float)(window * window);
  const float src_area = fabsf(0.5f * (src1[0] * src2[1] - src2[0] * src1[1] - src1[0] * src4[1] + src2[0] * src3[1] - src3[0] * src2[1] +
                                       src4[0] * src1[1] + src3[0] * src4[1] - src4[0] * src3[1]));
  if (ref_area > src_area) return src_area / ref_area;
  return ref_area / src_area;
}

// ---- LikelihoodComputer ----
__device__ inline float pm_ncc_prob(const PmParams& P, float cost) { return pm_exp(cost * cost * P.inv_ncc_sigma_sq) * P.ncc_norm; }
__device__ inline float pm_forward_message(const PmParams& P, float cost, float prev) {
  const float kUniformProb = 0.5f, kNoChangeProb = 0.99999f;
  const float kChangeProb = 1.0f - kNoChangeProb;
  const float emission = pm_ncc_prob(P, cost);
  const float zn0 = (prev * kChangeProb + (1.0f - prev) * kNoChangeProb) * kUniformProb;
  const float zn1 = (prev * kNoChangeProb + (1.0f - prev) * kChangeProb) * emission;
  return zn1 / (zn0 + zn1);
}
__device__ inline float pm_backward_message(const PmParams& P, float cost, float prev) {
  const float kUniformProb = 0.5f, kNoChangeProb = 0.99999f;
  const float kChangeProb = 1.0f - kNoChangeProb;
  const float emission = pm_ncc_prob(P, cost);
  const float zn0 = prev * emission * kChangeProb + (1.0f - prev) * kUniformProb * kNoChangeProb;
  const float zn1 = prev * emission * kNoChangeProb + (1.0f - prev) * kUniformProb * kChangeProb;
  return zn1 / (zn0 + zn1);
}
__device__ inline float pm_sel_prob(float alpha, float beta, float prev, float prev_weight) {
  const float zn0 = (1.0f - alpha) * (1.0f - beta);
  const float zn1 = alpha * beta;
  const float curr = zn1 / (zn0 + zn1);
  return prev_weight * prev + (1.0f - prev_weight) * curr;
}
__device__ inline float pm_tri_prob(const PmParams& P, float cos_tri) {
  const float a = fabsf(cos_tri);
  if (a > P.cos_min_tri) {
    const float scaled = 1.0f - (1.0f - a) / (1.0f - P.cos_min_tri);
    const float likelihood = 1.0f - scaled * scaled;
    return fminf(1.0f, fmaxf(0.0f, likelihood));
  }
  return 1.0f;
}
__device__ inline float pm_inc_prob(const PmParams& P, float cos_inc) {
  const float x = 1.0f - fmaxf(0.0f, cos_inc);
  return pm_exp(x * x * P.inv_inc_sigma_sq);
}

// ---- the LDS stripe of the reference image ----
struct PmTile {
  const float* tex;    // LDS copies of the two 256-entry tables
  const float* wcol;
  uint8_t* rows;       // [2 * radius + 1][stride]: image row r lives in slot (r + radius) % (2 * radius + 1)
  int32_t window;      // 2 * radius + 1
  int32_t stride;      // bytes of a row: 3 * PM_LANES columns for a wave of columns, PM_WTILE_STRIDE for the window of one column
};
__device__ inline void pm_tile_load_row(const PmTile& t, const uint8_t* img, int w, int h, int radius, int r, int col0, int lane) {
  uint8_t* dst = t.rows + (size_t)((r + radius) % t.window) * (3 * PM_LANES);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int c = col0 - PM_LANES + j * PM_LANES + lane;
    dst[j * PM_LANES + lane] = (r >= 0 && r < h && c >= 0 && c < w) ? img[(size_t)r * w + c] : (uint8_t)0;
  }
}
// ReadRefImageIntoSharedMemory: the window rows of `row`; all lanes of the block call it
__device__ inline void pm_tile_advance(const PmTile& t, const uint8_t* img, int w, int h, int radius, int row, int col0, int lane) {
  __syncthreads();  // the row that leaves the ring is no longer read
  if (row == 0) {
    for (int r = -radius; r <= radius; ++r) pm_tile_load_row(t, img, w, h, radius, r, col0, lane);
  } else {
    pm_tile_load_row(t, img, w, h, radius, row + radius, col0, lane);
  }
  __syncthreads();
}

// PhotoConsistencyCostComputer::Compute
__device__ inline float pm_photo_cost(const PmParams& P, const PmTile& t, const float* pose, const float* iK, const uint8_t* src_px, int src_w,
                                      int src_h, int row, int col, int center, float depth, const float* normal, float ref_sum, float ref_sq) {
  // center: the index of column `col` within a row of the tile
  const float kMaxCost = 2.0f;
  float tform[9];
  pm_compose_homography(pose, iK, row, col, depth, normal, tform);
  float tform_step[9];
  for (int i = 0; i < 9; ++i) tform_step[i] = P.step * tform[i];
  const int radius = P.radius;
  const int row_start = row - radius;
  const int col_start = col - radius;
  float col_src = tform[0] * col_start + tform[1] * row_start + tform[2];
  float row_src = tform[3] * col_start + tform[4] * row_start + tform[5];
  float z = tform[6] * col_start + tform[7] * row_start + tform[8];
  float base_col_src = col_src;
  float base_row_src = row_src;
  float base_z = z;
  const int center_byte = t.rows[(size_t)((row + radius) % t.window) * t.stride + center];
  float src_color_sum = 0.0f;
  float src_color_squared_sum = 0.0f;
  float src_ref_color_sum = 0.0f;
  float bilateral_weight_sum = 0.0f;
  int tap = 0;
  for (int wr = -radius; wr <= radius; wr += P.step) {
    const uint8_t* trow = t.rows + (size_t)((row + wr + radius) % t.window) * t.stride + center;
    for (int wc = -radius; wc <= radius; wc += P.step) {
      const float inv_z = 1.0f / z;
      const float norm_col_src = inv_z * col_src + 0.5f;
      const float norm_row_src = inv_z * row_src + 0.5f;
      const int b = trow[wc];
      const float ref_color = t.tex[b];
      const float src_color = pm_sample(src_px, t.tex, src_w, src_h, norm_col_src, norm_row_src);
      const int diff = b > center_byte ? b - center_byte : center_byte - b;
      const float bilateral_weight = P.w_spatial[tap] * t.wcol[diff];
      const float bilateral_weight_src = bilateral_weight * src_color;
      src_color_sum += bilateral_weight_src;
      src_color_squared_sum += bilateral_weight_src * src_color;
      src_ref_color_sum += bilateral_weight_src * ref_color;
      bilateral_weight_sum += bilateral_weight;
      col_src += tform_step[0];
      row_src += tform_step[3];
      z += tform_step[6];
      ++tap;
    }
    base_col_src += tform_step[1];
    base_row_src += tform_step[4];
    base_z += tform_step[7];
    col_src = base_col_src;
    row_src = base_row_src;
    z = base_z;
  }
  const float inv_bilateral_weight_sum = 1.0f / bilateral_weight_sum;
  src_color_sum *= inv_bilateral_weight_sum;
  src_color_squared_sum *= inv_bilateral_weight_sum;
  src_ref_color_sum *= inv_bilateral_weight_sum;
  const float ref_color_var = ref_sq - ref_sum * ref_sum;
  const float src_color_var = src_color_squared_sum - src_color_sum * src_color_sum;
  const float kMinVar = 1e-5f;
  if (ref_color_var < kMinVar || src_color_var < kMinVar) return kMaxCost;
  const float src_ref_color_covar = src_ref_color_sum - ref_sum * src_color_sum;
  const float src_ref_color_var = sqrtf(ref_color_var * src_color_var);
  return fmaxf(0.0f, fminf(kMaxCost, 1.0f - src_ref_color_covar / src_ref_color_var));
}

// ComputeGeomConsistencyCost
__device__ inline float pm_geom_cost(const float* pose, const float* K, const float* iK, const float* src_depth_map, int src_w, int src_h, float row,
                                     float col, float depth, float max_cost) {
  const float* Pm = pose + 19;
  const float* inv_P = pose + 31;
  float forward_point[3];
  pm_point_at_depth(iK, row, col, depth, forward_point);
  const float inv_forward_z = 1.0f / (Pm[8] * forward_point[0] + Pm[9] * forward_point[1] + Pm[10] * forward_point[2] + Pm[11]);
  float src_col = inv_forward_z * (Pm[0] * forward_point[0] + Pm[1] * forward_point[1] + Pm[2] * forward_point[2] + Pm[3]);
  float src_row = inv_forward_z * (Pm[4] * forward_point[0] + Pm[5] * forward_point[1] + Pm[6] * forward_point[2] + Pm[7]);
  const float src_depth = pm_sample_depth(src_depth_map, src_w, src_h, src_col + 0.5f, src_row + 0.5f);
  if (src_depth == 0.0f) return max_cost;
  src_col *= src_depth;
  src_row *= src_depth;
  const float backward_point_x = inv_P[0] * src_col + inv_P[1] * src_row + inv_P[2] * src_depth + inv_P[3];
  const float backward_point_y = inv_P[4] * src_col + inv_P[5] * src_row + inv_P[6] * src_depth + inv_P[7];
  const float backward_point_z = inv_P[8] * src_col + inv_P[9] * src_row + inv_P[10] * src_depth + inv_P[11];
  const float inv_backward_point_z = 1.0f / backward_point_z;
  const float backward_col = inv_backward_point_z * (K[0] * backward_point_x + K[1] * backward_point_z);
  const float backward_row = inv_backward_point_z * (K[2] * backward_point_y + K[3] * backward_point_z);
  const float diff_col = col - backward_col;
  const float diff_row = row - backward_row;
  return fminf(max_cost, sqrtf(diff_col * diff_col + diff_row * diff_row));
}

// PerturbNormal: the recursion of :171-176 as its four trials
__device__ inline void pm_perturb_normal(const float* iK, int row, int col, float perturbation, const float* normal, PmRand& rng, float* out) {
  const float view_ray[3] = {iK[0] * col + iK[1], iK[2] * row + iK[3], 1.0f};
  for (int trial = 0; trial < 4; ++trial) {
    const float a1 = (rng.uniform() - 0.5f) * perturbation;
    const float a2 = (rng.uniform() - 0.5f) * perturbation;
    const float a3 = (rng.uniform() - 0.5f) * perturbation;
    const float sin_a1 = (float)dsm_sin((double)a1), sin_a2 = (float)dsm_sin((double)a2), sin_a3 = (float)dsm_sin((double)a3);
    const float cos_a1 = (float)dsm_cos((double)a1), cos_a2 = (float)dsm_cos((double)a2), cos_a3 = (float)dsm_cos((double)a3);
    float R[9];
    R[0] = cos_a2 * cos_a3;
    R[1] = -cos_a2 * sin_a3;
    R[2] = sin_a2;
    R[3] = cos_a1 * sin_a3 + cos_a3 * sin_a1 * sin_a2;
    R[4] = cos_a1 * cos_a3 - sin_a1 * sin_a2 * sin_a3;
    R[5] = -cos_a2 * sin_a1;
    R[6] = sin_a1 * sin_a3 - cos_a1 * cos_a3 * sin_a2;
    R[7] = cos_a3 * sin_a1 + cos_a1 * sin_a2 * sin_a3;
    R[8] = cos_a1 * cos_a2;
    out[0] = R[0] * normal[0] + R[1] * normal[1] + R[2] * normal[2];
    out[1] = R[3] * normal[0] + R[4] * normal[1] + R[5] * normal[2];
    out[2] = R[6] * normal[0] + R[7] * normal[1] + R[8] * normal[2];
    if (!(pm_dot3(out, view_ray) >= 0.0f)) {
      const float inv_norm = pm_rsqrt(pm_dot3(out, out));
      out[0] *= inv_norm;
      out[1] *= inv_norm;
      out[2] *= inv_norm;
      return;
    }
    perturbation = 0.5f * perturbation;
  }
  out[0] = normal[0];
  out[1] = normal[1];
  out[2] = normal[2];
}

// ---- kernels ----
__global__ void __launch_bounds__(PM_BLOCK) k_pm_filter(PmParams P) {
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = pb.w0, h = pb.h0;
  const int i = blockIdx.x * PM_BLOCK + threadIdx.x;
  if (i >= w * h) return;
  const int row = i / w, col = i % w;
  const PmImage im = P.images[pb.ref];
  const uint8_t* px = P.pixels + im.px_off;
  const int bc = px[(size_t)row * w + col];
  const float center_color = P.tex[bc];
  float color_sum = 0.0f, color_squared_sum = 0.0f, bilateral_weight_sum = 0.0f;
  int tap = 0;
  for (int wr = -P.radius; wr <= P.radius; wr += P.step) {
    for (int wc = -P.radius; wc <= P.radius; wc += P.step) {
      const int r = row + wr, c = col + wc;
      const int b = (r >= 0 && r < h && c >= 0 && c < w) ? px[(size_t)r * w + c] : 0;
      const float color = P.tex[b];
      const int diff = b > bc ? b - bc : bc - b;
      const float bilateral_weight = P.w_spatial[tap] * P.w_color[diff];
      color_sum += bilateral_weight * color;
      color_squared_sum += bilateral_weight * color * color;
      bilateral_weight_sum += bilateral_weight;
      ++tap;
    }
  }
  color_sum /= bilateral_weight_sum;
  color_squared_sum /= bilateral_weight_sum;
  pb.ref_img[0][i] = (uint8_t)(255.0f * center_color);
  pb.sum[0][i] = color_sum;
  pb.sq[0][i] = color_squared_sum;
}

template <bool RANDOM>
__global__ void __launch_bounds__(PM_BLOCK) k_pm_init(PmParams P) {
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = pb.w0, h = pb.h0;
  const int i = blockIdx.x * PM_BLOCK + threadIdx.x;
  if (i >= w * h) return;
  const size_t n = (size_t)w * h;
  for (int s = 0; s < pb.S; ++s) pb.prev[(size_t)s * n + i] = 0.5f;
  if (!RANDOM) return;
  const int row = i / w, col = i % w;
  PmRand rng{P.seed, pb.key1, (uint32_t)row, (uint32_t)col, 0u, 0u};
  pb.depth[0][i] = rng.uniform() * (pb.dmax - pb.dmin) + pb.dmin;
  float v1 = 0.0f, v2 = 0.0f, s = 2.0f;
  bool found = false;
  for (int t = 0; t < PM_MAX_REJECT; ++t) {
    v1 = 2.0f * rng.uniform() - 1.0f;
    v2 = 2.0f * rng.uniform() - 1.0f;
    s = v1 * v1 + v2 * v2;
    if (s < 1.0f) {
      found = true;
      break;
    }
  }
  float normal[3] = {0.0f, 0.0f, -1.0f};
  if (found) {
    const float s_norm = sqrtf(1.0f - s);
    normal[0] = 2.0f * v1 * s_norm;
    normal[1] = 2.0f * v2 * s_norm;
    normal[2] = 1.0f - 2.0f * s;
  }
  const float* iK = pb.iK[0];
  const float view_ray[3] = {iK[0] * col + iK[1], iK[2] * row + iK[3], 1.0f};
  if (pm_dot3(normal, view_ray) > 0) {
    normal[0] = -normal[0];
    normal[1] = -normal[1];
    normal[2] = -normal[2];
  }
  for (int k = 0; k < 3; ++k) pb.normal[0][(size_t)k * n + i] = normal[k];
}

__device__ inline PmTile pm_tile_setup(const PmParams& P, float* smem, int lane) {
  for (int k = lane; k < 256; k += PM_LANES) {
    smem[k] = P.tex[k];
    smem[256 + k] = P.w_color[k];
  }
  PmTile t;
  t.tex = smem;
  t.wcol = smem + 256;
  t.rows = reinterpret_cast<uint8_t*>(smem + 512);
  t.window = 2 * P.radius + 1;
  t.stride = 3 * PM_LANES;
  return t;
}

__global__ void __launch_bounds__(PM_LANES) k_pm_initial_cost(PmParams P) {
  extern __shared__ float pm_smem[];
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = (P.rot & 1) ? pb.h0 : pb.w0, h = (P.rot & 1) ? pb.w0 : pb.h0;
  const int col0 = blockIdx.x * PM_LANES;
  if (col0 >= w) return;
  const int lane = threadIdx.x, col = col0 + lane;
  const PmTile tile = pm_tile_setup(P, pm_smem, lane);
  const size_t n = (size_t)w * h;
  const float* iK = pb.iK[P.rot];
  const uint8_t* ref = pb.ref_img[P.cur];
  for (int row = 0; row < h; ++row) {
    pm_tile_advance(tile, ref, w, h, P.radius, row, col0, lane);
    if (col >= w) continue;
    const size_t i = (size_t)row * w + col;
    const float depth = pb.depth[P.cur][i];
    const float normal[3] = {pb.normal[P.cur][i], pb.normal[P.cur][n + i], pb.normal[P.cur][2 * n + i]};
    const float ref_sum = pb.sum[P.cur][i], ref_sq = pb.sq[P.cur][i];
    for (int s = 0; s < pb.S; ++s) {
      const PmImage im = P.images[pb.src[s]];
      pb.cost[P.cur][(size_t)s * n + i] = pm_photo_cost(P, tile, pb.poses + ((size_t)P.rot * pb.S + s) * PM_POSE, iK, P.pixels + im.px_off, (int)im.w,
                                                       (int)im.h, row, col, PM_LANES + lane, depth, normal, ref_sum, ref_sq);
    }
  }
}

// FILTER: 0 none, 1 photometric (kFilterPhotoConsistency), 2 photometric and geometric (both flags)
#ifdef DSM_CHECK_BUILD
// The direct restatement of the reference's schedule, a lane per column: the independently written cross-check of
// k_pm_sweep_wave below (check build only, DSM_PATCH_MATCH_LANES).
template <bool GEOM, int FILTER>
__global__ void __launch_bounds__(PM_LANES) k_pm_sweep(PmParams P) {
  extern __shared__ float pm_smem[];
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = (P.rot & 1) ? pb.h0 : pb.w0, h = (P.rot & 1) ? pb.w0 : pb.h0;
  const int col0 = blockIdx.x * PM_LANES;
  if (col0 >= w) return;
  const int lane = threadIdx.x, col = col0 + lane;
  const bool active = col < w;
  const PmTile tile = pm_tile_setup(P, pm_smem, lane);
  const size_t n = (size_t)w * h;
  const int S = pb.S;
  const int ncols = pb.w0 > pb.h0 ? pb.w0 : pb.h0;
  const float* K = pb.K[P.rot];
  const float* iK = pb.iK[P.rot];
  const float* poses = pb.poses + (size_t)P.rot * S * PM_POSE;
  const uint8_t* ref = pb.ref_img[P.cur];
  float* depth_map = pb.depth[P.cur];
  float* normal_map = pb.normal[P.cur];
  float* cost_map = pb.cost[P.cur];
  uint8_t* mask = pb.mask[0];
  const float kUniformProb = 0.5f;

  // the backward messages of all rows, kept in sel_prob_map until the forward pass replaces them row by row
  if (active) {
    for (int s = 0; s < S; ++s) {
      float beta = kUniformProb;
      for (int row = h - 1; row >= 0; --row) {
        const size_t i = (size_t)s * n + (size_t)row * w + col;
        beta = pm_backward_message(P, cost_map[i], beta);
        pb.sel[i] = beta;
      }
      pb.fwd[(size_t)s * ncols + col] = kUniformProb;
    }
  }

  float prev_depth = 0.0f, prev_normal[3] = {0.0f, 0.0f, 0.0f};
  PmRand rng{P.seed, pb.key1, P.sweep_no, (uint32_t)col, 1u, 0u};
  if (active) {
    prev_depth = depth_map[col];
    for (int k = 0; k < 3; ++k) prev_normal[k] = normal_map[(size_t)k * n + col];
  }

  for (int row = 0; row < h; ++row) {
    pm_tile_advance(tile, ref, w, h, P.radius, row, col0, lane);
    if (!active) continue;
    const size_t i = (size_t)row * w + col;
    const float ref_sum = pb.sum[P.cur][i], ref_sq = pb.sq[P.cur][i];

    prev_depth = pm_propagate_depth(iK, prev_depth, prev_normal, row - 1, row);
    const float curr_depth = depth_map[i];
    const float curr_normal[3] = {normal_map[i], normal_map[n + i], normal_map[2 * n + i]};
    const float dmin = (1.0f - P.perturbation) * curr_depth, dmax = (1.0f + P.perturbation) * curr_depth;
    const float rand_depth = rng.uniform() * (dmax - dmin) + dmin;
    float rand_normal[3];
    pm_perturb_normal(iK, row, col, P.perturbation_normal, curr_normal, rng, rand_normal);

    float point[3];
    pm_point_at_depth(iK, row, col, curr_depth, point);
    for (int s = 0; s < S; ++s) {
      const float* pose = poses + (size_t)s * PM_POSE;
      const float alpha = pm_forward_message(P, cost_map[(size_t)s * n + i], pb.fwd[(size_t)s * ncols + col]);
      const float beta = pb.sel[(size_t)s * n + i];
      const float sel_prob = pm_sel_prob(alpha, beta, pb.prev[(size_t)s * n + i], P.prev_weight);
      float cos_tri, cos_inc;
      pm_viewing_angles(pose, point, curr_normal, &cos_tri, &cos_inc);
      const float tri_prob = pm_tri_prob(P, cos_tri);
      const float inc_prob = pm_inc_prob(P, cos_inc);
      float H[9];
      pm_compose_homography(pose, iK, row, col, curr_depth, curr_normal, H);
      const float res_prob = pm_resolution_prob(H, row, col, P.radius);
      pb.probs[(size_t)s * ncols + col] = sel_prob * tri_prob * inc_prob * res_prob;
    }
    {  // TransformPDFToCDF
      float prob_sum = 0.0f;
      for (int s = 0; s < S; ++s) prob_sum += pb.probs[(size_t)s * ncols + col];
      const float inv_prob_sum = 1.0f / prob_sum;
      float cum_prob = 0.0f;
      for (int s = 0; s < S; ++s) {
        const float prob = pb.probs[(size_t)s * ncols + col] * inv_prob_sum;
        cum_prob += prob;
        pb.probs[(size_t)s * ncols + col] = cum_prob;
      }
    }

    const int kNumCosts = 5;
    float costs[kNumCosts] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    const float depths[kNumCosts] = {curr_depth, prev_depth, rand_depth, curr_depth, rand_depth};
    const float* normals[kNumCosts] = {curr_normal, prev_normal, rand_normal, rand_normal, curr_normal};
    for (int sample = 0; sample < P.num_samples; ++sample) {
      const float rand_prob = rng.uniform() - 1.1920928955078125e-07f;  // FLT_EPSILON
      int src = -1;
      for (int s = 0; s < S; ++s) {
        if (pb.probs[(size_t)s * ncols + col] > rand_prob) {
          src = s;
          break;
        }
      }
      if (src == -1) continue;
      const float* pose = poses + (size_t)src * PM_POSE;
      const PmImage im = P.images[pb.src[src]];
      costs[0] += cost_map[(size_t)src * n + i];
      if (GEOM)
        costs[0] += P.geom_reg * pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, depths[0], P.geom_max_cost);
#pragma unroll 1
      for (int k = 1; k < kNumCosts; ++k) {
        costs[k] += pm_photo_cost(P, tile, pose, iK, P.pixels + im.px_off, (int)im.w, (int)im.h, row, col, PM_LANES + lane, depths[k], normals[k], ref_sum, ref_sq);
        if (GEOM)
          costs[k] += P.geom_reg * pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, depths[k], P.geom_max_cost);
      }
    }

    int min_cost_idx = 0;  // FindMinCost
    {
      float min_cost = costs[0];
      for (int k = 1; k < kNumCosts; ++k) {
        if (costs[k] <= min_cost) {
          min_cost = costs[k];
          min_cost_idx = k;
        }
      }
    }
    const float best_depth = depths[min_cost_idx];
    const float best_normal[3] = {normals[min_cost_idx][0], normals[min_cost_idx][1], normals[min_cost_idx][2]};
    depth_map[i] = best_depth;
    for (int k = 0; k < 3; ++k) normal_map[(size_t)k * n + i] = best_normal[k];

    for (int s = 0; s < S; ++s) {
      float cost;
      if (min_cost_idx == 0) {
        cost = cost_map[(size_t)s * n + i];
      } else {
        const PmImage im = P.images[pb.src[s]];
        cost = pm_photo_cost(P, tile, poses + (size_t)s * PM_POSE, iK, P.pixels + im.px_off, (int)im.w, (int)im.h, row, col, PM_LANES + lane, best_depth,
                             best_normal, ref_sum, ref_sq);
        cost_map[(size_t)s * n + i] = cost;
      }
      const float alpha = pm_forward_message(P, cost, pb.fwd[(size_t)s * ncols + col]);
      const float beta = pb.sel[(size_t)s * n + i];
      const float prob = pm_sel_prob(alpha, beta, pb.prev[(size_t)s * n + i], P.prev_weight);
      pb.fwd[(size_t)s * ncols + col] = alpha;
      pb.sel[(size_t)s * n + i] = prob;
    }

    if (FILTER) {
      int num_consistent = 0;
      float best_point[3];
      pm_point_at_depth(iK, row, col, best_depth, best_point);
      for (int s = 0; s < S; ++s) {
        const float* pose = poses + (size_t)s * PM_POSE;
        float cos_tri, cos_inc;
        pm_viewing_angles(pose, best_point, best_normal, &cos_tri, &cos_inc);
        if (cos_tri > P.filter_cos_min_tri || cos_inc <= 0.0f) continue;
        bool consistent = pb.sel[(size_t)s * n + i] >= P.filter_min_ncc_prob;
        if (FILTER == 2 && consistent) {
          const PmImage im = P.images[pb.src[s]];
          consistent = pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, best_depth, P.geom_max_cost) <=
                       P.filter_geom_max_cost;
        }
        if (consistent) {
          mask[(size_t)s * n + i] = 1;
          num_consistent += 1;
        }
      }
      if (num_consistent < P.filter_min_num_consistent) {
        depth_map[i] = 0.0f;
        for (int k = 0; k < 3; ++k) normal_map[(size_t)k * n + i] = 0.0f;
        for (int s = 0; s < S; ++s) mask[(size_t)s * n + i] = 0;
      }
    }

    prev_depth = best_depth;
    for (int k = 0; k < 3; ++k) prev_normal[k] = best_normal[k];
  }
}
#endif  // DSM_CHECK_BUILD

// ---- the product schedule: a wave per (problem, column) ----
// The reference's grid has a thread per column: 2 000 threads for a 2 000 pixel wide image, 31 waves on a chip that holds
// thousands.  Here a wave owns a column and spreads the work INSIDE a pixel over its lanes: the per-source-image priors (a
// lane per source image), the (sample, hypothesis) NCC items (a lane per item, 16 samples x 4 hypotheses per pass; every
// item's tap sums run in raster order inside its lane), the winner's costs (a lane per source image).  What the contract
// orders stays serial: the CDF over the source images (lane 0), the per-hypothesis sums over the samples (a lane per
// hypothesis, in sample order).  The scalars of the pixel (propagation, perturbation, the winner) are computed by every lane
// alike.  The backward messages are a kernel of their own over (problem, column, image).  Same device functions, same
// operations per value as k_pm_sweep: byte-identical results.
constexpr int PM_WAVES = PM_BLOCK / 64;   // columns of one block
constexpr int PM_WTILE_STRIDE = 68;       // bytes of a window row in LDS: 2 * PM_MAX_RADIUS + 1 columns, rounded up
constexpr int PM_CHUNK = 16;              // samples of one pass: 16 x 4 hypotheses = 64 items
constexpr int PM_WAVE_SCRATCH = 1024;     // bytes per wave behind its tile: items[64], geometric items[16][5], cost-0 items[16], sources[16], costs[5]

__global__ void __launch_bounds__(PM_BLOCK) k_pm_backward(PmParams P) {
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = (P.rot & 1) ? pb.h0 : pb.w0, h = (P.rot & 1) ? pb.w0 : pb.h0;
  const int ncols = pb.w0 > pb.h0 ? pb.w0 : pb.h0;
  const size_t idx = (size_t)blockIdx.x * PM_BLOCK + threadIdx.x;
  if (idx >= (size_t)w * pb.S) return;
  const int col = (int)(idx % w), s = (int)(idx / w);
  const size_t n = (size_t)w * h;
  const float* cost_map = pb.cost[P.cur];
  float beta = 0.5f;
  for (int row = h - 1; row >= 0; --row) {
    const size_t i = (size_t)s * n + (size_t)row * w + col;
    beta = pm_backward_message(P, cost_map[i], beta);
    pb.sel[i] = beta;
  }
  pb.fwd[(size_t)s * ncols + col] = 0.5f;
}

template <bool GEOM, int FILTER>
__global__ void __launch_bounds__(PM_BLOCK) k_pm_sweep_wave(PmParams P) {
  extern __shared__ float pm_smem[];
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = (P.rot & 1) ? pb.h0 : pb.w0, h = (P.rot & 1) ? pb.w0 : pb.h0;
  if ((int)blockIdx.x * PM_WAVES >= w) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int col = blockIdx.x * PM_WAVES + wave;
  const bool active = col < w;  // the same in every lane of a wave
  for (int k = threadIdx.x; k < 256; k += PM_BLOCK) {
    pm_smem[k] = P.tex[k];
    pm_smem[256 + k] = P.w_color[k];
  }
  const int radius = P.radius, window = 2 * radius + 1;
  const size_t tile_bytes = ((size_t)window * PM_WTILE_STRIDE + 15) & ~(size_t)15;
  uint8_t* wave_base = reinterpret_cast<uint8_t*>(pm_smem + 512) + (size_t)wave * (tile_bytes + PM_WAVE_SCRATCH);
  PmTile tile;
  tile.tex = pm_smem;
  tile.wcol = pm_smem + 256;
  tile.rows = wave_base;
  tile.window = window;
  tile.stride = PM_WTILE_STRIDE;
  float* items = reinterpret_cast<float*>(wave_base + tile_bytes);  // [PM_CHUNK][4]
  float* gitems = items + 4 * PM_CHUNK;                             // [PM_CHUNK][5]
  float* c0items = gitems + 5 * PM_CHUNK;                           // [PM_CHUNK]
  int* srcs = reinterpret_cast<int*>(c0items + PM_CHUNK);           // [PM_CHUNK]
  float* c5 = reinterpret_cast<float*>(srcs + PM_CHUNK);            // [5]

  const size_t n = (size_t)w * h;
  const int S = pb.S;
  const int ncols = pb.w0 > pb.h0 ? pb.w0 : pb.h0;
  const float* K = pb.K[P.rot];
  const float* iK = pb.iK[P.rot];
  const float* poses = pb.poses + (size_t)P.rot * S * PM_POSE;
  const uint8_t* ref = pb.ref_img[P.cur];
  float* depth_map = pb.depth[P.cur];
  float* normal_map = pb.normal[P.cur];
  float* cost_map = pb.cost[P.cur];
  uint8_t* mask = pb.mask[0];

  float prev_depth = 0.0f, prev_normal[3] = {0.0f, 0.0f, 0.0f};
  PmRand rng{P.seed, pb.key1, P.sweep_no, (uint32_t)col, 1u, 0u};
  if (active) {
    prev_depth = depth_map[col];
    for (int k = 0; k < 3; ++k) prev_normal[k] = normal_map[(size_t)k * n + col];
  }

  for (int row = 0; row < h; ++row) {
    const size_t i = (size_t)row * w + (active ? col : 0);
    __syncthreads();  // the tile row that leaves the ring and the scratch of the last row are no longer read
    if (active) {
      for (int r = (row == 0 ? -radius : row + radius); r <= row + radius; ++r) {
        uint8_t* dst = tile.rows + (size_t)((r + radius) % window) * PM_WTILE_STRIDE;
        for (int j = lane; j < window; j += 64) {
          const int c = col - radius + j;
          dst[j] = (r >= 0 && r < h && c >= 0 && c < w) ? ref[(size_t)r * w + c] : (uint8_t)0;
        }
      }
    }
    float ref_sum = 0.0f, ref_sq = 0.0f, curr_depth = 0.0f, rand_depth = 0.0f;
    float curr_normal[3] = {0.0f, 0.0f, 0.0f}, rand_normal[3] = {0.0f, 0.0f, 0.0f};
    if (active) {
      ref_sum = pb.sum[P.cur][i];
      ref_sq = pb.sq[P.cur][i];
      prev_depth = pm_propagate_depth(iK, prev_depth, prev_normal, row - 1, row);
      curr_depth = depth_map[i];
      for (int k = 0; k < 3; ++k) curr_normal[k] = normal_map[(size_t)k * n + i];
      const float dmin = (1.0f - P.perturbation) * curr_depth, dmax = (1.0f + P.perturbation) * curr_depth;
      rand_depth = rng.uniform() * (dmax - dmin) + dmin;
      pm_perturb_normal(iK, row, col, P.perturbation_normal, curr_normal, rng, rand_normal);
      float point[3];
      pm_point_at_depth(iK, row, col, curr_depth, point);
      for (int s = lane; s < S; s += 64) {  // the priors: a lane per source image
        const float* pose = poses + (size_t)s * PM_POSE;
        const float alpha = pm_forward_message(P, cost_map[(size_t)s * n + i], pb.fwd[(size_t)s * ncols + col]);
        const float sel_prob = pm_sel_prob(alpha, pb.sel[(size_t)s * n + i], pb.prev[(size_t)s * n + i], P.prev_weight);
        float cos_tri, cos_inc;
        pm_viewing_angles(pose, point, curr_normal, &cos_tri, &cos_inc);
        float H[9];
        pm_compose_homography(pose, iK, row, col, curr_depth, curr_normal, H);
        pb.probs[(size_t)s * ncols + col] = sel_prob * pm_tri_prob(P, cos_tri) * pm_inc_prob(P, cos_inc) * pm_resolution_prob(H, row, col, P.radius);
      }
    }
    __syncthreads();
    if (active && lane == 0) {  // TransformPDFToCDF: the order of the sums is the contract's
      float prob_sum = 0.0f;
      for (int s = 0; s < S; ++s) prob_sum += pb.probs[(size_t)s * ncols + col];
      const float inv_prob_sum = 1.0f / prob_sum;
      float cum_prob = 0.0f;
      for (int s = 0; s < S; ++s) {
        const float prob = pb.probs[(size_t)s * ncols + col] * inv_prob_sum;
        cum_prob += prob;
        pb.probs[(size_t)s * ncols + col] = cum_prob;
      }
    }
    __syncthreads();

    // the Monte Carlo samples: PM_CHUNK samples x 4 hypotheses per pass, lane = 4 * sample + hypothesis - 1
    float acc = 0.0f;  // lanes 0 .. 4: costs[lane]
    const uint32_t d0 = rng.d;
    for (int base = 0; base < P.num_samples; base += PM_CHUNK) {
      if (active) {
        const int jj = lane >> 2, j = base + jj, k = 1 + (lane & 3);
        int src = -1;
        float photo = 0.0f, g = 0.0f, c0 = 0.0f, g0 = 0.0f;
        if (j < P.num_samples) {
          const float rand_prob = rng.at(d0 + (uint32_t)j) - 1.1920928955078125e-07f;  // FLT_EPSILON
          for (int s = 0; s < S; ++s) {
            if (pb.probs[(size_t)s * ncols + col] > rand_prob) {
              src = s;
              break;
            }
          }
          if (src != -1) {
            const float* pose = poses + (size_t)src * PM_POSE;
            const PmImage im = P.images[pb.src[src]];
            const float depth_k = k == 1 ? prev_depth : ((k == 2 || k == 4) ? rand_depth : curr_depth);
            const float* normal_k = k == 1 ? prev_normal : ((k == 2 || k == 3) ? rand_normal : curr_normal);
            const float nk[3] = {normal_k[0], normal_k[1], normal_k[2]};
            photo = pm_photo_cost(P, tile, pose, iK, P.pixels + im.px_off, (int)im.w, (int)im.h, row, col, radius, depth_k, nk, ref_sum, ref_sq);
            if (GEOM) g = pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, depth_k, P.geom_max_cost);
            if (k == 1) {
              c0 = cost_map[(size_t)src * n + i];
              if (GEOM) g0 = pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, curr_depth, P.geom_max_cost);
            }
          }
        }
        items[lane] = photo;
        gitems[jj * 5 + k] = g;
        if (k == 1) {
          srcs[jj] = src;
          c0items[jj] = c0;
          gitems[jj * 5] = g0;
        }
      }
      __syncthreads();
      if (active && lane < 5) {  // costs[lane] over the samples of the pass, in sample order
        for (int jj = 0; jj < PM_CHUNK && base + jj < P.num_samples; ++jj) {
          if (srcs[jj] == -1) continue;
          acc += lane == 0 ? c0items[jj] : items[jj * 4 + lane - 1];
          if (GEOM) acc += P.geom_reg * gitems[jj * 5 + lane];
        }
      }
      __syncthreads();
    }
    rng.d = d0 + (uint32_t)P.num_samples;
    if (active && lane < 5) c5[lane] = acc;
    __syncthreads();
    if (!active) continue;

    int min_cost_idx = 0;  // FindMinCost
    {
      float min_cost = c5[0];
      for (int k = 1; k < 5; ++k) {
        if (c5[k] <= min_cost) {
          min_cost = c5[k];
          min_cost_idx = k;
        }
      }
    }
    const float best_depth = (min_cost_idx == 1) ? prev_depth : ((min_cost_idx == 2 || min_cost_idx == 4) ? rand_depth : curr_depth);
    const float* bn = (min_cost_idx == 1) ? prev_normal : ((min_cost_idx == 2 || min_cost_idx == 3) ? rand_normal : curr_normal);
    const float best_normal[3] = {bn[0], bn[1], bn[2]};
    if (lane == 0) {
      depth_map[i] = best_depth;
      for (int k = 0; k < 3; ++k) normal_map[(size_t)k * n + i] = best_normal[k];
    }

    int num_consistent = 0;
    float best_point[3];
    pm_point_at_depth(iK, row, col, best_depth, best_point);
    for (int s0 = 0; s0 < S; s0 += 64) {  // the winner's costs, messages and consistency: a lane per source image
      const int s = s0 + lane;
      bool consistent = false;
      if (s < S) {
        const float* pose = poses + (size_t)s * PM_POSE;
        float cost;
        if (min_cost_idx == 0) {
          cost = cost_map[(size_t)s * n + i];
        } else {
          const PmImage im = P.images[pb.src[s]];
          cost = pm_photo_cost(P, tile, pose, iK, P.pixels + im.px_off, (int)im.w, (int)im.h, row, col, radius, best_depth, best_normal, ref_sum, ref_sq);
          cost_map[(size_t)s * n + i] = cost;
        }
        const float alpha = pm_forward_message(P, cost, pb.fwd[(size_t)s * ncols + col]);
        const float prob = pm_sel_prob(alpha, pb.sel[(size_t)s * n + i], pb.prev[(size_t)s * n + i], P.prev_weight);
        pb.fwd[(size_t)s * ncols + col] = alpha;
        pb.sel[(size_t)s * n + i] = prob;
        if (FILTER) {
          float cos_tri, cos_inc;
          pm_viewing_angles(pose, best_point, best_normal, &cos_tri, &cos_inc);
          if (!(cos_tri > P.filter_cos_min_tri || cos_inc <= 0.0f)) {
            consistent = prob >= P.filter_min_ncc_prob;
            if (FILTER == 2 && consistent) {
              const PmImage im = P.images[pb.src[s]];
              consistent = pm_geom_cost(pose, K, iK, P.depths + im.depth_off, (int)im.w, (int)im.h, row, col, best_depth, P.geom_max_cost) <=
                           P.filter_geom_max_cost;
            }
          }
          if (consistent) mask[(size_t)s * n + i] = 1;
        }
      }
      if (FILTER) num_consistent += __popcll(__ballot(consistent));
    }
    if (FILTER && num_consistent < P.filter_min_num_consistent) {
      if (lane == 0) {
        depth_map[i] = 0.0f;
        for (int k = 0; k < 3; ++k) normal_map[(size_t)k * n + i] = 0.0f;
      }
      for (int s = lane; s < S; s += 64) mask[(size_t)s * n + i] = 0;
    }
    prev_depth = best_depth;
    for (int k = 0; k < 3; ++k) prev_normal[k] = best_normal[k];
  }
}

// every map of the problem a quarter turn counter-clockwise: out[(w - 1 - x) * h + y] = in[y * w + x]; with_mask: the
// consistency mask as well (after the last sweep with the filter)
__global__ void __launch_bounds__(PM_BLOCK) k_pm_rotate(PmParams P, int with_mask) {
  const PmProb& pb = P.probs[blockIdx.y];
  const int w = (P.rot & 1) ? pb.h0 : pb.w0, h = (P.rot & 1) ? pb.w0 : pb.h0;
  const int i = blockIdx.x * PM_BLOCK + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i % w;
  const size_t n = (size_t)w * h;
  const size_t o = (size_t)(w - 1 - x) * h + y;
  const int a = P.cur, b = P.cur ^ 1;
  pb.depth[b][o] = pb.depth[a][i];
  const float n0 = pb.normal[a][i], n1 = pb.normal[a][n + i], n2 = pb.normal[a][2 * n + i];
  pb.normal[b][o] = n1;  // RotateNormalMap
  pb.normal[b][n + o] = -n0;
  pb.normal[b][2 * n + o] = n2;
  pb.ref_img[b][o] = pb.ref_img[a][i];
  pb.sum[b][o] = pb.sum[a][i];
  pb.sq[b][o] = pb.sq[a][i];
  for (int s = 0; s < pb.S; ++s) {
    pb.prev[(size_t)s * n + o] = pb.sel[(size_t)s * n + i];
    pb.cost[b][(size_t)s * n + o] = pb.cost[a][(size_t)s * n + i];
    if (with_mask) pb.mask[1][(size_t)s * n + o] = pb.mask[0][(size_t)s * n + i];
  }
}

// ---- the host: InitTransforms ----
void mat33_mul(const float* A, const float* B, float* C) {  // each element summed left to right
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) C[3 * r + c] = A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c] + A[3 * r + 2] * B[6 + c];
}
void mat33_vec(const float* A, const float* v, float* out) {
  for (int r = 0; r < 3; ++r) out[r] = A[3 * r] * v[0] + A[3 * r + 1] * v[1] + A[3 * r + 2] * v[2];
}
void transpose33(const float* A, float* At) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) At[3 * c + r] = A[3 * r + c];
}

// one source image's PM_POSE floats against the (rotated) reference pose R1, T1: mvs/image.cc:92-130.  inv_P is the inverse of
// [P; 0 0 0 1] evaluated in double from the float P by the adjugate of its left 3 x 3 block, rounded to float (Eigen's 4 x 4
// float inverse is SSE cofactor code whose order no other compiler shares).
void compose_pose(const float* R1, const float* T1, const dsm_mvs_image& im, float* out) {
  out[0] = im.K[0];
  out[1] = im.K[2];
  out[2] = im.K[4];
  out[3] = im.K[5];
  float R1t[9], rel_R[9], rel_T[3], tmp[3];
  transpose33(R1, R1t);
  mat33_mul(im.R, R1t, rel_R);  // ComputeRelativePose
  mat33_vec(rel_R, T1, tmp);
  for (int k = 0; k < 3; ++k) rel_T[k] = im.T[k] - tmp[k];
  memcpy(out + 4, rel_R, sizeof(rel_R));
  memcpy(out + 13, rel_T, sizeof(rel_T));
  float Rt[9], C[3];  // ComputeProjectionCenter
  transpose33(rel_R, Rt);
  mat33_vec(Rt, rel_T, C);
  for (int k = 0; k < 3; ++k) out[16 + k] = -C[k];
  float KR[9], KT[3], Pm[12];  // ComposeProjectionMatrix
  mat33_mul(im.K, rel_R, KR);
  mat33_vec(im.K, rel_T, KT);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Pm[4 * r + c] = KR[3 * r + c];
    Pm[4 * r + 3] = KT[r];
  }
  memcpy(out + 19, Pm, sizeof(Pm));
  const double m00 = Pm[0], m01 = Pm[1], m02 = Pm[2], m10 = Pm[4], m11 = Pm[5], m12 = Pm[6], m20 = Pm[8], m21 = Pm[9], m22 = Pm[10];
  const double t0 = Pm[3], t1 = Pm[7], t2 = Pm[11];
  const double c00 = m11 * m22 - m12 * m21, c01 = m12 * m20 - m10 * m22, c02 = m10 * m21 - m11 * m20;
  const double det = m00 * c00 + m01 * c01 + m02 * c02;
  const double inv[9] = {c00 / det, (m02 * m21 - m01 * m22) / det, (m01 * m12 - m02 * m11) / det,
                         c01 / det, (m00 * m22 - m02 * m20) / det, (m02 * m10 - m00 * m12) / det,
                         c02 / det, (m01 * m20 - m00 * m21) / det, (m00 * m11 - m01 * m10) / det};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[31 + 4 * r + c] = (float)inv[3 * r + c];
    out[31 + 4 * r + 3] = (float)(-(inv[3 * r] * t0 + inv[3 * r + 1] * t1 + inv[3 * r + 2] * t2));
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the device bytes of one problem's maps and tables
size_t problem_bytes(uint64_t w, uint64_t h, uint64_t S) {
  const uint64_t n = w * h, m = std::max(w, h);
  size_t b = 0;
  b += 2 * align256(n);                 // ref_img, both buffers of the rotation
  b += 6 * align256(n * 4);             // sum, sq, depth
  b += 2 * align256(3 * n * 4);         // normal
  b += 2 * align256(S * n * 4);         // cost
  b += 2 * align256(S * n);             // mask
  b += 2 * align256(S * n * 4);         // sel, prev
  b += 2 * align256(S * m * 4);         // fwd, probs
  b += align256(4 * S * PM_POSE * 4);   // poses
  b += align256(S * 4);                 // src
  return b;
}

struct Carver {
  uint8_t* base;
  size_t off;
  template <typename T>
  T* take(size_t count) {
    T* p = reinterpret_cast<T*>(base + off);
    off += align256(count * sizeof(T));
    return p;
  }
};

}  // namespace

extern "C" void dsm_default_patch_match_options(dsm_patch_match_options* o) {  // patch_match.h:59-139
  memset(o, 0, sizeof(*o));
  o->window_radius = 5;
  o->window_step = 1;
  o->num_samples = 15;
  o->num_iterations = 5;
  o->geom_consistency = 1;
  o->filter = 1;
  o->filter_min_num_consistent = 2;
  o->seed = 0;
  o->sigma_spatial = -1;
  o->sigma_color = 0.2f;
  o->ncc_sigma = 0.6f;
  o->min_triangulation_angle = 1.0f;
  o->incident_angle_sigma = 0.9f;
  o->geom_consistency_regularizer = 0.3f;
  o->geom_consistency_max_cost = 3.0f;
  o->filter_min_ncc = 0.1f;
  o->filter_min_triangulation_angle = 3.0f;
  o->filter_geom_consistency_max_cost = 1.0f;
}

extern "C" int dsm_patch_match(dsm_ctx* ctx, const dsm_patch_match_options* options, uint32_t n_images, const dsm_mvs_image* images,
                               uint32_t n_problems, const uint32_t* ref_image, const uint64_t* src_offsets, const uint32_t* src_images,
                               const float* depth_min, const float* depth_max, float* const* out_depth, float* const* out_normal,
                               float* const* out_sel_prob, uint8_t* const* out_mask) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_patch_match", msg); };
  dsm_patch_match_options o;
  if (options)
    o = *options;
  else
    dsm_default_patch_match_options(&o);
  // PatchMatchOptions::Check, patch_match.h:141-168 (written so that a NaN fails them)
  if (!(o.window_radius > 0)) return fail("window_radius <= 0");
  if (!(o.window_radius <= PM_MAX_RADIUS)) return fail("window_radius > 32");
  if (!(o.window_step > 0)) return fail("window_step <= 0");
  if (!(o.window_step <= 2)) return fail("window_step > 2");
  if (!(o.sigma_color > 0.0)) return fail("sigma_color <= 0");
  if (!(o.num_samples > 0)) return fail("num_samples <= 0");
  if (!(o.ncc_sigma > 0.0)) return fail("ncc_sigma <= 0");
  if (!(o.min_triangulation_angle >= 0.0)) return fail("min_triangulation_angle < 0");
  if (!(o.min_triangulation_angle < 180.0)) return fail("min_triangulation_angle >= 180");
  if (!(o.incident_angle_sigma > 0.0)) return fail("incident_angle_sigma <= 0");
  if (!(o.num_iterations > 0)) return fail("num_iterations <= 0");
  if (!(o.geom_consistency_regularizer >= 0.0)) return fail("geom_consistency_regularizer < 0");
  if (!(o.geom_consistency_max_cost >= 0.0)) return fail("geom_consistency_max_cost < 0");
  if (!(o.filter_min_ncc >= -1.0)) return fail("filter_min_ncc < -1");
  if (!(o.filter_min_ncc <= 1.0)) return fail("filter_min_ncc > 1");
  if (!(o.filter_min_triangulation_angle >= 0.0)) return fail("filter_min_triangulation_angle < 0");
  if (!(o.filter_min_triangulation_angle <= 180.0)) return fail("filter_min_triangulation_angle > 180");
  if (!(o.filter_min_num_consistent >= 0)) return fail("filter_min_num_consistent < 0");
  if (!(o.filter_geom_consistency_max_cost >= 0.0)) return fail("filter_geom_consistency_max_cost < 0");
  if (o.sigma_spatial != o.sigma_spatial) return fail("sigma_spatial is NaN");
  if (o.num_iterations > 4096) return fail("num_iterations > 4096");
  if (n_problems && (!ref_image || !src_offsets || !depth_min || !depth_max || !out_depth || !out_normal)) return fail("NULL argument");
  if (n_images && !images) return fail("NULL argument");
  const bool geom = o.geom_consistency != 0, filter = o.filter != 0;
  if (n_problems && filter && !out_mask) return fail("filter without out_mask");
  for (uint32_t i = 0; i < n_images; ++i) {
    const dsm_mvs_image& im = images[i];
    if (!im.data) return fail("an image without data");
    if (im.width == 0 || im.height == 0 || im.width > PM_MAX_SIDE || im.height > PM_MAX_SIDE)
      return fail("an image without pixels, or with a side above 32768");
    if (im.row_stride < im.width) return fail("row_stride below width");
  }
  for (uint32_t p = 0; p < n_problems; ++p) {
    if (ref_image[p] >= n_images) return fail("a reference image index out of range");
    if (src_offsets[p] > src_offsets[p + 1]) return fail("src_offsets must not decrease");
    if (src_offsets[p + 1] - src_offsets[p] > 65535) return fail("more than 65535 source images in one problem");
    if (src_offsets[p + 1] > src_offsets[p] && !src_images) return fail("NULL argument");
    if (!(depth_min[p] > 0.0f)) return fail("depth_min <= 0");
    if (!(depth_min[p] <= depth_max[p])) return fail("depth_min > depth_max");
    if (!out_depth[p] || !out_normal[p] || (filter && !out_mask[p])) return fail("NULL output pointer");
    if (geom && (!images[ref_image[p]].depth_map || !images[ref_image[p]].normal_map))
      return fail("geom_consistency without the depth and normal map of a reference image");
    for (uint64_t k = src_offsets[p]; k < src_offsets[p + 1]; ++k) {
      if (src_images[k] >= n_images) return fail("a source image index out of range");
      if (geom && !images[src_images[k]].depth_map) return fail("geom_consistency without the depth map of a source image");
    }
  }
  auto mark = [&]() {
    if (!ctx->patch_match_ready) ctx->patch_match_ready = true;
  };
  double ms[DSM_PATCH_MATCH_STAGES] = {0, 0, 0, 0, 0, 0};
  if (!n_problems) {
    mark();
    memcpy(ctx->patch_match_ms, ms, sizeof(ms));
    return DSM_OK;
  }

  // ---- the constants of the call (computed once, on the host) ----
  const int radius = o.window_radius, step = o.window_step;
  const float sigma_spatial = o.sigma_spatial <= 0.0 ? (float)radius : (float)o.sigma_spatial;
  const float sigma_color = (float)o.sigma_color;
  const float ncc_sigma = (float)o.ncc_sigma;
  const float incident_angle_sigma = (float)o.incident_angle_sigma;
  const float min_tri_rad = (float)(o.min_triangulation_angle * 0.0174532925199432);
  const float filter_tri_rad = (float)(o.filter_min_triangulation_angle * 0.0174532925199432);
  const float filter_min_ncc = (float)o.filter_min_ncc;
  std::vector<float> tables;
  {
    const float spatial_normalization = 1.0f / (2.0f * sigma_spatial * sigma_spatial);
    const float color_normalization = 1.0f / (2.0f * sigma_color * sigma_color);
    for (int wr = -radius; wr <= radius; wr += step)
      for (int wc = -radius; wc <= radius; wc += step) {
        const float d2 = (float)(wr * wr + wc * wc);
        tables.push_back((float)std::exp((double)(-d2 * spatial_normalization)));
      }
    const size_t taps = tables.size();
    tables.resize(align256(taps * 4) / 4, 0.0f);
    for (int k = 0; k < 256; ++k) {
      const float cd = (float)k / 255.0f;
      tables.push_back((float)std::exp((double)(-(cd * cd) * color_normalization)));
    }
    for (int k = 0; k < 256; ++k) tables.push_back((float)k / 255.0f);
  }
  const size_t taps_floats = tables.size() - 512;

  PmParams P;
  memset(&P, 0, sizeof(P));
  P.radius = radius;
  P.step = step;
  P.num_samples = o.num_samples;
  P.filter_min_num_consistent = o.filter_min_num_consistent;
  P.seed = o.seed;
  P.cos_min_tri = (float)std::cos((double)min_tri_rad);
  P.inv_inc_sigma_sq = -0.5f / (incident_angle_sigma * incident_angle_sigma);
  P.inv_ncc_sigma_sq = -0.5f / (ncc_sigma * ncc_sigma);
  {
    const float erf_arg = 2.0f / (ncc_sigma * 1.414213562f);
    const float erf_val = (float)std::erf((double)erf_arg);
    P.ncc_norm = (float)(2.0 / (std::sqrt(2.0 * M_PI) * (double)ncc_sigma * (double)erf_val));
  }
  P.geom_reg = (float)o.geom_consistency_regularizer;
  P.geom_max_cost = (float)o.geom_consistency_max_cost;
  {
    const float c = 1.0f - filter_min_ncc;
    P.filter_min_ncc_prob = (float)dsm_exp((double)(c * c * P.inv_ncc_sigma_sq)) * P.ncc_norm;
  }
  P.filter_cos_min_tri = (float)std::cos((double)filter_tri_rad);
  P.filter_geom_max_cost = (float)o.filter_geom_consistency_max_cost;

  // ---- the resident part: the image table, the pixels, the depth maps, the tables ----
  std::vector<PmImage> himg(std::max<uint32_t>(n_images, 1));
  uint64_t px_bytes = 0, depth_floats = 0;
  for (uint32_t i = 0; i < n_images; ++i) {
    himg[i].w = images[i].width;
    himg[i].h = images[i].height;
    himg[i].px_off = px_bytes;
    px_bytes += align256((uint64_t)images[i].width * images[i].height);
    himg[i].depth_off = depth_floats;
    if (geom && images[i].depth_map) depth_floats += align256((uint64_t)images[i].width * images[i].height * 4) / 4;
  }
  const size_t fixed_bytes = align256(himg.size() * sizeof(PmImage)) + align256(px_bytes + 16) + align256(depth_floats * 4 + 16) + align256(tables.size() * 4);

  // ---- chunks of consecutive problems under the budget ----
  const uint64_t budget = ctx->memory_budget ? ctx->memory_budget : PM_DEFAULT_CHUNK_BYTES;
  std::vector<uint32_t> chunk_begin;
  size_t max_chunk_bytes = 0;
  uint32_t max_chunk_problems = 0;
  {
    size_t acc = 0;
    uint32_t first = 0;
    chunk_begin.push_back(0);
    for (uint32_t p = 0; p < n_problems; ++p) {
      const dsm_mvs_image& im = images[ref_image[p]];
      const size_t b = problem_bytes(im.width, im.height, src_offsets[p + 1] - src_offsets[p]) + align256(sizeof(PmProb));
      if (p > first && acc + b > budget) {
        chunk_begin.push_back(p);
        first = p;
        acc = 0;
      }
      acc += b;
      max_chunk_bytes = std::max(max_chunk_bytes, acc);
      max_chunk_problems = std::max(max_chunk_problems, p - first + 1);
    }
    chunk_begin.push_back(n_problems);
  }

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, ctx->d_pm.reserve(fixed_bytes + max_chunk_bytes + align256((size_t)max_chunk_problems * sizeof(PmProb)) + 4096));
  Carver fixed{ctx->d_pm.as<uint8_t>(), 0};
  PmImage* d_images = fixed.take<PmImage>(himg.size());
  uint8_t* d_pixels = fixed.take<uint8_t>(px_bytes + 16);
  float* d_depths = fixed.take<float>(depth_floats + 4);
  float* d_tables = fixed.take<float>(tables.size());
  P.images = d_images;
  P.pixels = d_pixels;
  P.depths = d_depths;
  P.w_spatial = d_tables;
  P.w_color = d_tables + taps_floats;
  P.tex = d_tables + taps_floats + 256;

  const int total_sweeps = 4 * o.num_iterations;
  DevEventList ev(5 + 2 * (size_t)total_sweeps);
  HIPCHK(ctx, ev.create());

  bool resident_uploaded = false;
  const size_t smem = 2048 + (size_t)(2 * radius + 1) * 3 * PM_LANES;
  const size_t wave_smem = 2048 + (size_t)PM_WAVES * ((((size_t)(2 * radius + 1) * PM_WTILE_STRIDE + 15) & ~(size_t)15) + PM_WAVE_SCRATCH);
#ifdef DSM_CHECK_BUILD
  const bool lane_schedule = ctx->dbg("DSM_PATCH_MATCH_LANES") != nullptr && std::string(ctx->dbg("DSM_PATCH_MATCH_LANES")) != "0";
#endif
  for (size_t ci = 0; ci + 1 < chunk_begin.size(); ++ci) {
    const uint32_t p0 = chunk_begin[ci], p1 = chunk_begin[ci + 1], np = p1 - p0;
    Carver cv{ctx->d_pm.as<uint8_t>(), fixed.off};
    PmProb* d_probs = cv.take<PmProb>(np);
    std::vector<PmProb> hp(np);
    std::vector<std::vector<float>> hposes(np);
    uint32_t max_px = 0, max_cols = 0;
    uint64_t max_col_sources = 0;
    for (uint32_t q = 0; q < np; ++q) {
      const uint32_t p = p0 + q;
      const dsm_mvs_image& rim = images[ref_image[p]];
      PmProb& b = hp[q];
      memset(&b, 0, sizeof(b));
      b.w0 = (int32_t)rim.width;
      b.h0 = (int32_t)rim.height;
      b.S = (int32_t)(src_offsets[p + 1] - src_offsets[p]);
      b.ref = (int32_t)ref_image[p];
      b.dmin = depth_min[p];
      b.dmax = depth_max[p];
      b.key1 = ref_image[p];
      const size_t n = (size_t)rim.width * rim.height, S = (size_t)b.S, m = std::max(rim.width, rim.height);
      max_px = std::max<uint32_t>(max_px, (uint32_t)n);
      max_cols = std::max<uint32_t>(max_cols, (uint32_t)m);
      max_col_sources = std::max<uint64_t>(max_col_sources, (uint64_t)m * S);
      for (int k = 0; k < 2; ++k) {
        b.ref_img[k] = cv.take<uint8_t>(n);
        b.sum[k] = cv.take<float>(n);
        b.sq[k] = cv.take<float>(n);
        b.depth[k] = cv.take<float>(n);
        b.normal[k] = cv.take<float>(3 * n);
        b.cost[k] = cv.take<float>(S * n);
        b.mask[k] = cv.take<uint8_t>(S * n);
      }
      b.sel = cv.take<float>(S * n);
      b.prev = cv.take<float>(S * n);
      b.fwd = cv.take<float>(S * m);
      b.probs = cv.take<float>(S * m);
      float* d_poses = cv.take<float>(4 * S * PM_POSE);
      uint32_t* d_src = cv.take<uint32_t>(S);
      b.poses = d_poses;
      b.src = d_src;

      // InitTransforms :1500-1608: the four rotated calibrations and poses
      float Kr[4][4];
      for (int r = 0; r < 4; ++r) {
        Kr[r][0] = rim.K[0];
        Kr[r][1] = rim.K[2];
        Kr[r][2] = rim.K[4];
        Kr[r][3] = rim.K[5];
      }
      const float wm1 = (float)(rim.width - 1), hm1 = (float)(rim.height - 1);
      std::swap(Kr[1][0], Kr[1][2]);
      std::swap(Kr[1][1], Kr[1][3]);
      Kr[1][3] = wm1 - Kr[1][3];
      Kr[2][1] = wm1 - Kr[2][1];
      Kr[2][3] = hm1 - Kr[2][3];
      std::swap(Kr[3][0], Kr[3][2]);
      std::swap(Kr[3][1], Kr[3][3]);
      Kr[3][1] = hm1 - Kr[3][1];
      for (int r = 0; r < 4; ++r) {
        for (int k = 0; k < 4; ++k) b.K[r][k] = Kr[r][k];
        b.iK[r][0] = 1.0f / Kr[r][0];
        b.iK[r][1] = -Kr[r][1] / Kr[r][0];
        b.iK[r][2] = 1.0f / Kr[r][2];
        b.iK[r][3] = -Kr[r][3] / Kr[r][2];
      }
      float rotated_R[9], rotated_T[3];
      memcpy(rotated_R, rim.R, sizeof(rotated_R));
      memcpy(rotated_T, rim.T, sizeof(rotated_T));
      const float R_z90[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
      std::vector<float>& poses = hposes[q];
      poses.resize(4 * S * PM_POSE);
      for (int r = 0; r < 4; ++r) {
        for (size_t s = 0; s < S; ++s) compose_pose(rotated_R, rotated_T, images[src_images[src_offsets[p] + s]], &poses[(r * S + s) * PM_POSE]);
        float nR[9], nT[3];  // RotatePose
        mat33_mul(R_z90, rotated_R, nR);
        mat33_vec(R_z90, rotated_T, nT);
        memcpy(rotated_R, nR, sizeof(nR));
        memcpy(rotated_T, nT, sizeof(nT));
      }
      if (S) {
        HIPCHK(ctx, hipMemcpyAsync(d_poses, poses.data(), poses.size() * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(d_src, src_images + src_offsets[p], S * 4, hipMemcpyHostToDevice, st));
      }
    }
    P.probs = d_probs;

    size_t e = 0;
    HIPCHK(ctx, hipEventRecord(ev[e++], st));
    if (!resident_uploaded) {
      HIPCHK(ctx, hipMemcpyAsync(d_images, himg.data(), himg.size() * sizeof(PmImage), hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipMemcpyAsync(d_tables, tables.data(), tables.size() * 4, hipMemcpyHostToDevice, st));
      for (uint32_t i = 0; i < n_images; ++i) {
        HIPCHK(ctx, hipMemcpy2DAsync(d_pixels + himg[i].px_off, himg[i].w, images[i].data, images[i].row_stride, himg[i].w, himg[i].h,
                                     hipMemcpyHostToDevice, st));
        if (geom && images[i].depth_map)
          HIPCHK(ctx, hipMemcpyAsync(d_depths + himg[i].depth_off, images[i].depth_map, (size_t)himg[i].w * himg[i].h * 4, hipMemcpyHostToDevice, st));
      }
      resident_uploaded = true;
    }
    HIPCHK(ctx, hipMemcpyAsync(d_probs, hp.data(), (size_t)np * sizeof(PmProb), hipMemcpyHostToDevice, st));
    if (geom)
      for (uint32_t q = 0; q < np; ++q) {
        const dsm_mvs_image& rim = images[ref_image[p0 + q]];
        const size_t n = (size_t)rim.width * rim.height;
        HIPCHK(ctx, hipMemcpyAsync(hp[q].depth[0], rim.depth_map, n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(hp[q].normal[0], rim.normal_map, 3 * n * 4, hipMemcpyHostToDevice, st));
      }
    HIPCHK(ctx, hipEventRecord(ev[e++], st));

    const dim3 px_grid((max_px + PM_BLOCK - 1) / PM_BLOCK, np), col_grid((max_cols + PM_LANES - 1) / PM_LANES, np);
    const dim3 wave_grid((max_cols + PM_WAVES - 1) / PM_WAVES, np);
    P.rot = 0;
    P.cur = 0;
    hipLaunchKernelGGL(k_pm_filter, px_grid, dim3(PM_BLOCK), 0, st, P);
    if (geom)
      hipLaunchKernelGGL(k_pm_init<false>, px_grid, dim3(PM_BLOCK), 0, st, P);
    else
      hipLaunchKernelGGL(k_pm_init<true>, px_grid, dim3(PM_BLOCK), 0, st, P);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[e++], st));
    hipLaunchKernelGGL(k_pm_initial_cost, col_grid, dim3(PM_LANES), smem, st, P);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[e++], st));

    // RunWithWindowSizeAndStep :1283-1368
    const float total_num_steps = (float)(o.num_iterations * 4);
    for (int iter = 0; iter < o.num_iterations; ++iter) {
      for (int sweep = 0; sweep < 4; ++sweep) {
        const float exponent = (float)iter + (float)sweep / 4.0f;
        P.perturbation = 1.0f / (float)std::pow(2.0, (double)exponent);
        P.perturbation_normal = (float)((double)P.perturbation * M_PI);
        P.prev_weight = (float)(iter * 4 + sweep) / total_num_steps;
        P.sweep_no = (uint32_t)(iter * 4 + sweep);
        const bool last_sweep = iter == o.num_iterations - 1 && sweep == 3;
        const bool with_mask = last_sweep && filter;
        if (with_mask)
          for (uint32_t q = 0; q < np; ++q) {
            const size_t bytes = (size_t)hp[q].S * hp[q].w0 * hp[q].h0;
            if (bytes) HIPCHK(ctx, hipMemsetAsync(hp[q].mask[0], 0, bytes, st));
          }
#ifdef DSM_CHECK_BUILD
        if (lane_schedule) {
          if (geom) {
            if (with_mask)
              hipLaunchKernelGGL((k_pm_sweep<true, 2>), col_grid, dim3(PM_LANES), smem, st, P);
            else
              hipLaunchKernelGGL((k_pm_sweep<true, 0>), col_grid, dim3(PM_LANES), smem, st, P);
          } else {
            if (with_mask)
              hipLaunchKernelGGL((k_pm_sweep<false, 1>), col_grid, dim3(PM_LANES), smem, st, P);
            else
              hipLaunchKernelGGL((k_pm_sweep<false, 0>), col_grid, dim3(PM_LANES), smem, st, P);
          }
        } else
#endif
        {
          if (max_col_sources) hipLaunchKernelGGL(k_pm_backward, dim3((uint32_t)((max_col_sources + PM_BLOCK - 1) / PM_BLOCK), np), dim3(PM_BLOCK), 0, st, P);
          if (geom) {
            if (with_mask)
              hipLaunchKernelGGL((k_pm_sweep_wave<true, 2>), wave_grid, dim3(PM_BLOCK), wave_smem, st, P);
            else
              hipLaunchKernelGGL((k_pm_sweep_wave<true, 0>), wave_grid, dim3(PM_BLOCK), wave_smem, st, P);
          } else {
            if (with_mask)
              hipLaunchKernelGGL((k_pm_sweep_wave<false, 1>), wave_grid, dim3(PM_BLOCK), wave_smem, st, P);
            else
              hipLaunchKernelGGL((k_pm_sweep_wave<false, 0>), wave_grid, dim3(PM_BLOCK), wave_smem, st, P);
          }
        }
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[e++], st));
        hipLaunchKernelGGL(k_pm_rotate, px_grid, dim3(PM_BLOCK), 0, st, P, with_mask ? 1 : 0);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[e++], st));
        P.rot = (P.rot + 1) & 3;
        P.cur ^= 1;
      }
    }
    // 4 * num_iterations quarter turns: the original frame again, in buffer 0
    for (uint32_t q = 0; q < np; ++q) {
      const uint32_t p = p0 + q;
      const size_t n = (size_t)hp[q].w0 * hp[q].h0, S = (size_t)hp[q].S;
      HIPCHK(ctx, hipMemcpyAsync(out_depth[p], hp[q].depth[0], n * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(out_normal[p], hp[q].normal[0], 3 * n * 4, hipMemcpyDeviceToHost, st));
      if (S && out_sel_prob && out_sel_prob[p]) HIPCHK(ctx, hipMemcpyAsync(out_sel_prob[p], hp[q].prev, S * n * 4, hipMemcpyDeviceToHost, st));
      if (S && filter) HIPCHK(ctx, hipMemcpyAsync(out_mask[p], hp[q].mask[1], S * n, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(ev[e++], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (size_t k = 0; k + 1 < e; ++k) {
      double t = 0;
      HIPCHK(ctx, ev.ms(k, k + 1, &t));
      int stage;
      if (k < 3)
        stage = (int)k;
      else if (k + 2 == e)
        stage = 5;
      else
        stage = ((k - 3) & 1) ? 4 : 3;
      ms[stage] += t;
    }
  }
  mark();
  memcpy(ctx->patch_match_ms, ms, sizeof(ms));
  return DSM_OK;
}

extern "C" int dsm_get_patch_match_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->patch_match_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_patch_match_time: no dsm_patch_match call yet");
  memcpy(stage_ms, ctx->patch_match_ms, sizeof(ctx->patch_match_ms));
  return DSM_OK;
}
