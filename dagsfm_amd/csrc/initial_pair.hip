// initial_pair.hip -- the initial image pair of a batch of reconstructions on the device.
//   IncrementalMapper::FindInitialImagePair / FindFirstInitialImage / FindSecondInitialImage   src/sfm/incremental_mapper.cc:146-200, 791-930
//   IncrementalMapper::EstimateInitialTwoViewGeometry                                          :1121-1176
//   TwoViewGeometry::EstimateCalibrated / EstimateRelativePose                                  src/estimators/two_view_geometry.cc:292-380, 169-230
//   IncrementalMapper::RegisterInitialImagePair (the triangulation)                             :289-339
//   CalculateTriangulationAngles / CalculateTriangulationAngle, Median                          src/base/triangulation.cc:122-181, src/util/math.h:211-229
// The search is sequential in the reference: candidate after candidate until one passes.  Here every problem's candidate list is
// built first (the duplicate rule's counts per pair, k_ip_sums, k_ip_slot_rank, k_ip_entry_keys, k_ip_entry_rank: a candidate's
// place in its problem's list is the number of kept directed entries of the problem with a smaller packed key), then rounds
// speculate: every unfinished problem contributes its next speculation_window candidates, their oriented sorted match lists are
// gathered (k_ip_gather), the whole batch goes through the verifier on the leaf context (dsm_verify_on_leaf: the verifier's
// kernels, a fresh generator stream per candidate), k_ip_relative_pose decides every candidate, and the host replays the
// reference's order: the first accepted candidate of a problem wins, the candidates behind it were speculated.  The winners are
// triangulated at the end (k_ip_triangulate).  No floating-point atomics; every result is the same bytes for any window, any
// batch and any memory budget.  The check build has the reference's nested loops, a window of 1 and one lane per kernel as well
// (DSM_INITIAL_PAIR_SERIAL).
#include <hip/hip_runtime.h>
#include <math.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "ctx.h"
#include "rt_dedup.h"
#include "verify_camera.h"
#include "verify_linalg.h"

#define IP_HD static __host__ __device__ inline
#define IP_D static __device__ inline
#include "initial_pair.h"
#include "wave_reduce.h"

namespace {

constexpr int IP_BLOCK = 256;
constexpr uint32_t IP_NONE = 0xffffffffu;

// ------------------------------------------------------------------ counts and the candidate order
__global__ void k_ip_pair_count(uint32_t n_pairs, const uint64_t* __restrict__ moff, const uint8_t* __restrict__ acc, uint32_t* __restrict__ cnt) {
  __shared__ uint32_t sh[IP_BLOCK];
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  uint32_t c = 0;
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x) c += acc[m];
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int d = IP_BLOCK / 2; d > 0; d /= 2) {
    if ((int)threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[k] = sh[0];
}

struct IpOrder {
  IpOrderView v;
  uint32_t n_slots, n_entries;
  const uint32_t* slot_prob;  // [slots]
  const uint32_t* ent_prob;   // [entries]
  uint32_t* sum;              // [slots] NumCorrespondences inside the problem
  uint32_t* slot_rank;        // [slots] the place among the problem's slots in FindFirstInitialImage's order
  uint64_t* key;              // [2 entries] the packed key of a directed entry, IP_KEY_NONE for none
  uint32_t* cand;             // [2 entries] problem p's candidates from 2 ent_off[p]: 2 * entry + direction
  uint32_t* cand_n;           // [problems]
  uint8_t* seen;              // [entries] (the serial form)
};

// an image's NumCorrespondences inside its problem (integer atomics: the sums do not depend on their order)
__global__ void k_ip_sums(IpOrder o) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= o.n_entries) return;
  const uint32_t c = o.v.pair_cnt[o.v.ent_pair[e]];
  atomicAdd(&o.sum[o.v.ent_slot[2 * e]], c);
  atomicAdd(&o.sum[o.v.ent_slot[2 * e + 1]], c);
}

__global__ void k_ip_slot_rank(IpOrder o) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= o.n_slots) return;
  const uint32_t p = o.slot_prob[s];
  const uint64_t mine = ip_first_key(o.v.slot_flags[s], o.sum[s], s);
  uint32_t r = 0;
  for (uint32_t t = o.v.slot_off[p]; t < o.v.slot_off[p + 1]; ++t) r += ip_first_key(o.v.slot_flags[t], o.sum[t], t) < mine;
  o.slot_rank[s] = r;
}

// directed entry 2 e + d: image 1 is the pair's image d, image 2 the other one
__global__ void k_ip_entry_keys(IpOrder o) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * o.n_entries) return;
  const uint32_t e = i >> 1, d = i & 1u;
  const uint32_t first = o.v.ent_slot[2 * e + d], other = o.v.ent_slot[2 * e + 1 - d], cnt = o.v.pair_cnt[o.v.ent_pair[e]];
  const bool ok = (o.v.slot_flags[first] & IP_SLOT_FIRST) && (o.v.slot_flags[other] & IP_SLOT_SECOND) && cnt >= o.v.min_count;
  o.key[i] = ok ? ((uint64_t)o.slot_rank[first] << 40) | ip_second_key(o.v.slot_flags[other], cnt, other) : IP_KEY_NONE;
}

// kept = a candidate's first occurrence (its reversed entry is none or later) and not tried before
__device__ inline bool ip_entry_kept(const IpOrder& o, uint32_t i) {
  const uint64_t k = o.key[i];
  return k != IP_KEY_NONE && !o.v.ent_tried[i >> 1] && k < o.key[i ^ 1u];  // (IP_KEY_NONE is above every key)
}

__global__ void k_ip_entry_rank(IpOrder o) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 2 * o.n_entries) return;
  if (!ip_entry_kept(o, i)) return;
  const uint32_t p = o.ent_prob[i >> 1], i0 = 2 * o.v.ent_off[p], i1 = 2 * o.v.ent_off[p + 1];
  const uint64_t mine = o.key[i];
  uint32_t r = 0;
  for (uint32_t j = i0; j < i1; ++j) r += o.key[j] < mine && ip_entry_kept(o, j);
  o.cand[i0 + r] = i;
  atomicAdd(&o.cand_n[p], 1u);
}

#ifdef DSM_CHECK_BUILD
// DSM_INITIAL_PAIR_SERIAL: the reference's nested loops, problem after problem, on one lane
__global__ void k_ip_serial_order(IpOrder o) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t p = 0; p < o.v.n_problems; ++p) o.cand_n[p] = ip_serial_order(o.v, p, o.sum, o.seen, o.cand + 2 * o.v.ent_off[p]);
}
#endif

// ------------------------------------------------------------------ a batch of candidates
struct IpBatch {
  uint32_t n;
  const uint32_t* img;       // [2 n] image 1, image 2
  const uint32_t* src;       // [2 n] the pair (IP_NONE: the images share no pair) and whether image 1 is the pair's second image
  const uint64_t* off;       // [n + 1] the candidates' match lists
  uint32_t* out;             // the oriented lists, (point2D_idx1, point2D_idx2) ascending in point2D_idx1
  const uint64_t* moff;
  const uint32_t* matches;
  const uint8_t* acc;
  const uint32_t* nfeat;
};

// FindCorrespondencesBetweenImages(image 1, image 2): the kept matches of the pair, oriented, in ascending point2D index of
// image 1.  A kept match's place is the number of kept matches with a smaller index: a bitmap of image 1's matched points2D
// in LDS, popcounts per run of 32 words, a scan of the runs.
__global__ void k_ip_gather(IpBatch b) {
  __shared__ uint32_t bits[IP_MAX_POINTS2D / 32];
  __shared__ uint32_t run[IP_BLOCK], ex[IP_BLOCK];
  const uint32_t c = blockIdx.x;
  if (c >= b.n) return;
  const uint32_t k = b.src[2 * c], sw = b.src[2 * c + 1];
  if (k == IP_NONE) return;
  const uint32_t words = (b.nfeat[b.img[2 * c]] + 31) / 32;
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) bits[w] = 0u;
  __syncthreads();
  for (uint64_t m = b.moff[k] + threadIdx.x; m < b.moff[k + 1]; m += blockDim.x)
    if (b.acc[m]) {
      const uint32_t f = b.matches[2 * m + sw];
      atomicOr(&bits[f >> 5], 1u << (f & 31));
    }
  __syncthreads();
  uint32_t s = 0;
  for (uint32_t w = 32 * threadIdx.x; w < 32 * threadIdx.x + 32 && w < words; ++w) s += __popc(bits[w]);
  run[threadIdx.x] = s;
  __syncthreads();
  for (int d = 1; d < IP_BLOCK; d *= 2) {
    const uint32_t x = (int)threadIdx.x >= d ? run[threadIdx.x - d] : 0u;
    __syncthreads();
    run[threadIdx.x] += x;
    __syncthreads();
  }
  ex[threadIdx.x] = run[threadIdx.x] - s;
  __syncthreads();
  const uint64_t n_out = b.off[c + 1] - b.off[c];
  for (uint64_t m = b.moff[k] + threadIdx.x; m < b.moff[k + 1]; m += blockDim.x)
    if (b.acc[m]) {
      const uint32_t f = b.matches[2 * m + sw], w = f >> 5;
      uint32_t r = ex[w >> 5] + __popc(bits[w] & ((1u << (f & 31)) - 1u));
      for (uint32_t x = w & ~31u; x < w; ++x) r += __popc(bits[x]);
      if (r < n_out) {  // (always: the list holds the pair's kept matches)
        b.out[2 * (b.off[c] + r)] = f;
        b.out[2 * (b.off[c] + r) + 1] = b.matches[2 * m + 1 - sw];
      }
    }
}

// Camera::ImageToWorld of one point2D; one copy of the eleven models for all kernels of this file
__device__ __noinline__ void ip_to_world(const dsm_camera* cams, uint32_t image, const double* kp, uint32_t f, double* u, double* v) {
  image_to_world(cams[image], kp[2 * (size_t)f], kp[2 * (size_t)f + 1], u, v);
}

// triangulate_two_view (verify_linalg.h), one copy out of line for the kernels of this file
__device__ __noinline__ void ip_triangulate(const double* P1, const double* P2, double u1, double v1, double u2, double v2, double* X) {
  triangulate_two_view(P1, P2, u1, v1, u2, v2, X);
}

struct IpPoseParams {
  uint32_t n;
  const uint32_t* img;  // [2 n]
  const dsm_two_view_geometry* tvg;
  const uint64_t* inl_off;
  const uint32_t* inl;
  const double* kp;
  const uint32_t* row0;
  const dsm_camera* cams;
  double* angles;       // [inliers] scratch
  int32_t min_num_inliers;
  double max_forward, min_tri_angle_rad;
};
struct IpPose {  // the decision of one candidate
  int32_t accept, config;
  double tri_angle, forward_margin, tri_margin;
};

struct IpPoseSetup {
  double P1[12], P2[12], C1[3], C2[3], max_depth, n2;
};
__device__ inline void ip_pose_setup(const dsm_two_view_geometry& g, IpPoseSetup* s) {
  double R[9];
  ip_quat_to_R(g.qvec, R);
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  for (int i = 0; i < 12; ++i) s->P1[i] = I[i];
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) s->P2[4 * r + k] = R[3 * r + k];
    s->P2[4 * r + 3] = g.tvec[r];
  }
  s->C1[0] = s->C1[1] = s->C1[2] = 0.0;
  ip_minus_Rt_t(R, g.tvec, s->C2);
  // CheckCheirality (pose.cc:225-247)
  double rt[3];
  for (int i = 0; i < 3; ++i) rt[i] = R[i] * g.tvec[0] + R[3 + i] * g.tvec[1] + R[6 + i] * g.tvec[2];
  s->max_depth = 1000.0f * sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2]);
  s->n2 = sqrt(R[2] * R[2] + R[5] * R[5] + R[8] * R[8]);
}
// one inlier of CheckCheirality and its element of CalculateTriangulationAngles; false behind a camera or beyond max_depth
__device__ inline bool ip_pose_point(const IpPoseParams& p, const IpPoseSetup& s, uint32_t c, uint64_t j, double* angle) {
  const uint32_t i1 = p.img[2 * c], i2 = p.img[2 * c + 1];
  const uint32_t f1 = p.row0[i1] + p.inl[2 * j], f2 = p.row0[i2] + p.inl[2 * j + 1];
  double u1, v1, u2, v2, X[3];
  ip_to_world(p.cams, i1, p.kp, f1, &u1, &v1);
  ip_to_world(p.cams, i2, p.kp, f2, &u2, &v2);
  ip_triangulate(s.P1, s.P2, u1, v1, u2, v2, X);
  const double kMinDepth = DBL_EPSILON;
  const double d1 = (0.0 * X[0] + 0.0 * X[1] + 1.0 * X[2] + 0.0 * 1.0) * 1.0;
  if (!(d1 > kMinDepth && d1 < s.max_depth)) return false;
  const double d2 = (s.P2[8] * X[0] + s.P2[9] * X[1] + s.P2[10] * X[2] + s.P2[11] * 1.0) * s.n2;
  if (!(d2 > kMinDepth && d2 < s.max_depth)) return false;
  *angle = ip_tri_angle(s.C1, s.C2, X);
  return true;
}
__device__ inline bool ip_pose_defined(int32_t config) {
  return config == DSM_CONFIG_CALIBRATED || config == DSM_CONFIG_UNCALIBRATED || config == DSM_CONFIG_PLANAR || config == DSM_CONFIG_PANORAMIC ||
         config == DSM_CONFIG_PLANAR_OR_PANORAMIC;
}
__device__ inline void ip_pose_decide(const IpPoseParams& p, const dsm_two_view_geometry& g, bool defined, double tri_angle, IpPose* out) {
  IpPose r;
  r.accept = 0, r.config = g.config, r.tri_angle = 0.0, r.forward_margin = r.tri_margin = ip_inf();
  if (defined) {
    if (g.config == DSM_CONFIG_PLANAR_OR_PANORAMIC)  // two_view_geometry.cc:220-227
      r.config = sqrt((g.tvec[0] * g.tvec[0] + g.tvec[1] * g.tvec[1]) + g.tvec[2] * g.tvec[2]) == 0 ? DSM_CONFIG_PANORAMIC : DSM_CONFIG_PLANAR;
    r.tri_angle = r.config == DSM_CONFIG_PANORAMIC ? 0.0 : tri_angle;
    IpMargins mg = {ip_inf(), ip_inf(), ip_inf(), ip_inf()};
    r.accept = ip_accept(g.num_inliers, g.tvec[2], r.tri_angle, p.min_num_inliers, p.max_forward, p.min_tri_angle_rad, &mg);
    r.forward_margin = mg.forward, r.tri_margin = mg.tri_angle;
  }
  *out = r;
}

// EstimateRelativePose's acceptance for one verified candidate per one-wave workgroup: the points in front of both cameras in
// inlier order (ballot and popcount), their angles, the median by bisection on the bits, the three tests
__global__ void __launch_bounds__(64) k_ip_relative_pose(IpPoseParams p, IpPose* __restrict__ out) {
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  if (c >= p.n) return;
  const dsm_two_view_geometry g = p.tvg[c];
  const bool defined = ip_pose_defined(g.config);
  double tri_angle = 0.0;
  if (defined) {
    IpPoseSetup s;
    ip_pose_setup(g, &s);
    const uint64_t j0 = p.inl_off[c], ni = p.inl_off[c + 1] - j0;
    double* ang = p.angles + j0;
    uint64_t total = 0;
    for (uint64_t base = 0; base < ni; base += 64) {
      const uint64_t j = base + lane;
      double a = 0.0;
      const bool ok = j < ni && ip_pose_point(p, s, c, j0 + j, &a);
      const unsigned long long bal = __ballot(ok);
      if (ok) ang[total + __popcll(bal & ((1ull << lane) - 1ull))] = a;
      total += __popcll(bal);
    }
    __syncthreads();
    if (total) {
      auto count_below = [&](uint64_t v) {
        uint32_t cnt = 0;
        for (uint64_t i = lane; i < total; i += 64) cnt += ip_double_bits(ang[i]) < v;
        return (uint64_t)wave_sum(cnt);
      };
      const double mid = ip_bits_double(ip_select_bits(total / 2, count_below));
      const double below = total % 2 == 0 ? ip_bits_double(ip_select_bits(total / 2 - 1, count_below)) : 0.0;
      tri_angle = ip_median_of(mid, below, total);
    }
  }
  if (lane == 0) ip_pose_decide(p, g, defined, tri_angle, &out[c]);
}

struct IpTriParams {
  uint32_t n;
  const uint32_t* img;   // [2 n]
  const double* pose;    // [7 n] qvec, tvec of image 2
  const uint64_t* off;   // [n + 1] the winners' match lists
  const uint32_t* list;  // (point2D_idx1, point2D_idx2)
  const double* kp;
  const uint32_t* row0;
  const dsm_camera* cams;
  double min_angle_rad;
  double* xyz;           // the kept points of winner w from off[w], in correspondence order
  uint32_t* obs;
  uint32_t* count;       // [n]
  double* margins;       // [2 n] angle, depth
};
struct IpTriSetup {
  double P1[12], P2[12], C1[3], C2[3];
};
__device__ inline void ip_tri_setup(const double* pose, IpTriSetup* s) {
  const double I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};  // ComposeIdentityQuaternion, a zero tvec
  for (int i = 0; i < 12; ++i) s->P1[i] = I[i];
  s->C1[0] = s->C1[1] = s->C1[2] = 0.0;
  ip_compose_P(pose, pose + 4, s->P2);
  ip_projection_center(pose, pose + 4, s->C2);
}
__device__ inline bool ip_tri_point(const IpTriParams& p, const IpTriSetup& s, uint32_t w, uint64_t j, double* X, IpMargins* mg) {
  const uint32_t i1 = p.img[2 * w], i2 = p.img[2 * w + 1];
  const uint32_t f1 = p.row0[i1] + p.list[2 * j], f2 = p.row0[i2] + p.list[2 * j + 1];
  double u1, v1, u2, v2;
  ip_to_world(p.cams, i1, p.kp, f1, &u1, &v1);
  ip_to_world(p.cams, i2, p.kp, f2, &u2, &v2);
  ip_triangulate(s.P1, s.P2, u1, v1, u2, v2, X);
  return ip_point_gates(ip_tri_angle(s.C1, s.C2, X), p.min_angle_rad, s.P1, s.P2, X, mg);
}

// RegisterInitialImagePair's loop over the correspondences of one winning pair per workgroup: a lane per correspondence, the
// gates, a fixed-block scan per run of IP_BLOCK correspondences for the ordered compaction
__global__ void __launch_bounds__(IP_BLOCK) k_ip_triangulate(IpTriParams p) {
  __shared__ uint32_t sh[IP_BLOCK];
  __shared__ double shm[2][IP_BLOCK];
  const uint32_t w = blockIdx.x;
  if (w >= p.n) return;
  IpTriSetup s;
  ip_tri_setup(p.pose + 7 * (size_t)w, &s);
  IpMargins mg = {ip_inf(), ip_inf(), ip_inf(), ip_inf()};
  const uint64_t j0 = p.off[w], n = p.off[w + 1] - j0;
  uint32_t kept = 0;
  for (uint64_t base = 0; base < n; base += IP_BLOCK) {
    const uint64_t j = base + threadIdx.x;
    double X[3] = {0, 0, 0};
    const bool ok = j < n && ip_tri_point(p, s, w, j0 + j, X, &mg);
    sh[threadIdx.x] = ok;
    __syncthreads();
    for (int d = 1; d < IP_BLOCK; d *= 2) {
      const uint32_t x = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
      __syncthreads();
      sh[threadIdx.x] += x;
      __syncthreads();
    }
    if (ok) {
      const uint64_t at = j0 + kept + sh[threadIdx.x] - 1;
      p.xyz[3 * at] = X[0], p.xyz[3 * at + 1] = X[1], p.xyz[3 * at + 2] = X[2];
      p.obs[2 * at] = p.list[2 * (j0 + j)], p.obs[2 * at + 1] = p.list[2 * (j0 + j) + 1];
    }
    kept += sh[IP_BLOCK - 1];
    __syncthreads();
  }
  shm[0][threadIdx.x] = mg.point_angle;
  shm[1][threadIdx.x] = mg.point_depth;
  __syncthreads();
  for (int d = IP_BLOCK / 2; d > 0; d /= 2) {
    if ((int)threadIdx.x < d) {
      shm[0][threadIdx.x] = fmin(shm[0][threadIdx.x], shm[0][threadIdx.x + d]);
      shm[1][threadIdx.x] = fmin(shm[1][threadIdx.x], shm[1][threadIdx.x + d]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    p.count[w] = kept;
    p.margins[2 * w] = shm[0][0];
    p.margins[2 * w + 1] = shm[1][0];
  }
}

#ifdef DSM_CHECK_BUILD
// DSM_INITIAL_PAIR_SERIAL: the same pieces in the reference's loops on one lane
__global__ void k_ip_relative_pose_serial(IpPoseParams p, IpPose* __restrict__ out) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t c = 0; c < p.n; ++c) {
    const dsm_two_view_geometry g = p.tvg[c];
    const bool defined = ip_pose_defined(g.config);
    double tri_angle = 0.0;
    if (defined) {
      IpPoseSetup s;
      ip_pose_setup(g, &s);
      double* ang = p.angles + p.inl_off[c];
      uint64_t total = 0;
      for (uint64_t j = p.inl_off[c]; j < p.inl_off[c + 1]; ++j) {
        double a;
        if (ip_pose_point(p, s, c, j, &a)) ang[total++] = a;
      }
      if (total) tri_angle = ip_median_serial(ang, total);
    }
    ip_pose_decide(p, g, defined, tri_angle, &out[c]);
  }
}
__global__ void k_ip_triangulate_serial(IpTriParams p) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t w = 0; w < p.n; ++w) {
    IpTriSetup s;
    ip_tri_setup(p.pose + 7 * (size_t)w, &s);
    IpMargins mg = {ip_inf(), ip_inf(), ip_inf(), ip_inf()};
    uint32_t kept = 0;
    for (uint64_t j = p.off[w]; j < p.off[w + 1]; ++j) {
      double X[3];
      if (!ip_tri_point(p, s, w, j, X, &mg)) continue;
      const uint64_t at = p.off[w] + kept++;
      p.xyz[3 * at] = X[0], p.xyz[3 * at + 1] = X[1], p.xyz[3 * at + 2] = X[2];
      p.obs[2 * at] = p.list[2 * j], p.obs[2 * at + 1] = p.list[2 * j + 1];
    }
    p.count[w] = kept;
    p.margins[2 * w] = mg.point_angle;
    p.margins[2 * w + 1] = mg.point_depth;
  }
}
#endif

struct IpBufs {
  DevBuf pair_img, moff, matches, nfeat, acc, cnt, kp, row0, cams;
  DevBuf slot_off, slot_flags, slot_prob, ent_off, ent_pair, ent_slot, ent_tried, ent_prob, sum, slot_rank, key, cand, cand_n, seen;
  DevBuf b_img, b_src, b_off, b_list, b_seeds, b_pose, angles, t_pose, t_xyz, t_obs, t_count, t_margins;
};

struct IpCand {
  uint32_t img1, img2, pair, swapped;  // image indices; pair IP_NONE: the images share no pair
};

}  // namespace

extern "C" void dsm_default_initial_pair_options(dsm_initial_pair_options* o) { ip_default_options(o); }

extern "C" int dsm_find_initial_pairs(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                      uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                      const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                                      const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                      uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                                      const uint32_t* num_registrations, const uint32_t* init_num_reg_trials, const uint64_t* tried_offsets,
                                      const uint32_t* tried_pairs, const uint32_t* seed_image1, const uint32_t* seed_image2,
                                      const dsm_initial_pair_options* options, dsm_initial_pair_result* results,
                                      uint64_t* tried_out_offsets, uint32_t* tried_out_pairs, uint64_t tried_capacity,
                                      uint64_t* point_offsets, double* point_xyz, uint32_t* point_obs, uint64_t point_capacity,
                                      uint64_t* inlier_offsets, uint32_t* inlier_matches, uint64_t inlier_capacity,
                                      dsm_initial_pair_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](int code, const char* msg) { return dsm_fail(ctx, code, "dsm_find_initial_pairs", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  if ((num_cameras && (!camera_ids || !cameras)) || (num_images && (!image_ids || !image_camera_ids)) || !points2D_offsets || !match_offsets ||
      !problem_image_offsets || (num_problems && (!results || !tried_out_offsets || !point_offsets)))
    return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  dsm_initial_pair_options o;
  if (options)
    o = *options;
  else
    ip_default_options(&o);
  // cameras and the images' prior flags
  std::vector<uint32_t> cam_order;
  {
    const std::vector<uint64_t> wide(camera_ids, camera_ids + num_cameras);
    ip_sort_indices(cam_order, num_cameras, wide.data());
  }
  for (uint32_t c = 0; c < num_cameras; ++c) {
    if (c && camera_ids[cam_order[c]] == camera_ids[cam_order[c - 1]]) return fail(DSM_ERR_INVALID_ARGUMENT, "a repeated camera id");
    if (!cam_model_exists(cameras[c].model_id)) return fail(DSM_ERR_INVALID_ARGUMENT, "an unknown camera model");
    for (int i = 0; i < cam_num_params(cameras[c].model_id); ++i)
      if (!std::isfinite(cameras[c].params[i])) return fail(DSM_ERR_INVALID_ARGUMENT, "non-finite camera parameters");
  }
  std::vector<uint8_t> image_prior(num_images);
  std::vector<dsm_camera> image_cams(std::max<uint32_t>(num_images, 1));
  for (uint32_t i = 0; i < num_images; ++i) {
    auto it = std::lower_bound(cam_order.begin(), cam_order.end(), image_camera_ids[i], [&](uint32_t a, uint32_t v) { return camera_ids[a] < v; });
    if (it == cam_order.end() || camera_ids[*it] != image_camera_ids[i]) return fail(DSM_ERR_INVALID_ARGUMENT, "an image on an unknown camera id");
    image_prior[i] = cameras[*it].has_prior_focal_length != 0;
    image_cams[i] = cameras[*it];
    image_cams[i].has_prior_focal_length = 1;  // EstimateCalibrated is what the mapper calls, whatever the prior says
  }
  IpSetup S;
  if (const char* bad = S.load(num_images, image_ids, image_prior.data(), points2D_offsets, num_pairs, pair_image_ids, match_offsets, matches,
                               num_problems, problem_image_offsets, problem_image_ids, num_registrations, init_num_reg_trials, tried_offsets,
                               tried_pairs, seed_image1, seed_image2, o))
    return fail(S.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT, bad);
  const uint64_t F = points2D_offsets[num_images], NM = match_offsets[num_pairs];
  if (F && !points2D_xy) return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  for (uint64_t i = 0; i < 2 * F; ++i)
    if (!std::isfinite(points2D_xy[i])) return fail(DSM_ERR_INVALID_ARGUMENT, "non-finite points2D xy");
  const uint32_t n_slots = (uint32_t)S.slot_img.size(), n_entries = (uint32_t)S.ent_pair.size();
  std::vector<uint32_t> slot_prob(n_slots), ent_prob(n_entries);
  for (uint32_t p = 0; p < num_problems; ++p) {
    for (uint32_t s = S.slot_off[p]; s < S.slot_off[p + 1]; ++s) slot_prob[s] = p;
    for (uint32_t e = S.ent_off[p]; e < S.ent_off[p + 1]; ++e) ent_prob[e] = p;
  }
  dsm_initial_pair_report rep{};
  rep.min_tri_angle_margin = rep.min_forward_motion_margin = rep.min_point_angle_margin = rep.min_point_depth_margin = INFINITY;
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  bool serial = false;
#ifdef DSM_CHECK_BUILD
  if (const char* v = ctx->dbg("DSM_INITIAL_PAIR_SERIAL")) serial = atoi(v) != 0;
#endif
  const uint32_t window = serial ? 1u : o.speculation_window;

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  IpBufs d;
  DevEvents<4> ev, bev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, bev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  auto grid = [](uint64_t n) { return dim3(dsm_grid(n, IP_BLOCK)); };

  // ------------------------------------------------------------ the scene, the duplicate rule, the counts, the candidate order
  const size_t K1 = std::max<uint32_t>(num_pairs, 1);
  HIPCHK(ctx, dev_upload(d.nfeat, S.nfeat.data(), (size_t)num_images * 4, st));
  HIPCHK(ctx, dev_upload(d.row0, points2D_offsets, ((size_t)num_images + 1) * 4, st));
  HIPCHK(ctx, dev_upload(d.cams, image_cams.data(), (size_t)num_images * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.kp, points2D_xy, F * 16, st));
  HIPCHK(ctx, dev_upload(d.pair_img, S.pair_img.data(), S.pair_img.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.moff, match_offsets, ((size_t)num_pairs + 1) * 8, st));
  HIPCHK(ctx, dev_upload(d.matches, matches, NM * 8, st));
  HIPCHK(ctx, d.acc.reserve(std::max<uint64_t>(NM, 16)));
  HIPCHK(ctx, dev_fill(d.cnt, 0, K1 * 4, st));
  if (num_pairs) {
    hipLaunchKernelGGL(k_rt_dedup, dim3(num_pairs), dim3(IP_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.nfeat.as<uint32_t>(), d.acc.as<uint8_t>());
    hipLaunchKernelGGL(k_ip_pair_count, dim3(num_pairs), dim3(IP_BLOCK), 0, st, num_pairs, d.moff.as<uint64_t>(), d.acc.as<uint8_t>(),
                       d.cnt.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, dev_upload(d.slot_off, S.slot_off.data(), S.slot_off.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.slot_flags, S.slot_flags.data(), (size_t)n_slots * 4, st));
  HIPCHK(ctx, dev_upload(d.slot_prob, slot_prob.data(), (size_t)n_slots * 4, st));
  HIPCHK(ctx, dev_upload(d.ent_off, S.ent_off.data(), S.ent_off.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.ent_pair, S.ent_pair.data(), (size_t)n_entries * 4, st));
  HIPCHK(ctx, dev_upload(d.ent_slot, S.ent_slot.data(), (size_t)n_entries * 8, st));
  HIPCHK(ctx, dev_upload(d.ent_tried, S.ent_tried.data(), n_entries, st));
  HIPCHK(ctx, dev_upload(d.ent_prob, ent_prob.data(), (size_t)n_entries * 4, st));
  HIPCHK(ctx, dev_fill(d.sum, 0, (size_t)n_slots * 4, st));
  HIPCHK(ctx, d.slot_rank.reserve(std::max<size_t>((size_t)n_slots * 4, 16)));
  HIPCHK(ctx, d.key.reserve(std::max<size_t>((size_t)n_entries * 16, 16)));
  HIPCHK(ctx, dev_fill(d.cand, 0, (size_t)n_entries * 8, st));
  HIPCHK(ctx, dev_fill(d.cand_n, 0, (size_t)std::max<uint32_t>(num_problems, 1) * 4, st));
  HIPCHK(ctx, d.seen.reserve(std::max<uint32_t>(n_entries, 16)));
  IpOrder od;
  od.v = IpOrderView{num_problems,         d.slot_off.as<uint32_t>(), d.slot_flags.as<uint32_t>(), d.ent_off.as<uint32_t>(), d.ent_pair.as<uint32_t>(),
                     d.ent_slot.as<uint32_t>(), d.ent_tried.as<uint8_t>(),  d.cnt.as<uint32_t>(),        (uint32_t)std::max(o.init_min_num_inliers, 1)};
  od.n_slots = n_slots, od.n_entries = n_entries;
  od.slot_prob = d.slot_prob.as<uint32_t>(), od.ent_prob = d.ent_prob.as<uint32_t>();
  od.sum = d.sum.as<uint32_t>(), od.slot_rank = d.slot_rank.as<uint32_t>(), od.key = d.key.as<uint64_t>();
  od.cand = d.cand.as<uint32_t>(), od.cand_n = d.cand_n.as<uint32_t>(), od.seen = d.seen.as<uint8_t>();
  if (serial) {
#ifdef DSM_CHECK_BUILD
    hipLaunchKernelGGL(k_ip_serial_order, dim3(1), dim3(1), 0, st, od);
#endif
  } else if (n_entries) {
    hipLaunchKernelGGL(k_ip_sums, grid(n_entries), dim3(IP_BLOCK), 0, st, od);
    hipLaunchKernelGGL(k_ip_slot_rank, grid(n_slots), dim3(IP_BLOCK), 0, st, od);
    hipLaunchKernelGGL(k_ip_entry_keys, grid(2ull * n_entries), dim3(IP_BLOCK), 0, st, od);
    hipLaunchKernelGGL(k_ip_entry_rank, grid(2ull * n_entries), dim3(IP_BLOCK), 0, st, od);
  }
  HIPCHK(ctx, hipGetLastError());
  std::vector<uint32_t> cnt(num_pairs), cand_raw(2 * (size_t)n_entries), cand_n(num_problems);
  if (num_pairs) HIPCHK(ctx, hipMemcpyAsync(cnt.data(), d.cnt.p, (size_t)num_pairs * 4, hipMemcpyDeviceToHost, st));
  if (n_entries) HIPCHK(ctx, hipMemcpyAsync(cand_raw.data(), d.cand.p, (size_t)n_entries * 8, hipMemcpyDeviceToHost, st));
  if (num_problems) HIPCHK(ctx, hipMemcpyAsync(cand_n.data(), d.cand_n.p, (size_t)num_problems * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  HIPCHK(ctx, hipStreamSynchronize(st));

  // every problem's candidate list
  std::vector<std::vector<IpCand>> cands(num_problems);
  for (uint32_t p = 0; p < num_problems; ++p) {
    if (S.both_seed_entry[p] != -2) {  // both seed images: that pair alone
      IpCand c{S.both_seed_img[2 * p], S.both_seed_img[2 * p + 1], IP_NONE, 0};
      if (S.both_seed_entry[p] >= 0) {
        c.pair = S.ent_pair[S.both_seed_entry[p]];
        c.swapped = S.pair_img[2 * (size_t)c.pair] != c.img1;
      }
      cands[p].push_back(c);
    } else {
      if (cand_n[p] > 2 * (S.ent_off[p + 1] - S.ent_off[p])) return fail(DSM_ERR_HIP, "the candidate order overran its list");
      for (uint32_t i = 0; i < cand_n[p]; ++i) {
        const uint32_t v = cand_raw[2 * (size_t)S.ent_off[p] + i], e = v >> 1, dir = v & 1u, k = S.ent_pair[e];
        cands[p].push_back(IpCand{S.pair_img[2 * (size_t)k + dir], S.pair_img[2 * (size_t)k + 1 - dir], k, dir});
      }
    }
    rep.num_candidates += cands[p].size();
  }

  // ------------------------------------------------------------ the rounds
  dsm_two_view_options to;
  dsm_default_two_view_options(&to);
  to.min_num_trials = 30;  // incremental_mapper.cc:1155-1157
  to.max_error = o.init_max_error;
  to.multiple_models = 0;
  const double min_tri_rad = o.init_min_tri_angle * IP_DEG_TO_RAD;
  std::vector<uint32_t> next(num_problems, 0);
  std::vector<int64_t> winner(num_problems, -1);
  std::vector<dsm_two_view_geometry> win_tvg(num_problems);
  std::vector<std::vector<uint32_t>> win_inl(num_problems);
  std::vector<uint64_t> h_inl_off;
  std::vector<uint8_t> finished(num_problems, 0);
  uint32_t unfinished = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    finished[p] = cands[p].empty();
    unfinished += !finished[p];
  }
  // what a candidate costs on the device: its gathered list, and the verifier's arrays per match and per pair (capi.hip)
  auto cand_bytes = [&](const IpCand& c) { return (uint64_t)(c.pair == IP_NONE ? 0 : cnt[c.pair]) * 160 + 8192; };
  struct Item {
    uint32_t p, i;
  };
  std::vector<Item> items;
  std::vector<IpPose> poses;
  std::vector<dsm_two_view_geometry> tvgs;
  std::vector<uint32_t> b_img, b_src, b_seeds, counts;
  std::vector<uint64_t> b_off;
  double ms = 0;
  while (unfinished) {
    ++rep.num_rounds;
    uint32_t p_next = 0;
    while (p_next < num_problems) {  // a round's batches: cut by problems where the memory budget asks for it
      items.clear();
      uint64_t bytes = 0;
      for (; p_next < num_problems; ++p_next) {
        const uint32_t p = p_next;
        if (finished[p]) continue;
        const uint32_t hi = (uint32_t)std::min<uint64_t>(cands[p].size(), (uint64_t)next[p] + window);
        uint64_t mine = 0;
        for (uint32_t i = next[p]; i < hi; ++i) mine += cand_bytes(cands[p][i]);
        if (ctx->memory_budget && !items.empty() && bytes + mine > ctx->memory_budget) break;
        for (uint32_t i = next[p]; i < hi; ++i) items.push_back(Item{p, i});
        bytes += mine;
      }
      if (items.empty()) break;
      ++rep.num_batches;
      const uint32_t n = (uint32_t)items.size();
      b_img.resize(2 * (size_t)n), b_src.resize(2 * (size_t)n), b_seeds.resize(n), counts.resize(n), b_off.assign((size_t)n + 1, 0);
      for (uint32_t c = 0; c < n; ++c) {
        const IpCand& cd = cands[items[c].p][items[c].i];
        b_img[2 * c] = cd.img1, b_img[2 * c + 1] = cd.img2;
        b_src[2 * c] = cd.pair, b_src[2 * c + 1] = cd.swapped;
        counts[c] = cd.pair == IP_NONE ? 0 : cnt[cd.pair];
        b_off[c + 1] = b_off[c] + counts[c];
        b_seeds[c] = dsm_pair_seed(image_ids[cd.img1], image_ids[cd.img2], o.user_seed);
      }
      const uint64_t total = b_off[n];
      HIPCHK(ctx, hipEventRecord(bev[0], st));
      HIPCHK(ctx, dev_upload(d.b_img, b_img.data(), b_img.size() * 4, st));
      HIPCHK(ctx, dev_upload(d.b_src, b_src.data(), b_src.size() * 4, st));
      HIPCHK(ctx, dev_upload(d.b_off, b_off.data(), b_off.size() * 8, st));
      HIPCHK(ctx, dev_upload(d.b_seeds, b_seeds.data(), b_seeds.size() * 4, st));
      HIPCHK(ctx, d.b_list.reserve(std::max<uint64_t>(total * 8, 16)));
      IpBatch bt{n,        d.b_img.as<uint32_t>(),   d.b_src.as<uint32_t>(), d.b_off.as<uint64_t>(), d.b_list.as<uint32_t>(), d.moff.as<uint64_t>(),
                 d.matches.as<uint32_t>(), d.acc.as<uint8_t>(), d.nfeat.as<uint32_t>()};
      hipLaunchKernelGGL(k_ip_gather, dim3(n), dim3(IP_BLOCK), 0, st, bt);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipEventRecord(bev[1], st));
      HIPCHK(ctx, hipStreamSynchronize(st));  // the leaf context runs on its own stream
      IpPoseParams pp;
      uint64_t total_inliers = 0;
      int rc = dsm_verify_on_leaf(ctx, n, d.b_img.as<uint32_t>(), d.b_off.as<uint64_t>(), d.b_list.as<uint32_t>(), total, counts, d.kp.as<double>(),
                                  d.row0.as<uint32_t>(), d.cams.as<dsm_camera>(), &to, d.b_seeds.as<uint32_t>(), &pp.tvg, &pp.inl_off, &pp.inl,
                                  &total_inliers, nullptr);
      if (rc != DSM_OK) return rc;
      HIPCHK(ctx, hipSetDevice(ctx->device));
      HIPCHK(ctx, hipEventRecord(bev[2], st));
      HIPCHK(ctx, d.angles.reserve(std::max<uint64_t>(total_inliers * 8, 16)));
      HIPCHK(ctx, d.b_pose.reserve((size_t)n * sizeof(IpPose)));
      pp.n = n, pp.img = d.b_img.as<uint32_t>(), pp.kp = d.kp.as<double>(), pp.row0 = d.row0.as<uint32_t>(), pp.cams = d.cams.as<dsm_camera>();
      pp.angles = d.angles.as<double>(), pp.min_num_inliers = o.init_min_num_inliers, pp.max_forward = o.init_max_forward_motion;
      pp.min_tri_angle_rad = min_tri_rad;
      if (serial) {
#ifdef DSM_CHECK_BUILD
        hipLaunchKernelGGL(k_ip_relative_pose_serial, dim3(1), dim3(1), 0, st, pp, d.b_pose.as<IpPose>());
#endif
      } else {
        hipLaunchKernelGGL(k_ip_relative_pose, dim3(n), dim3(64), 0, st, pp, d.b_pose.as<IpPose>());
      }
      HIPCHK(ctx, hipGetLastError());
      poses.resize(n), tvgs.resize(n);
      HIPCHK(ctx, hipMemcpyAsync(poses.data(), d.b_pose.p, (size_t)n * sizeof(IpPose), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(tvgs.data(), pp.tvg, (size_t)n * sizeof(dsm_two_view_geometry), hipMemcpyDeviceToHost, st));
      h_inl_off.resize((size_t)n + 1);
      HIPCHK(ctx, hipMemcpyAsync(h_inl_off.data(), pp.inl_off, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipEventRecord(bev[3], st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, bev.ms(0, 1, &ms));
      rep.gather_ms += ms;
      HIPCHK(ctx, bev.ms(1, 2, &ms));
      rep.verify_ms += ms;
      HIPCHK(ctx, bev.ms(2, 3, &ms));
      rep.pose_ms += ms;
      rep.num_verified += n;
      // the replay: a problem's candidates in list order, the first accepted one wins
      for (uint32_t c = 0; c < n;) {
        const uint32_t p = items[c].p;
        uint32_t c1 = c;
        while (c1 < n && items[c1].p == p) ++c1;
        for (uint32_t x = c; x < c1; ++x) {
          rep.min_forward_motion_margin = std::min(rep.min_forward_motion_margin, poses[x].forward_margin);
          rep.min_tri_angle_margin = std::min(rep.min_tri_angle_margin, poses[x].tri_margin);
          if (!poses[x].accept) continue;
          winner[p] = items[x].i;
          win_tvg[p] = tvgs[x];
          win_tvg[p].config = poses[x].config;
          win_tvg[p].tri_angle = poses[x].tri_angle;
          win_inl[p].resize(2 * (h_inl_off[x + 1] - h_inl_off[x]));
          if (!win_inl[p].empty()) HIPCHK(ctx, hipMemcpy(win_inl[p].data(), pp.inl + 2 * h_inl_off[x], win_inl[p].size() * 4, hipMemcpyDeviceToHost));
          rep.num_speculated += c1 - x - 1;
          break;
        }
        next[p] = winner[p] >= 0 ? (uint32_t)winner[p] + 1 : items[c1 - 1].i + 1;
        if (winner[p] >= 0 || next[p] >= cands[p].size()) finished[p] = 1, --unfinished;
        c = c1;
      }
    }
  }
  HIPCHK(ctx, hipEventRecord(ev[2], st));

  // ------------------------------------------------------------ the winners' points
  std::vector<uint32_t> wins;
  for (uint32_t p = 0; p < num_problems; ++p)
    if (winner[p] >= 0) wins.push_back(p);
  const uint32_t nw = (uint32_t)wins.size();
  std::vector<uint64_t> t_off((size_t)nw + 1, 0);
  std::vector<uint32_t> t_count(nw);
  std::vector<double> t_xyz, t_margins(2 * (size_t)nw);
  std::vector<uint32_t> t_obs;
  if (nw) {
    b_img.resize(2 * (size_t)nw), b_src.resize(2 * (size_t)nw);
    std::vector<double> pose(7 * (size_t)nw);
    for (uint32_t w = 0; w < nw; ++w) {
      const IpCand& cd = cands[wins[w]][winner[wins[w]]];
      b_img[2 * w] = cd.img1, b_img[2 * w + 1] = cd.img2, b_src[2 * w] = cd.pair, b_src[2 * w + 1] = cd.swapped;
      t_off[w + 1] = t_off[w] + (cd.pair == IP_NONE ? 0 : cnt[cd.pair]);
      for (int k = 0; k < 4; ++k) pose[7 * (size_t)w + k] = win_tvg[wins[w]].qvec[k];
      for (int k = 0; k < 3; ++k) pose[7 * (size_t)w + 4 + k] = win_tvg[wins[w]].tvec[k];
    }
    const uint64_t total = t_off[nw], T1 = std::max<uint64_t>(total, 1);
    HIPCHK(ctx, dev_upload(d.b_img, b_img.data(), b_img.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.b_src, b_src.data(), b_src.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.b_off, t_off.data(), t_off.size() * 8, st));
    HIPCHK(ctx, dev_upload(d.t_pose, pose.data(), pose.size() * 8, st));
    HIPCHK(ctx, d.b_list.reserve(T1 * 8));
    HIPCHK(ctx, d.t_xyz.reserve(T1 * 24));
    HIPCHK(ctx, d.t_obs.reserve(T1 * 8));
    HIPCHK(ctx, dev_fill(d.t_count, 0, (size_t)nw * 4, st));
    HIPCHK(ctx, d.t_margins.reserve((size_t)nw * 16));
    IpBatch bt{nw,       d.b_img.as<uint32_t>(),   d.b_src.as<uint32_t>(), d.b_off.as<uint64_t>(), d.b_list.as<uint32_t>(), d.moff.as<uint64_t>(),
               d.matches.as<uint32_t>(), d.acc.as<uint8_t>(), d.nfeat.as<uint32_t>()};
    hipLaunchKernelGGL(k_ip_gather, dim3(nw), dim3(IP_BLOCK), 0, st, bt);
    IpTriParams tp{nw,           d.b_img.as<uint32_t>(),   d.t_pose.as<double>(), d.b_off.as<uint64_t>(), d.b_list.as<uint32_t>(), d.kp.as<double>(),
                   d.row0.as<uint32_t>(), d.cams.as<dsm_camera>(), min_tri_rad,           d.t_xyz.as<double>(),   d.t_obs.as<uint32_t>(),  d.t_count.as<uint32_t>(),
                   d.t_margins.as<double>()};
    if (serial) {
#ifdef DSM_CHECK_BUILD
      hipLaunchKernelGGL(k_ip_triangulate_serial, dim3(1), dim3(1), 0, st, tp);
#endif
    } else {
      hipLaunchKernelGGL(k_ip_triangulate, dim3(nw), dim3(IP_BLOCK), 0, st, tp);
    }
    HIPCHK(ctx, hipGetLastError());
    t_xyz.resize(3 * T1), t_obs.resize(2 * T1);
    HIPCHK(ctx, hipMemcpyAsync(t_count.data(), d.t_count.p, (size_t)nw * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(t_margins.data(), d.t_margins.p, (size_t)nw * 16, hipMemcpyDeviceToHost, st));
    if (total) {
      HIPCHK(ctx, hipMemcpyAsync(t_xyz.data(), d.t_xyz.p, total * 24, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(t_obs.data(), d.t_obs.p, total * 8, hipMemcpyDeviceToHost, st));
    }
  }
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, ev.ms(0, 1, &rep.graph_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rep.triangulate_ms));
  HIPCHK(ctx, ev.ms(0, 3, &rep.device_ms));

  // ------------------------------------------------------------ the results
  uint64_t n_tried = 0, n_points = 0, n_inl = 0, at_inl = 0;
  for (uint32_t p = 0; p < num_problems; ++p) n_inl += win_inl[p].size() / 2;
  if (inlier_matches && n_inl > inlier_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "inlier_matches is too small");
  for (uint32_t p = 0; p < num_problems; ++p) n_tried += winner[p] >= 0 ? (uint64_t)winner[p] + 1 : cands[p].size();
  for (uint32_t w = 0; w < nw; ++w) {
    if (t_count[w] > t_off[w + 1] - t_off[w]) return fail(DSM_ERR_HIP, "the triangulation overran its list");
    n_points += t_count[w];
  }
  if (tried_out_pairs && n_tried > tried_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "tried_out_pairs is too small");
  if ((point_xyz || point_obs) && n_points > point_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "point_xyz / point_obs are too small");
  uint64_t at_tried = 0, at_point = 0;
  uint32_t w = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    dsm_initial_pair_result r;
    memset(&r, 0, sizeof(r));
    const uint32_t tried = winner[p] >= 0 ? (uint32_t)winner[p] + 1 : (uint32_t)cands[p].size();
    r.status = winner[p] >= 0 ? DSM_INITIAL_PAIR_FOUND : DSM_INITIAL_PAIR_NONE;
    r.image_id1 = r.image_id2 = DSM_NO_IMAGE;
    r.num_tried = tried;
    tried_out_offsets[p] = at_tried;
    point_offsets[p] = at_point;
    if (inlier_offsets) inlier_offsets[p] = at_inl;
    if (inlier_matches && !win_inl[p].empty()) memcpy(inlier_matches + 2 * at_inl, win_inl[p].data(), win_inl[p].size() * 4);
    at_inl += win_inl[p].size() / 2;
    for (uint32_t i = 0; i < tried; ++i, ++at_tried)
      if (tried_out_pairs) tried_out_pairs[2 * at_tried] = image_ids[cands[p][i].img1], tried_out_pairs[2 * at_tried + 1] = image_ids[cands[p][i].img2];
    if (winner[p] >= 0) {
      const IpCand& cd = cands[p][winner[p]];
      r.image_id1 = image_ids[cd.img1], r.image_id2 = image_ids[cd.img2];
      r.two_view_geometry = win_tvg[p];
      r.num_points = t_count[w];
      if (point_xyz && t_count[w]) memcpy(point_xyz + 3 * at_point, t_xyz.data() + 3 * t_off[w], (size_t)t_count[w] * 24);
      if (point_obs && t_count[w]) memcpy(point_obs + 2 * at_point, t_obs.data() + 2 * t_off[w], (size_t)t_count[w] * 8);
      at_point += t_count[w];
      rep.min_point_angle_margin = std::min(rep.min_point_angle_margin, t_margins[2 * (size_t)w]);
      rep.min_point_depth_margin = std::min(rep.min_point_depth_margin, t_margins[2 * (size_t)w + 1]);
      ++w;
    }
    results[p] = r;
  }
  if (num_problems) tried_out_offsets[num_problems] = at_tried, point_offsets[num_problems] = at_point;
  if (num_problems && inlier_offsets) inlier_offsets[num_problems] = at_inl;
  if (report) *report = rep;
  return DSM_OK;
}
