// cluster_alignment.hip -- alignment of the cluster reconstructions for merging ("Cluster alignment").
//   SfMAligner::Align / ConstructReconsGraph / ComputeEdgeWeight   src/controllers/sfm_aligner.cpp:149-327
//   FindSimilarityTransform, FindCommon3DPoints, CheckReprojError   src/controllers/sfm_aligner.cpp:34-125
//   RansacSimilarity (PROSAC, sample 4, MLE cost)                  src/estimators/ransac_similarity.h:206-245
//   ProsacSampler::Sample, SampleConsensusEstimator::Estimate      src/ransac/prosac_sampler.cpp, sample_consensus_estimator.h:277-345
//   FindRTS (Eigen::umeyama with scaling)                           src/estimators/rigid_transformation3D_srt.cpp:48-82
//   FindAnchorNode, ComputePath                                     src/controllers/sfm_aligner.cpp:329-417
// The join: every observation (image_id, point2D_idx) of every cluster is radix-sorted by that key (stable: cluster order
// inside a key); a key held by m clusters yields m (m - 1) / 2 correspondences, counted, scanned and written, then sorted
// stably by (cluster pair, rank of the point id in the second cluster) into a CSR per pair -- the canonical order.
// PROSAC: one workgroup per (pair, direction), largest N first.  Lane 0 draws the next batch of samples from the problem's
// std::mt19937 stream (the host tabulated PROSAC's n(k) and branch and ComputeMaxIterations per inlier count), every lane fits
// one 4-point Umeyama and sums its MLE cost over all N in index order, then lane 0 replays the batch in trial order: the strict
// best update and the iteration cap, exactly as the serial loop.  Trials past the cap are speculation and are dropped.
// The refit (Umeyama on the inliers or on all N) and msd are block reductions in a fixed order.  The K-node graph, Kruskal,
// the anchor and the composed transforms run on the host.  Every result is the same bytes from run to run and for any order
// of the points and observations inside a cluster.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "block_reduce.h"
#include "ctx.h"
#include "std_mt19937.h"
#include "verify_linalg.h"

namespace {

constexpr int AL_BLOCK = 256;   // lanes of a PROSAC / refit workgroup = trials per speculative batch
constexpr int AL_CHUNK = 256;   // correspondences staged in LDS per step of the cost loop
constexpr int kAlMaxIterationsCap = 5000;
constexpr double kAlClearMargin = 1e-9;  // a relative cost gap no rounding of a model flips  // PROSAC's index n stays <= N - 1 up to here
constexpr uint32_t kAlFlagUnregistered = 1, kAlFlagPointRange = 2, kAlFlagDuplicateObs = 4, kAlFlagDuplicatePoint = 8;

// Eigen 3.3's 3 x 3 determinant (bruteforce_det3_helper order)
__device__ __host__ inline double al_det3(const double* m) {  // row-major
  return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2]);
}

// A model: s, R (row-major), t.  Sim3() = (1, I, 0).
struct AlModel {
  double s, R[9], t[3];
};
__device__ inline void al_identity(AlModel* m) {
  m->s = 1.0;
  for (int i = 0; i < 9; ++i) m->R[i] = (i % 4 == 0) ? 1.0 : 0.0;
  m->t[0] = m->t[1] = m->t[2] = 0.0;
}

// FindRTS from the moments of Eigen::umeyama(x1, x2, true): means, sigma = (sum d2 d1^T) / m (row-major), src_var.
// In / out as FindRTS: on det(cR) < 0 only R changes (to cR); on S < eps R and s change, t does not.
__device__ void al_find_rts(const double* mean1, const double* mean2, const double* sigma, double src_var, AlModel* m) {
  double U[9], V[9], sv[3];
  pl_jacobi_svd_square<3, true>(sigma, U, V, sv);  // U, V column-major
  double Ur[9], Vr[9];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      Ur[r * 3 + c] = U[c * 3 + r];
      Vr[r * 3 + c] = V[c * 3 + r];
    }
  double S[3] = {1.0, 1.0, 1.0};
  if (al_det3(Ur) * al_det3(Vr) < 0.0) S[2] = -1.0;
  double R[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = (Ur[i * 3 + 0] * S[0]) * Vr[j * 3 + 0] + (Ur[i * 3 + 1] * S[1]) * Vr[j * 3 + 1] +
                                               (Ur[i * 3 + 2] * S[2]) * Vr[j * 3 + 2];
  const double c = (1.0 / src_var) * (sv[0] * S[0] + sv[1] * S[1] + sv[2] * S[2]);
  double t[3], cR[9];
  for (int i = 0; i < 3; ++i)
    t[i] = mean2[i] - ((c * R[i * 3 + 0]) * mean1[0] + (c * R[i * 3 + 1]) * mean1[1] + (c * R[i * 3 + 2]) * mean1[2]);
  for (int i = 0; i < 9; ++i) cR[i] = R[i] * c;
  for (int i = 0; i < 9; ++i) m->R[i] = cR[i];
  const double det = al_det3(cR);
  if (det < 0.0) return;
  const double S3 = pow(det, 1.0 / 3.0);
  m->s = S3;
  if (S3 < DBL_EPSILON) return;
  for (int i = 0; i < 9; ++i) m->R[i] = cR[i] / S3;
  for (int i = 0; i < 3; ++i) m->t[i] = t[i];
}

// the residual ||s R x1 + t - x2|| (ReprojectionErr), with A = s R precomputed
__device__ inline double al_residual(const double* A, const double* t, double a0, double a1, double a2, double b0, double b1, double b2) {
  const double d0 = (A[0] * a0 + A[1] * a1 + A[2] * a2 + t[0]) - b0;
  const double d1 = (A[3] * a0 + A[4] * a1 + A[5] * a2 + t[1]) - b1;
  const double d2 = (A[6] * a0 + A[7] * a1 + A[8] * a2 + t[2]) - b2;
  return sqrt(d0 * d0 + d1 * d1 + d2 * d2);
}

// ---------------------------------------------------------------- the join
__device__ inline uint32_t al_segment(const uint32_t* off, uint32_t K, uint32_t x) {  // c with off[c] <= x < off[c + 1]
  uint32_t lo = 0, hi = K;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(256) k_al_obs_prep(uint32_t M, uint32_t K, const uint32_t* __restrict__ obs_off, const uint32_t* __restrict__ obs,
                                                     const uint32_t* __restrict__ pt_off, const uint64_t* __restrict__ reg, uint32_t n_reg,
                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ ocl,
                                                     uint32_t* __restrict__ opt, uint32_t* __restrict__ flags) {
  const uint32_t m = blockIdx.x * 256 + threadIdx.x;
  if (m >= M) return;
  const uint32_t c = al_segment(obs_off, K, m);
  const uint32_t img = obs[3 * (size_t)m], p2d = obs[3 * (size_t)m + 1], pl = obs[3 * (size_t)m + 2];
  if (pl >= pt_off[c + 1] - pt_off[c]) atomicOr(flags, kAlFlagPointRange);
  const uint64_t want = ((uint64_t)img << 32) | c;
  uint32_t lo = 0, hi = n_reg;  // registration keys sorted ascending
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (reg[mid] < want) lo = mid + 1; else hi = mid;
  }
  if (lo >= n_reg || reg[lo] != want) atomicOr(flags, kAlFlagUnregistered);
  key[m] = ((uint64_t)img << 32) | p2d;
  val[m] = m;
  ocl[m] = c;
  opt[m] = pt_off[c] + min(pl, pt_off[c + 1] - pt_off[c] - 1u);  // clamped: an invalid index is reported, never read
}

__global__ void __launch_bounds__(256) k_al_iota(uint32_t n, uint32_t* __restrict__ v) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] = i;
}

// points sorted by id: their cluster as the key of the second (stable) sort
__global__ void __launch_bounds__(256) k_al_point_cluster(uint32_t P, uint32_t K, const uint32_t* __restrict__ pt_off, const uint32_t* __restrict__ val,
                                                          uint32_t* __restrict__ ckey) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n < P) ckey[n] = al_segment(pt_off, K, val[n]);
}

// sorted by (cluster, id): the rank of a point inside its cluster; equal ids inside a cluster are an error
__global__ void __launch_bounds__(256) k_al_point_rank(uint32_t P, const uint32_t* __restrict__ pt_off, const uint32_t* __restrict__ ckey,
                                                       const uint32_t* __restrict__ val, const uint64_t* __restrict__ ids,
                                                       uint32_t* __restrict__ rank, uint32_t* __restrict__ flags) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= P) return;
  const uint32_t c = ckey[n];
  rank[val[n]] = n - pt_off[c];
  if (n > 0 && ckey[n - 1] == c && ids[val[n - 1]] == ids[val[n]]) atomicOr(flags, kAlFlagDuplicatePoint);
}

// sorted observations: the heads of the key runs; a repeated key inside one cluster is an error (checked before any
// work that grows with a run's length)
__global__ void __launch_bounds__(256) k_al_heads(uint32_t M, const uint64_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                  const uint32_t* __restrict__ ocl, uint32_t* __restrict__ head, uint32_t* __restrict__ flags) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= M) return;
  const bool h = n == 0 || key[n] != key[n - 1];
  head[n] = h ? 1u : 0u;
  if (!h && ocl[val[n]] == ocl[val[n - 1]]) atomicOr(flags, kAlFlagDuplicateObs);
}
// rid = inclusive scan of head: the first position of every run
__global__ void __launch_bounds__(256) k_al_head_pos(uint32_t M, const uint32_t* __restrict__ head, const uint32_t* __restrict__ rid,
                                                     uint32_t* __restrict__ hpos) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n < M && head[n]) hpos[rid[n] - 1] = n;
}
// count = the later elements of the key's run
__global__ void __launch_bounds__(256) k_al_count(uint32_t M, const uint32_t* __restrict__ rid, const uint32_t* __restrict__ hpos,
                                                  uint64_t* __restrict__ cnt) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= M) return;
  const uint32_t r = rid[n], n_runs = rid[M - 1];  // run r - 1 (0-based) holds n
  const uint32_t end = r < n_runs ? hpos[r] : M;
  cnt[n] = end - n - 1;
}

__global__ void __launch_bounds__(256) k_al_emit(uint32_t M, uint32_t K, const uint64_t* __restrict__ cnt, const uint32_t* __restrict__ val,
                                                 const uint32_t* __restrict__ ocl, const uint32_t* __restrict__ opt,
                                                 const uint32_t* __restrict__ rank, const uint64_t* __restrict__ off,
                                                 uint64_t* __restrict__ ckey, uint32_t* __restrict__ cval, uint32_t* __restrict__ csrc,
                                                 uint32_t* __restrict__ cref) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= M) return;
  const uint32_t a = val[n], ci = ocl[a];
  uint64_t e = off[n];
  const uint32_t end = n + 1 + (uint32_t)cnt[n];
  for (uint32_t l = n + 1; l < end; ++l, ++e) {
    const uint32_t b = val[l], cj = ocl[b];  // ci < cj: the stable sort keeps cluster order inside a key
    ckey[e] = ((uint64_t)(ci * K + cj) << 32) | rank[opt[b]];
    cval[e] = (uint32_t)e;
    csrc[e] = opt[a];
    cref[e] = opt[b];
  }
}

// canonical order -> contiguous coordinates (x1 of cluster i, x2 of cluster j) and the heads of the pair runs
__global__ void __launch_bounds__(256) k_al_gather(uint32_t C, const uint64_t* __restrict__ ckey, const uint32_t* __restrict__ cval,
                                                   const uint32_t* __restrict__ csrc, const uint32_t* __restrict__ cref,
                                                   const double* __restrict__ xyz, double* __restrict__ X1, double* __restrict__ X2,
                                                   uint32_t* __restrict__ heads, uint32_t* __restrict__ n_heads) {
  const uint32_t n = blockIdx.x * 256 + threadIdx.x;
  if (n >= C) return;
  const uint32_t e = cval[n], s = csrc[e], r = cref[e];
  for (int d = 0; d < 3; ++d) {
    X1[3 * (size_t)n + d] = xyz[3 * (size_t)s + d];
    X2[3 * (size_t)n + d] = xyz[3 * (size_t)r + d];
  }
  if (n == 0 || (ckey[n] >> 32) != (ckey[n - 1] >> 32)) {
    const uint32_t h = atomicAdd(n_heads, 1u);
    heads[2 * h] = (uint32_t)(ckey[n] >> 32);
    heads[2 * h + 1] = n;
  }
}

// ---------------------------------------------------------------- PROSAC
struct AlProblem {
  uint32_t off, N;     // the pair's correspondences
  uint32_t dir;        // 0: x1 -> x2, 1: x2 -> x1
  uint32_t seed;
  uint32_t ntab;       // offset of n(k) | branch << 31, k = 1 .. max_iterations
  uint32_t mtab;       // offset of ComputeMaxIterations(c / N), c = 0 .. N
  uint32_t slot;       // output slot
  uint32_t pad;
};
struct AlProsacOut {
  AlModel model;
  uint32_t iterations, pad;
  double residual_margin, cost_margin;
  double best_cost;  // the MLE cost of the best model
};

struct AlSmem {
  StdMt19937 gen;  // std::mt19937 and uniform_int_distribution<int>(0, hi) on it, lane 0 of the workgroup
  int samp[AL_BLOCK][4];
  double pts[AL_CHUNK][6];
  double cost[AL_BLOCK];
  double rmarg[AL_BLOCK];
  int cnt[AL_BLOCK];
  AlModel models[AL_BLOCK];
  int ctl[3];  // lane 0's serial loop: [0] ended inside this batch, [1] trials done, [2] the iteration cap
};

__device__ inline void al_load(const double* X1, const double* X2, uint32_t dir, size_t i, double* a, double* b) {
  const double* p = dir ? X2 : X1;
  const double* q = dir ? X1 : X2;
  a[0] = p[3 * i], a[1] = p[3 * i + 1], a[2] = p[3 * i + 2];
  b[0] = q[3 * i], b[1] = q[3 * i + 1], b[2] = q[3 * i + 2];
}

__global__ void __launch_bounds__(AL_BLOCK) k_al_prosac(const AlProblem* __restrict__ probs, const double* __restrict__ X1,
                                                        const double* __restrict__ X2, const int32_t* __restrict__ tabs, double thr,
                                                        int max_iterations, AlProsacOut* __restrict__ out) {
  __shared__ AlSmem sm;
  const AlProblem pb = probs[blockIdx.x];
  const int lane = threadIdx.x;
  const uint32_t N = pb.N;
  if (lane == 0) std_mt19937_seed(&sm.gen, pb.seed);
  int max_it = max_iterations, k = 0, iterations = 0;
  double best = DBL_MAX, rmin = INFINITY, cmin = INFINITY, pending = INFINITY;
  int best_cnt = 0;
  AlModel best_model;
  al_identity(&best_model);
  bool done = false;
  while (!done) {
    const int nb = min(AL_BLOCK, max_it - k);
    if (lane == 0) {
      for (int b = 0; b < nb; ++b) {
        const int e = tabs[pb.ntab + k + b];  // sample number k + b + 1
        const int n = e & 0x7fffffff;
        int* s = sm.samp[b];
        if (e < 0) {  // t_n_prime < k: 4 distinct of the top n
          for (int i = 0; i < 4; ++i) {
            int r;
            bool dup;
            do {
              r = (int)std_uniform_u32(&sm.gen, 0u, (uint32_t)(n - 1));
              dup = false;
              for (int q = 0; q < i; ++q) dup |= (s[q] == r);
            } while (dup);
            s[i] = r;
          }
        } else {  // 3 distinct of the top n - 1, then n
          for (int i = 0; i < 3; ++i) {
            int r;
            bool dup;
            do {
              r = (int)std_uniform_u32(&sm.gen, 0u, (uint32_t)(n - 2));
              dup = false;
              for (int q = 0; q < i; ++q) dup |= (s[q] == r);
            } while (dup);
            s[i] = r;
          }
          s[3] = n;
        }
      }
    }
    __syncthreads();
    AlModel m;
    double A[9];
    if (lane < nb) {
      double a[4][3], b[4][3];
      for (int q = 0; q < 4; ++q) al_load(X1 + 3 * (size_t)pb.off, X2 + 3 * (size_t)pb.off, pb.dir, (size_t)sm.samp[lane][q], a[q], b[q]);
      double m1[3], m2[3], sig[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, var3[3] = {0, 0, 0};
      for (int d = 0; d < 3; ++d) {
        m1[d] = (((a[0][d] + a[1][d]) + a[2][d]) + a[3][d]) * 0.25;
        m2[d] = (((b[0][d] + b[1][d]) + b[2][d]) + b[3][d]) * 0.25;
      }
      for (int q = 0; q < 4; ++q) {
        double d1[3], d2[3];
        for (int d = 0; d < 3; ++d) d1[d] = a[q][d] - m1[d], d2[d] = b[q][d] - m2[d];
        for (int r = 0; r < 3; ++r) {
          var3[r] += d1[r] * d1[r];
          for (int c = 0; c < 3; ++c) sig[r * 3 + c] += d2[r] * d1[c];
        }
      }
      for (int i = 0; i < 9; ++i) sig[i] = 0.25 * sig[i];
      const double var = ((var3[0] + var3[1]) + var3[2]) * 0.25;
      al_identity(&m);
      al_find_rts(m1, m2, sig, var, &m);
      for (int i = 0; i < 9; ++i) A[i] = m.s * m.R[i];
      sm.models[lane] = m;
    }
    double cost = 0.0, rm = INFINITY;
    int cnt = 0;
    for (uint32_t c0 = 0; c0 < N; c0 += AL_CHUNK) {
      const uint32_t len = min((uint32_t)AL_CHUNK, N - c0);
      if ((uint32_t)lane < len) al_load(X1 + 3 * (size_t)pb.off, X2 + 3 * (size_t)pb.off, pb.dir, (size_t)(c0 + lane), &sm.pts[lane][0], &sm.pts[lane][3]);
      __syncthreads();
      if (lane < nb)
        for (uint32_t i = 0; i < len; ++i) {
          const double* p = sm.pts[i];
          const double r = al_residual(A, m.t, p[0], p[1], p[2], p[3], p[4], p[5]);
          if (r < thr) {
            cost += r;
            ++cnt;
          } else {
            cost += thr;
          }
          rm = fmin(rm, fabs(r - thr));
        }
      __syncthreads();
    }
    if (lane < nb) {
      sm.cost[lane] = cost;
      sm.cnt[lane] = cnt;
      sm.rmarg[lane] = rm;
    }
    __syncthreads();
    if (lane == 0) {  // the serial loop over this batch
      for (int b = 0; b < nb; ++b) {
        rmin = fmin(rmin, sm.rmarg[b]);
        // the margin of the strict-best test where its outcome could matter: none between two costs without an
        // inlier (both N * thr); a near-tie of one inlier count leaves the cap alone and is moot once a clearly better model follows
        if (best != DBL_MAX && (sm.cnt[b] || best_cnt)) {
          const double mg = fabs(sm.cost[b] - best) / fmax(best, DBL_MIN);
          if (sm.cnt[b] != best_cnt)
            cmin = fmin(cmin, mg);
          else if (sm.cost[b] < best && mg >= kAlClearMargin)
            pending = INFINITY;
          else
            pending = fmin(pending, mg);
        }
        if (sm.cost[b] < best) {
          best = sm.cost[b];
          best_cnt = sm.cnt[b];
          best_model = sm.models[b];
          if (sm.cnt[b] >= 4) max_it = min(tabs[pb.mtab + sm.cnt[b]], max_it);
        }
        if (k + b + 1 >= max_it) {
          iterations = k + b + 1;
          done = true;
          break;
        }
      }
      if (!done) k += nb;
      sm.ctl[0] = done ? 1 : 0;
      sm.ctl[1] = k;
      sm.ctl[2] = max_it;
    }
    __syncthreads();
    done = sm.ctl[0] != 0;
    k = sm.ctl[1];
    max_it = sm.ctl[2];
    __syncthreads();
  }
  if (lane == 0) {
    AlProsacOut o;
    o.model = best_model;
    o.iterations = (uint32_t)iterations;
    o.pad = 0;
    o.residual_margin = rmin / thr;
    o.cost_margin = fmin(cmin, pending);
    o.best_cost = best;
    out[pb.slot] = o;
  }
}

// ---------------------------------------------------------------- refit + msd (FindSimilarityTransform after PROSAC)
struct AlRefitIn {
  uint32_t off, N, dir, prosac;  // prosac: 1 when a PROSAC model is in `model`
  AlModel model;                 // PROSAC's best (or the identity)
};
struct AlRefitOut {
  AlModel model;
  double msd;
  uint32_t inliers, pad;
};

// Umeyama over the selected correspondences (mask: residual of `ref` < thr, or all), FindRTS into m
__device__ void al_fit(const double* X1, const double* X2, const AlRefitIn& in, bool use_mask, const AlModel& ref, double thr,
                       double* sh, AlModel* m) {
  double A[9];
  for (int i = 0; i < 9; ++i) A[i] = ref.s * ref.R[i];
  double v[12];
  for (int q = 0; q < 7; ++q) v[q] = 0.0;
  for (uint32_t i = threadIdx.x; i < in.N; i += AL_BLOCK) {
    double a[3], b[3];
    al_load(X1, X2, in.dir, i, a, b);
    if (use_mask && !(al_residual(A, ref.t, a[0], a[1], a[2], b[0], b[1], b[2]) < thr)) continue;
    for (int d = 0; d < 3; ++d) v[d] += a[d], v[3 + d] += b[d];
    v[6] += 1.0;
  }
  block_sum<AL_BLOCK, 7>(v, sh);
  const double one_over_n = 1.0 / v[6];
  double m1[3], m2[3];
  for (int d = 0; d < 3; ++d) m1[d] = v[d] * one_over_n, m2[d] = v[3 + d] * one_over_n;
  for (int q = 0; q < 12; ++q) v[q] = 0.0;
  for (uint32_t i = threadIdx.x; i < in.N; i += AL_BLOCK) {
    double a[3], b[3];
    al_load(X1, X2, in.dir, i, a, b);
    if (use_mask && !(al_residual(A, ref.t, a[0], a[1], a[2], b[0], b[1], b[2]) < thr)) continue;
    double d1[3], d2[3];
    for (int d = 0; d < 3; ++d) d1[d] = a[d] - m1[d], d2[d] = b[d] - m2[d];
    for (int r = 0; r < 3; ++r) {
      v[9 + r] += d1[r] * d1[r];
      for (int c = 0; c < 3; ++c) v[r * 3 + c] += d2[r] * d1[c];
    }
  }
  block_sum<AL_BLOCK, 12>(v, sh);
  double sig[9];
  for (int i = 0; i < 9; ++i) sig[i] = one_over_n * v[i];
  const double var = ((v[9] + v[10]) + v[11]) * one_over_n;
  al_find_rts(m1, m2, sig, var, m);  // every lane the same inputs, the same model
}

__global__ void __launch_bounds__(AL_BLOCK) k_al_refit(const AlRefitIn* __restrict__ ins, const double* __restrict__ X1g,
                                                       const double* __restrict__ X2g, double thr, AlRefitOut* __restrict__ outs) {
  __shared__ double sh[12 * AL_BLOCK];
  const AlRefitIn in = ins[blockIdx.x];
  const double* X1 = X1g + 3 * (size_t)in.off;
  const double* X2 = X2g + 3 * (size_t)in.off;
  AlModel m = in.model;
  double v[1];
  uint32_t inliers = 0;
  bool no_edge = false;
  if (in.prosac) {
    double A[9];
    for (int i = 0; i < 9; ++i) A[i] = in.model.s * in.model.R[i];
    v[0] = 0.0;
    for (uint32_t i = threadIdx.x; i < in.N; i += AL_BLOCK) {
      double a[3], b[3];
      al_load(X1, X2, in.dir, i, a, b);
      if (al_residual(A, in.model.t, a[0], a[1], a[2], b[0], b[1], b[2]) < thr) v[0] += 1.0;
    }
    block_sum<AL_BLOCK, 1>(v, sh);
    inliers = (uint32_t)v[0];
    if (inliers >= 3) al_fit(X1, X2, in, true, in.model, thr, sh, &m);  // FindRTS returns at once below 3 columns
    if (inliers < 4) no_edge = true;
  }
  if (!no_edge && (!in.prosac || inliers <= 5) && in.N >= 3) al_fit(X1, X2, in, false, in.model, thr, sh, &m);
  double msd = DBL_MAX;
  if (!no_edge) {
    double A[9];
    for (int i = 0; i < 9; ++i) A[i] = m.s * m.R[i];
    v[0] = 0.0;
    for (uint32_t i = threadIdx.x; i < in.N; i += AL_BLOCK) {
      double a[3], b[3];
      al_load(X1, X2, in.dir, i, a, b);
      v[0] += al_residual(A, m.t, a[0], a[1], a[2], b[0], b[1], b[2]);
    }
    block_sum<AL_BLOCK, 1>(v, sh);
    msd = v[0] / (double)in.N;
  }
  if (threadIdx.x == 0) {
    AlRefitOut o;
    o.model = m;
    o.msd = msd;
    o.inliers = inliers;
    o.pad = 0;
    outs[blockIdx.x] = o;
  }
}

// ---------------------------------------------------------------- host: PROSAC tables
// ProsacSampler::Sample's n and branch for sample numbers 1 .. kmax (incremental: the loop over t is the same every call)
bool al_prosac_table(int N, int kmax, int32_t* out) {
  double t_n = 20000.0;
  int n = 4;
  for (int i = 0; i < 4; ++i) t_n *= static_cast<double>(n - i) / (N - i);
  double t_n_prime = 1.0;
  for (int t = 1; t <= kmax; ++t) {
    if (t > t_n_prime && n < N) {
      const double t_n_plus1 = (t_n * (n + 1.0)) / (n + 1.0 - 4);
      t_n_prime += std::ceil(t_n_plus1 - t_n);
      t_n = t_n_plus1;
      n++;
    }
    out[t - 1] = n | ((t_n_prime < t) ? (int32_t)0x80000000 : 0);
    if (n > N - 1) return false;  // the sampler would index past the data (not reached for kmax <= 5000)
  }
  return true;
}
// SampleConsensusEstimator::ComputeMaxIterations(4, c / N, log(failure_probability)) for c = 0 .. N
void al_max_iter_table(int N, const dsm_align_options& o, int32_t* out) {
  const double log_failure_prob = std::log(o.failure_probability);
  out[0] = o.max_iterations;  // never read: a count below 4 does not update the cap
  for (int c = 1; c <= N; ++c) {
    const double r = static_cast<double>(c) / static_cast<double>(N);
    if (r == 1.0) {
      out[c] = o.min_iterations;
      continue;
    }
    const double log_prob = std::log(1.0 - std::pow(r, 4.0)) - std::numeric_limits<double>::epsilon();
    const double num = log_failure_prob / log_prob;
    out[c] = static_cast<int>(std::max(static_cast<double>(o.min_iterations), std::min(num, static_cast<double>(o.max_iterations))));
  }
}

struct AlSim3 {
  double s, R[9], t[3];
};
AlSim3 al_sim3_identity() {
  AlSim3 a{};
  a.s = 1.0;
  a.R[0] = a.R[4] = a.R[8] = 1.0;
  return a;
}

struct AlBufs {
  DevBuf obs_off, obs, pt_off, pcl, reg, head, rid, hpos, key, key2, val, val2, ocl, opt, flags, ids, pkey, pkey2, pval, pval2, rank, cnt, coff;
  DevBuf ckey, ckey2, cval, cval2, csrc, cref, xyz, X1, X2, heads, nheads, tmp, tabs, probs, pout, rin, rout;
};

}  // namespace

extern "C" void dsm_default_align_options(dsm_align_options* o) {
  o->threshold = 0.1;               // AlignOptions::threshold (sfm_aligner.h)
  o->max_reprojection_error = 1.8;  // AlignOptions::max_reprojection_error
  o->failure_probability = 0.01;    // RansacParameters
  o->min_iterations = 100;
  o->max_iterations = 5000;         // RansacSimilarity
  o->random_seed = 0;
  o->reserved = 0;
}

extern "C" uint32_t dsm_align_seed(uint32_t i, uint32_t j, uint32_t direction, uint32_t user_seed) {
  return dsm_pair_seed(i, j, user_seed) ^ (direction ? 0x85ebca6bu : 0u);
}

extern "C" int dsm_align_clusters(dsm_ctx* ctx, uint32_t K, const uint32_t* image_offsets, const uint32_t* image_ids,
                                  const uint32_t* point_offsets, const uint64_t* point_ids, const double* point_xyz,
                                  const uint32_t* obs_offsets, const uint32_t* obs, const dsm_align_options* options,
                                  const uint32_t* seeds, dsm_align_pair* pairs_out, uint32_t pairs_capacity, uint32_t* n_pairs_out,
                                  int32_t* anchor_out, uint8_t* in_component, int32_t* mst_parent, double* sim3_to_anchor,
                                  uint32_t* separators, uint32_t* n_separators_out, dsm_align_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](int code, const char* msg) { return dsm_fail(ctx, code, "dsm_align_clusters", msg); };
  if (K == 0 || K > 65536) return fail(DSM_ERR_INVALID_ARGUMENT, "num_clusters must be in [1, 65536]");
  if (!image_offsets || !point_offsets || !obs_offsets || !n_pairs_out || !anchor_out || !in_component || !mst_parent ||
      !sim3_to_anchor || !n_separators_out || (pairs_capacity && !pairs_out))
    return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  for (uint32_t c = 0; c < K; ++c)
    if (image_offsets[c + 1] < image_offsets[c] || point_offsets[c + 1] < point_offsets[c] || obs_offsets[c + 1] < obs_offsets[c])
      return fail(DSM_ERR_INVALID_ARGUMENT, "offsets must be non-decreasing");
  if (image_offsets[0] || point_offsets[0] || obs_offsets[0]) return fail(DSM_ERR_INVALID_ARGUMENT, "offsets must start at 0");
  const uint32_t R = image_offsets[K], P = point_offsets[K], M = obs_offsets[K];
  if ((R && !image_ids) || (P && (!point_ids || !point_xyz)) || (M && !obs) || (R && !separators))
    return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  dsm_align_options o;
  if (options)
    o = *options;
  else
    dsm_default_align_options(&o);
  if (!std::isfinite(o.threshold)) return fail(DSM_ERR_INVALID_ARGUMENT, "non-finite threshold");
  if (!(o.threshold > 0.0) || !(o.failure_probability > 0.0 && o.failure_probability < 1.0) || !(o.max_reprojection_error >= 0.0) ||
      o.min_iterations < 0 || o.max_iterations < 1 || o.max_iterations < o.min_iterations || o.max_iterations > kAlMaxIterationsCap)
    return fail(DSM_ERR_INVALID_ARGUMENT, "option out of range");
  auto flags_fail = [&](uint32_t flags) {
    if (flags & kAlFlagUnregistered) return fail(DSM_ERR_INVALID_ARGUMENT, "an observation on an image its cluster has not registered");
    if (flags & kAlFlagPointRange) return fail(DSM_ERR_INVALID_ARGUMENT, "a point index out of range");
    if (flags & kAlFlagDuplicateObs) return fail(DSM_ERR_INVALID_ARGUMENT, "a repeated (image_id, point2D_idx) inside one cluster");
    return fail(DSM_ERR_INVALID_ARGUMENT, "a repeated point id inside one cluster");
  };
  if (M >= 0x80000000u || P >= 0x80000000u) return fail(DSM_ERR_INVALID_ARGUMENT, "too many points or observations");
  // a NaN or an infinite coordinate would reach the SVD of every trial that samples it: refused here, before the first launch
  for (size_t q = 0; q < 3 * (size_t)P; ++q)
    if (!std::isfinite(point_xyz[q])) return fail(DSM_ERR_INVALID_ARGUMENT, "non-finite point_xyz");
  dsm_align_report rep{};
  rep.num_clusters = K;
  rep.num_observations = M;
  rep.min_residual_margin = rep.min_cost_margin = rep.min_weight_margin = INFINITY;

  // ------------------------------------------------------------ registered images: common images and separators (host)
  std::vector<uint64_t> reg(R);
  for (uint32_t c = 0; c < K; ++c)
    for (uint32_t r = image_offsets[c]; r < image_offsets[c + 1]; ++r) reg[r] = ((uint64_t)image_ids[r] << 32) | c;
  std::sort(reg.begin(), reg.end());
  reg.erase(std::unique(reg.begin(), reg.end()), reg.end());
  std::map<uint64_t, uint32_t> common;  // i * K + j -> common registered images
  std::vector<uint32_t> seps;
  for (size_t a = 0; a < reg.size();) {
    size_t b = a;
    while (b < reg.size() && (reg[b] >> 32) == (reg[a] >> 32)) ++b;
    if (b - a >= 2) seps.push_back((uint32_t)(reg[a] >> 32));
    for (size_t x = a; x < b; ++x)
      for (size_t y = x + 1; y < b; ++y) common[(reg[x] & 0xffffffffu) * (uint64_t)K + (reg[y] & 0xffffffffu)]++;
    a = b;
  }

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return fail(DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  AlBufs d;
  DevEvents<4> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));

  // ------------------------------------------------------------ the join (device)
  std::vector<std::pair<uint32_t, uint32_t>> heads;  // (pair key, first correspondence)
  uint64_t C = 0;
  const size_t P1 = std::max<uint32_t>(P, 1);
  HIPCHK(ctx, d.flags.reserve(8));
  HIPCHK(ctx, hipMemsetAsync(d.flags.p, 0, 8, st));
  HIPCHK(ctx, d.pt_off.reserve(((size_t)K + 1) * 4));
  HIPCHK(ctx, hipMemcpyAsync(d.pt_off.p, point_offsets, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, d.xyz.reserve(P1 * 24));
  HIPCHK(ctx, d.rank.reserve(P1 * 4));
  if (P) {
    HIPCHK(ctx, hipMemcpyAsync(d.xyz.p, point_xyz, (size_t)P * 24, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, d.ids.reserve((size_t)P * 8));
    HIPCHK(ctx, d.pkey2.reserve((size_t)P * 8));
    HIPCHK(ctx, d.pval.reserve((size_t)P * 4));
    HIPCHK(ctx, d.pval2.reserve((size_t)P * 4));
    HIPCHK(ctx, d.pkey.reserve((size_t)P * 4));
    HIPCHK(ctx, hipMemcpyAsync(d.ids.p, point_ids, (size_t)P * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_al_iota, dim3((P + 255) / 256), dim3(256), 0, st, P, d.pval.as<uint32_t>());
    size_t tb = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, d.ids.as<uint64_t>(), d.pkey2.as<uint64_t>(), d.pval.as<uint32_t>(), d.pval2.as<uint32_t>(),
                                          (size_t)P, 0, 64, st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::radix_sort_pairs(d.tmp.p, tb, d.ids.as<uint64_t>(), d.pkey2.as<uint64_t>(), d.pval.as<uint32_t>(), d.pval2.as<uint32_t>(),
                                          (size_t)P, 0, 64, st));
    hipLaunchKernelGGL(k_al_point_cluster, dim3((P + 255) / 256), dim3(256), 0, st, P, K, d.pt_off.as<uint32_t>(), d.pval2.as<uint32_t>(),
                       d.pkey.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    int kb = 1;
    while (kb < 32 && (1ull << kb) <= K) ++kb;
    // then stably by cluster: ascending id inside each cluster
    HIPCHK(ctx, d.pcl.reserve((size_t)P * 4));
    tb = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, d.pkey.as<uint32_t>(), d.pcl.as<uint32_t>(), d.pval2.as<uint32_t>(), d.pval.as<uint32_t>(),
                                          (size_t)P, 0, (unsigned)kb, st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::radix_sort_pairs(d.tmp.p, tb, d.pkey.as<uint32_t>(), d.pcl.as<uint32_t>(), d.pval2.as<uint32_t>(), d.pval.as<uint32_t>(),
                                          (size_t)P, 0, (unsigned)kb, st));
    hipLaunchKernelGGL(k_al_point_rank, dim3((P + 255) / 256), dim3(256), 0, st, P, d.pt_off.as<uint32_t>(), d.pcl.as<uint32_t>(),
                       d.pval.as<uint32_t>(), d.ids.as<uint64_t>(), d.rank.as<uint32_t>(), d.flags.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  if (M) {
    HIPCHK(ctx, d.obs_off.reserve(((size_t)K + 1) * 4));
    HIPCHK(ctx, d.obs.reserve((size_t)M * 12));
    HIPCHK(ctx, d.reg.reserve(std::max<size_t>(reg.size(), 1) * 8));
    for (DevBuf* b : {&d.key, &d.key2, &d.cnt, &d.coff}) HIPCHK(ctx, b->reserve((size_t)M * 8));
    for (DevBuf* b : {&d.val, &d.val2, &d.ocl, &d.opt}) HIPCHK(ctx, b->reserve((size_t)M * 4));
    HIPCHK(ctx, hipMemcpyAsync(d.obs_off.p, obs_offsets, ((size_t)K + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d.obs.p, obs, (size_t)M * 12, hipMemcpyHostToDevice, st));
    if (!reg.empty()) HIPCHK(ctx, hipMemcpyAsync(d.reg.p, reg.data(), reg.size() * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_al_obs_prep, dim3((M + 255) / 256), dim3(256), 0, st, M, K, d.obs_off.as<uint32_t>(), d.obs.as<uint32_t>(),
                       d.pt_off.as<uint32_t>(), d.reg.as<uint64_t>(), (uint32_t)reg.size(), d.key.as<uint64_t>(), d.val.as<uint32_t>(),
                       d.ocl.as<uint32_t>(), d.opt.as<uint32_t>(), d.flags.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    size_t tb = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, d.key.as<uint64_t>(), d.key2.as<uint64_t>(), d.val.as<uint32_t>(), d.val2.as<uint32_t>(),
                                          (size_t)M, 0, 64, st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::radix_sort_pairs(d.tmp.p, tb, d.key.as<uint64_t>(), d.key2.as<uint64_t>(), d.val.as<uint32_t>(), d.val2.as<uint32_t>(),
                                          (size_t)M, 0, 64, st));
    HIPCHK(ctx, d.head.reserve((size_t)M * 4));
    HIPCHK(ctx, d.rid.reserve((size_t)M * 4));
    HIPCHK(ctx, d.hpos.reserve((size_t)M * 4));
    hipLaunchKernelGGL(k_al_heads, dim3((M + 255) / 256), dim3(256), 0, st, M, d.key2.as<uint64_t>(), d.val2.as<uint32_t>(), d.ocl.as<uint32_t>(),
                       d.head.as<uint32_t>(), d.flags.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    // every input check is in the flags now: refuse before the work that grows with the runs
    uint32_t flags = 0;
    HIPCHK(ctx, hipMemcpyAsync(&flags, d.flags.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (flags) return flags_fail(flags);
    tb = 0;
    HIPCHK(ctx, rocprim::inclusive_scan(nullptr, tb, d.head.as<uint32_t>(), d.rid.as<uint32_t>(), (size_t)M, rocprim::plus<uint32_t>(), st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::inclusive_scan(d.tmp.p, tb, d.head.as<uint32_t>(), d.rid.as<uint32_t>(), (size_t)M, rocprim::plus<uint32_t>(), st));
    hipLaunchKernelGGL(k_al_head_pos, dim3((M + 255) / 256), dim3(256), 0, st, M, d.head.as<uint32_t>(), d.rid.as<uint32_t>(),
                       d.hpos.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_al_count, dim3((M + 255) / 256), dim3(256), 0, st, M, d.rid.as<uint32_t>(), d.hpos.as<uint32_t>(), d.cnt.as<uint64_t>());
    HIPCHK(ctx, hipGetLastError());
    tb = 0;
    HIPCHK(ctx, rocprim::exclusive_scan(nullptr, tb, d.cnt.as<uint64_t>(), d.coff.as<uint64_t>(), (uint64_t)0, (size_t)M, rocprim::plus<uint64_t>(), st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::exclusive_scan(d.tmp.p, tb, d.cnt.as<uint64_t>(), d.coff.as<uint64_t>(), (uint64_t)0, (size_t)M, rocprim::plus<uint64_t>(), st));
    uint64_t last[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(&last[0], d.coff.as<uint64_t>() + (M - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(&last[1], d.cnt.as<uint64_t>() + (M - 1), 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    C = last[0] + last[1];
  }
  if (!M) {  // the point checks ran without observations
    uint32_t flags = 0;
    HIPCHK(ctx, hipMemcpyAsync(&flags, d.flags.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (flags) return flags_fail(flags);
  }
  if (C >= 0x80000000ull) return fail(DSM_ERR_INVALID_ARGUMENT, "more than 2^31 correspondences");
  rep.num_correspondences = C;
  const size_t C1 = std::max<uint64_t>(C, 1);
  HIPCHK(ctx, d.X1.reserve(C1 * 24));
  HIPCHK(ctx, d.X2.reserve(C1 * 24));
  if (C) {
    for (DevBuf* b : {&d.ckey, &d.ckey2}) HIPCHK(ctx, b->reserve(C * 8));
    for (DevBuf* b : {&d.cval, &d.cval2, &d.csrc, &d.cref}) HIPCHK(ctx, b->reserve(C * 4));
    HIPCHK(ctx, d.heads.reserve(C * 8));
    HIPCHK(ctx, d.nheads.reserve(4));
    HIPCHK(ctx, hipMemsetAsync(d.nheads.p, 0, 4, st));
    hipLaunchKernelGGL(k_al_emit, dim3((M + 255) / 256), dim3(256), 0, st, M, K, d.cnt.as<uint64_t>(), d.val2.as<uint32_t>(), d.ocl.as<uint32_t>(),
                       d.opt.as<uint32_t>(), d.rank.as<uint32_t>(), d.coff.as<uint64_t>(), d.ckey.as<uint64_t>(), d.cval.as<uint32_t>(),
                       d.csrc.as<uint32_t>(), d.cref.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    size_t tb = 0;
    HIPCHK(ctx, rocprim::radix_sort_pairs(nullptr, tb, d.ckey.as<uint64_t>(), d.ckey2.as<uint64_t>(), d.cval.as<uint32_t>(), d.cval2.as<uint32_t>(),
                                          (size_t)C, 0, 64, st));
    HIPCHK(ctx, d.tmp.reserve(std::max<size_t>(tb, 16)));
    HIPCHK(ctx, rocprim::radix_sort_pairs(d.tmp.p, tb, d.ckey.as<uint64_t>(), d.ckey2.as<uint64_t>(), d.cval.as<uint32_t>(), d.cval2.as<uint32_t>(),
                                          (size_t)C, 0, 64, st));
    hipLaunchKernelGGL(k_al_gather, dim3((uint32_t)((C + 255) / 256)), dim3(256), 0, st, (uint32_t)C, d.ckey2.as<uint64_t>(), d.cval2.as<uint32_t>(),
                       d.csrc.as<uint32_t>(), d.cref.as<uint32_t>(), d.xyz.as<double>(), d.X1.as<double>(), d.X2.as<double>(),
                       d.heads.as<uint32_t>(), d.nheads.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    uint32_t nh = 0;
    HIPCHK(ctx, hipMemcpyAsync(&nh, d.nheads.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    std::vector<uint32_t> hh((size_t)nh * 2);
    if (nh) HIPCHK(ctx, hipMemcpyAsync(hh.data(), d.heads.p, (size_t)nh * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (uint32_t h = 0; h < nh; ++h) heads.emplace_back(hh[2 * h], hh[2 * h + 1]);
    std::sort(heads.begin(), heads.end());
  }
  HIPCHK(ctx, hipEventRecord(ev[1], st));

  // ------------------------------------------------------------ pairs with >= 2 common images, PROSAC problems
  struct PairW {
    uint32_t i, j, common, off, N;
  };
  std::vector<PairW> pw;
  {
    std::map<uint32_t, std::pair<uint32_t, uint32_t>> corr;  // pair key -> (off, N)
    for (size_t h = 0; h < heads.size(); ++h) {
      const uint64_t end = h + 1 < heads.size() ? heads[h + 1].second : C;
      corr[heads[h].first] = {heads[h].second, (uint32_t)(end - heads[h].second)};
    }
    for (const auto& kv : common) {
      if (kv.second < 2) continue;
      PairW p{(uint32_t)(kv.first / K), (uint32_t)(kv.first % K), kv.second, 0, 0};
      auto it = corr.find((uint32_t)kv.first);
      if (it != corr.end()) p.off = it->second.first, p.N = it->second.second;
      pw.push_back(p);
    }
  }
  const uint32_t NP = (uint32_t)pw.size();
  rep.num_pairs = NP;
  std::vector<int32_t> tabs;
  std::map<uint32_t, std::pair<uint32_t, uint32_t>> tab_of;  // N -> (ntab, mtab)
  std::vector<AlProblem> probs;
  for (uint32_t p = 0; p < NP; ++p) {
    if (pw[p].N <= 5) continue;
    const uint32_t N = pw[p].N;
    if (!tab_of.count(N)) {
      const uint32_t nt = (uint32_t)tabs.size();
      tabs.resize(nt + (size_t)o.max_iterations + N + 1);
      if (!al_prosac_table((int)N, o.max_iterations, tabs.data() + nt))
        return fail(DSM_ERR_INVALID_ARGUMENT, "PROSAC's sample index would pass N - 1 (max_iterations too large)");
      al_max_iter_table((int)N, o, tabs.data() + nt + o.max_iterations);
      tab_of[N] = {nt, nt + (uint32_t)o.max_iterations};
    }
    for (uint32_t dir = 0; dir < 2; ++dir) {
      const uint32_t a = dir ? pw[p].j : pw[p].i, b = dir ? pw[p].i : pw[p].j;
      AlProblem q{pw[p].off, N, dir, seeds ? seeds[(size_t)a * K + b] : dsm_align_seed(pw[p].i, pw[p].j, dir, o.random_seed),
                  tab_of[N].first, tab_of[N].second, 2 * p + dir, 0};
      probs.push_back(q);
    }
  }
  // the queue: largest N first (ties in pair order), one workgroup each
  std::stable_sort(probs.begin(), probs.end(), [](const AlProblem& l, const AlProblem& r) { return l.N > r.N; });
  rep.num_prosac_problems = (uint32_t)probs.size();
  std::vector<AlProsacOut> pout((size_t)NP * 2);
  if (!probs.empty()) {
    HIPCHK(ctx, d.tabs.reserve(tabs.size() * 4));
    HIPCHK(ctx, d.probs.reserve(probs.size() * sizeof(AlProblem)));
    HIPCHK(ctx, d.pout.reserve(pout.size() * sizeof(AlProsacOut)));
    HIPCHK(ctx, hipMemcpyAsync(d.tabs.p, tabs.data(), tabs.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d.probs.p, probs.data(), probs.size() * sizeof(AlProblem), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_al_prosac, dim3((uint32_t)probs.size()), dim3(AL_BLOCK), 0, st, d.probs.as<AlProblem>(), d.X1.as<double>(),
                       d.X2.as<double>(), d.tabs.as<int32_t>(), o.threshold, o.max_iterations, d.pout.as<AlProsacOut>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(pout.data(), d.pout.p, pout.size() * sizeof(AlProsacOut), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  // ------------------------------------------------------------ refit + msd for every direction with N >= 3
  HIPCHK(ctx, hipStreamSynchronize(st));
  std::vector<AlRefitIn> rin;
  std::vector<uint32_t> rslot;
  for (uint32_t p = 0; p < NP; ++p) {
    if (pw[p].N < 3) continue;
    for (uint32_t dir = 0; dir < 2; ++dir) {
      AlRefitIn in{};
      in.off = pw[p].off, in.N = pw[p].N, in.dir = dir, in.prosac = pw[p].N > 5;
      if (in.prosac) {
        in.model = pout[2 * p + dir].model;
      } else {
        in.model.s = 1.0;
        in.model.R[0] = in.model.R[4] = in.model.R[8] = 1.0;
      }
      rin.push_back(in);
      rslot.push_back(2 * p + dir);
    }
  }
  std::vector<AlRefitOut> rout(rin.size());
  if (!rin.empty()) {
    HIPCHK(ctx, d.rin.reserve(rin.size() * sizeof(AlRefitIn)));
    HIPCHK(ctx, d.rout.reserve(rin.size() * sizeof(AlRefitOut)));
    HIPCHK(ctx, hipMemcpyAsync(d.rin.p, rin.data(), rin.size() * sizeof(AlRefitIn), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_al_refit, dim3((uint32_t)rin.size()), dim3(AL_BLOCK), 0, st, d.rin.as<AlRefitIn>(), d.X1.as<double>(), d.X2.as<double>(),
                       o.threshold, d.rout.as<AlRefitOut>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(rout.data(), d.rout.p, rin.size() * sizeof(AlRefitOut), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, ev.ms(0, 1, &rep.join_ms));
  HIPCHK(ctx, ev.ms(1, 2, &rep.prosac_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rep.refit_ms));
  rep.device_ms = rep.join_ms + rep.prosac_ms + rep.refit_ms;

  // ------------------------------------------------------------ pair records
  std::vector<dsm_align_pair> out(NP);
  std::vector<AlSim3> sim(2 * (size_t)NP);
  for (uint32_t p = 0; p < NP; ++p) {
    dsm_align_pair& q = out[p];
    q = dsm_align_pair{};
    q.i = pw[p].i, q.j = pw[p].j, q.num_common_images = pw[p].common, q.num_correspondences = pw[p].N;
    q.msd[0] = q.msd[1] = q.weight = NAN;
    for (int dir = 0; dir < 2; ++dir) {
      sim[2 * p + dir] = al_sim3_identity();
      q.prosac_cost[dir] = NAN;
      q.prosac_s[dir] = 1.0;
      q.prosac_R[dir][0] = q.prosac_R[dir][4] = q.prosac_R[dir][8] = 1.0;
      if (pw[p].N > 5) {
        const AlProsacOut& po = pout[2 * p + dir];
        q.prosac_cost[dir] = po.best_cost;
        q.prosac_s[dir] = po.model.s;
        std::copy(po.model.R, po.model.R + 9, q.prosac_R[dir]);
        std::copy(po.model.t, po.model.t + 3, q.prosac_t[dir]);
        q.iterations[dir] = pout[2 * p + dir].iterations;
        rep.prosac_iterations += pout[2 * p + dir].iterations;
        rep.min_residual_margin = std::min(rep.min_residual_margin, pout[2 * p + dir].residual_margin);
        rep.min_cost_margin = std::min(rep.min_cost_margin, pout[2 * p + dir].cost_margin);
      }
    }
  }
  for (size_t r = 0; r < rin.size(); ++r) {
    const uint32_t p = rslot[r] / 2, dir = rslot[r] % 2;
    dsm_align_pair& q = out[p];
    const AlRefitOut& ro = rout[r];
    q.num_inliers[dir] = ro.inliers;
    q.msd[dir] = ro.msd;
    q.s[dir] = ro.model.s;
    for (int i = 0; i < 9; ++i) q.R[dir][i] = ro.model.R[i];
    for (int i = 0; i < 3; ++i) q.t[dir][i] = ro.model.t[i];
    AlSim3& sm = sim[rslot[r]];
    sm.s = ro.model.s;
    std::copy(ro.model.R, ro.model.R + 9, sm.R);
    std::copy(ro.model.t, ro.model.t + 3, sm.t);
  }
  struct Edge {
    float w;
    uint32_t i, j, p;
  };
  std::vector<Edge> edges;
  for (uint32_t p = 0; p < NP; ++p) {
    dsm_align_pair& q = out[p];
    if (q.num_correspondences < 3) continue;
    q.weight = std::max(q.msd[0], q.msd[1]);
    if (std::isnan(q.msd[0]) || std::isnan(q.msd[1]) || q.weight == DBL_MAX) continue;
    rep.min_weight_margin = std::min(rep.min_weight_margin, std::fabs(q.weight - o.max_reprojection_error) / o.max_reprojection_error);
    if (q.weight > o.max_reprojection_error) continue;
    q.edge = 1;
    edges.push_back({(float)q.weight, q.i, q.j, p});
  }
  rep.num_edges = (uint32_t)edges.size();

  // ------------------------------------------------------------ the largest component (ties: the smaller cluster index)
  std::vector<uint32_t> uf(K);
  std::iota(uf.begin(), uf.end(), 0u);
  auto find = [&](uint32_t x) {
    while (uf[x] != x) x = uf[x] = uf[uf[x]];
    return x;
  };
  for (const Edge& e : edges) {
    const uint32_t a = find(e.i), b = find(e.j);
    if (a != b) uf[std::max(a, b)] = std::min(a, b);  // a root is the smallest index of its component
  }
  std::vector<uint32_t> size(K, 0);
  for (uint32_t c = 0; c < K; ++c) size[find(c)]++;
  uint32_t root = 0;
  for (uint32_t c = 0; c < K; ++c)
    if (size[c] > size[root]) root = c;
  std::vector<uint8_t> inc(K, 0);
  for (uint32_t c = 0; c < K; ++c) inc[c] = find(c) == root;
  rep.num_in_component = size[root];

  // ------------------------------------------------------------ Kruskal (ties: (min, max) ascending)
  std::vector<Edge> ce;
  for (const Edge& e : edges)
    if (inc[e.i]) ce.push_back(e);
  std::sort(ce.begin(), ce.end(), [](const Edge& l, const Edge& r) {
    if (l.w != r.w) return l.w < r.w;
    if (l.i != r.i) return l.i < r.i;
    return l.j < r.j;
  });
  std::iota(uf.begin(), uf.end(), 0u);
  std::vector<std::vector<std::pair<uint32_t, uint32_t>>> adj(K);  // (neighbour, pair)
  for (const Edge& e : ce) {
    const uint32_t a = find(e.i), b = find(e.j);
    if (a == b) continue;
    uf[a] = b;
    adj[e.i].push_back({e.j, e.p});
    adj[e.j].push_back({e.i, e.p});
  }
  // ------------------------------------------------------------ FindAnchorNode: leaves layer by layer
  std::vector<int32_t> parent(K, -1);
  std::vector<uint32_t> deg(K, 0);
  uint32_t alive = 0;
  for (uint32_t c = 0; c < K; ++c) {
    deg[c] = (uint32_t)adj[c].size();
    if (deg[c]) ++alive;
  }
  std::vector<uint8_t> gone(K, 0);
  uint32_t anchor = 0;
  auto remove_leaf = [&](uint32_t c) {
    for (const auto& nb : adj[c])
      if (!gone[nb.first]) {
        parent[c] = (int32_t)nb.first;
        anchor = nb.first;
        deg[nb.first]--;
        break;
      }
    gone[c] = 1;
    --alive;
  };
  while (alive > 1) {
    std::vector<uint32_t> leaves;
    if (alive == 2) {
      for (uint32_t c = 0; c < K && leaves.empty(); ++c)
        if (deg[c] && !gone[c]) leaves.push_back(c);  // the smaller index goes, the larger is the anchor
    } else {
      for (uint32_t c = 0; c < K; ++c)
        if (!gone[c] && deg[c] == 1) leaves.push_back(c);
    }
    if (leaves.empty()) break;
    for (uint32_t c : leaves) remove_leaf(c);
  }
  // ------------------------------------------------------------ ComputePath: compose up to the anchor
  auto edge_sim = [&](uint32_t a, uint32_t b) -> const AlSim3& {  // sim3_graph_[a][b]
    const uint32_t i = std::min(a, b), j = std::max(a, b);
    uint32_t lo = 0, hi = NP;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (pw[mid].i < i || (pw[mid].i == i && pw[mid].j < j)) lo = mid + 1; else hi = mid;
    }
    return sim[2 * lo + (a < b ? 0 : 1)];
  };
  for (uint32_t c = 0; c < K; ++c) {
    AlSim3 a = al_sim3_identity();
    if (inc[c] && c != anchor) {
      for (uint32_t u = c; u != anchor && parent[u] >= 0; u = (uint32_t)parent[u]) {
        const AlSim3& e = edge_sim(u, (uint32_t)parent[u]);
        AlSim3 n;
        n.s = e.s * a.s;
        double sR[9];
        for (int i = 0; i < 9; ++i) sR[i] = e.s * e.R[i];
        for (int i = 0; i < 3; ++i) {
          for (int j = 0; j < 3; ++j) n.R[i * 3 + j] = e.R[i * 3] * a.R[j] + e.R[i * 3 + 1] * a.R[3 + j] + e.R[i * 3 + 2] * a.R[6 + j];
          n.t[i] = (sR[i * 3] * a.t[0] + sR[i * 3 + 1] * a.t[1] + sR[i * 3 + 2] * a.t[2]) + e.t[i];
        }
        a = n;
      }
    }
    double* o13 = sim3_to_anchor + 13 * (size_t)c;
    o13[0] = a.s;
    std::copy(a.R, a.R + 9, o13 + 1);
    std::copy(a.t, a.t + 3, o13 + 10);
    in_component[c] = inc[c];
    mst_parent[c] = inc[c] ? parent[c] : -1;
  }
  *anchor_out = (int32_t)anchor;
  for (uint32_t p = 0; p < std::min(NP, pairs_capacity); ++p) pairs_out[p] = out[p];
  *n_pairs_out = NP;
  std::copy(seps.begin(), seps.end(), separators);
  *n_separators_out = (uint32_t)seps.size();
  rep.num_separators = (uint32_t)seps.size();
  if (report) *report = rep;
  return DSM_OK;
}
