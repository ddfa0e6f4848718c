// vocabulary_build.hip -- training the vocabulary tree on the device: VisualIndex::Quantize
// (/root/reference/src/retrieval/visual_index.h:623-665), i.e. flann::hierarchicalClustering<L2<uint8_t>> with KMEANSPP seeding
// (lib/FLANN/algorithms/kmeans_index.h:329-345, 496-530, 544-713, 928-969; center_chooser.h:224-290; dist.h:149-177), and
// InvertedIndex::ComputeHammingEmbedding (src/retrieval/inverted_index.h:184-217, inverted_file.h:275-291, util/math.h:211-229).
// The result is the reference's bit for bit for the same stream of rand() values.
//
// One clustered node is a job: a range [off, off + m) of the indices permutation.  Its phases are device functions over chunks of
// 256 points, called in two forms:
//   whole-chip form   one launch per phase, a block per chunk (k_vb_seed, k_vb_select, k_vb_assign, ...); the host reads one
//                     flag per Lloyd iteration
//   workgroup form    k_vb_node: a block per job runs every phase itself, looping over the chunks; a batch of depth-first
//                     consecutive jobs whose number of draws is known beforehand goes out in one launch
// Phases:
//   seed      exact integer distances to the newest centre (v_dot4), the running minimum, the chunk's sum of it
//   select    the k-means++ draw: the first index whose inclusive prefix sum of the minima reaches rand * pot -- a scan of the
//             chunk sums, then of one chunk (the reference's subtractive walk takes integers from a double below 2^53: exact)
//   assign    a lane per point, the double centres staged through LDS 16 at a time; dist.h's float sum, four terms at a time,
//             no contraction; strict argmin; counts, radii (integer atomic max of the float bits) and the changed flag
//   accumulate / update   integer sums per (centre, dimension) in 64-bit atomics, times 1.0 / count in double
//   repair    the empty-cluster loop as written, the search for the first member of the donor cluster block-wide
//   distance  float distance of every point to its float-cast centre, for the children's variance
// The order-dependent pieces run on the host over what the device computed: the swap partition (kmeans_index.h:694-699) with the
// variance chain in the order it visits the points, the root's float mean chain, getMinVarianceClusters.  Draws are taken on
// the host in the reference's order; the device turns them into indices.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "ctx.h"

namespace {

constexpr int VB_CHUNK = 256;         // points of one chunk = threads of one block
constexpr int VB_TILE = 16;           // double centres staged in LDS at a time (16 KiB)
constexpr uint32_t VB_MAX_SLOTS = 64; // jobs of one batch
// the default switch between the forms: the nodes that can be batched (fewer than 2 * branching - 1 points), and at least one
// chunk -- a launch per phase gains nothing on a single chunk.  Measured at branching 256: a workgroup alone on a
// 1 024-point node is slower than the whole-chip form.
inline uint32_t vb_default_workgroup_node_max(int branching) { return (uint32_t)std::max(2 * branching - 2, VB_CHUNK); }
constexpr int32_t VB_MAX_BRANCHING = 4096;

struct VbJob {
  uint32_t off, m;        // the job's range of the indices permutation
  uint32_t csum_off;      // its chunk sums
  uint32_t reserved;
};

struct VbArgs {
  const uint8_t* desc;     // [n][128]
  const int32_t* idx;      // [n] the indices permutation
  int32_t* belongs;        // [n] by position
  uint32_t* closest;       // [n] by position: closestDistSq as integers
  float* dist;             // [n] by position: distance to the float centre
  const VbJob* jobs;       // [slots]
  unsigned long long* csum;
  const int32_t* draws;    // [slots][b] rand() values
  int32_t* cidx;           // [slots][b] positions of the seeds inside the job
  double* dcent;           // [slots][b][128]
  unsigned long long* sums;  // [slots][b][128]
  int32_t* counts;         // [slots][b] atomically counted by assign
  int32_t* cnt_final;      // [slots][b] after the repair
  uint32_t* radii;         // [slots][b] float bits
  int32_t* changed;        // [slots]
  float* centf;            // [slots][b][128]
  int32_t b, iterations;
};

template <typename T>
__device__ __forceinline__ T ld_agent(const T* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
template <typename T>
__device__ __forceinline__ void st_agent(T* p, T v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void load_row(const uint8_t* row, uint32_t a[32]) {
  const uint4* r = reinterpret_cast<const uint4*>(row);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = r[q];
    a[4 * q] = v.x;
    a[4 * q + 1] = v.y;
    a[4 * q + 2] = v.z;
    a[4 * q + 3] = v.w;
  }
}

// sum of (a - b)^2 over 128 bytes = |a|^2 + |b|^2 - 2 a.b, exact in uint32 (<= 128 * 255^2)
__device__ __forceinline__ uint32_t dist_u8(const uint32_t a[32], uint32_t aa, const uint8_t* brow) {
  const uint4* r = reinterpret_cast<const uint4*>(brow);
  uint32_t ab = 0, bb = 0;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const uint4 v = r[q];
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      ab = __builtin_amdgcn_udot4(a[4 * q + e], w[e], ab, false);
      bb = __builtin_amdgcn_udot4(w[e], w[e], bb, false);
    }
  }
  return aa + bb - 2u * ab;
}
__device__ __forceinline__ uint32_t norm_u8(const uint32_t a[32]) {
  uint32_t aa = 0;
#pragma unroll
  for (int g = 0; g < 32; ++g) aa = __builtin_amdgcn_udot4(a[g], a[g], aa, false);
  return aa;
}

// block-wide sum (256 threads)
__device__ __forceinline__ unsigned long long block_sum_u64(unsigned long long v) {
  __shared__ unsigned long long s_red[VB_CHUNK];
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = v;
  __syncthreads();
  for (int s = VB_CHUNK / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  return s_red[0];
}

// ---- seed: closest = min(closest, |p - newest centre|^2), and the chunk's sum (center_chooser.h:238-242, 281-284)
__device__ __forceinline__ void vb_seed(const VbArgs& A, uint32_t slot, uint32_t chunk, int c) {
  const VbJob J = A.jobs[slot];
  const uint32_t i = chunk * VB_CHUNK + threadIdx.x;
  const bool valid = i < J.m;
  uint32_t d = 0;
  if (valid) {
    uint32_t a[32];
    load_row(A.desc + (size_t)A.idx[J.off + i] * 128, a);
    const uint32_t cpos = (uint32_t)A.cidx[(size_t)slot * A.b + c];
    d = dist_u8(a, norm_u8(a), A.desc + (size_t)A.idx[J.off + cpos] * 128);
    if (c > 0) d = min(d, A.closest[J.off + i]);
    A.closest[J.off + i] = d;
  }
  const unsigned long long s = block_sum_u64(valid ? d : 0u);
  if (threadIdx.x == 0) A.csum[J.csum_off + chunk] = s;
}

// ---- select: centre c of the job.  c == 0: rand_int(m); else the first index < m - 1 whose inclusive prefix sum of closest
// reaches randVal = 0 + pot * (r / (RAND_MAX + 1.0)), else m - 1 (center_chooser.h:232, 258-262).  One block.
__device__ __forceinline__ void vb_select(const VbArgs& A, uint32_t slot, int c) {
  __shared__ unsigned long long s_part[VB_CHUNK];
  __shared__ unsigned long long s_base;
  __shared__ double s_rv;
  __shared__ uint32_t s_chunk, s_found;
  const VbJob J = A.jobs[slot];
  const int tid = threadIdx.x;
  const double frac = (double)A.draws[(size_t)slot * A.b + c] / (2147483647.0 + 1.0);
  __syncthreads();
  if (c == 0) {
    if (tid == 0) A.cidx[(size_t)slot * A.b] = (int32_t)((double)(int32_t)J.m * frac);
    __syncthreads();
    return;
  }
  const uint32_t nch = (J.m + VB_CHUNK - 1) / VB_CHUNK;
  const uint32_t per = (nch + VB_CHUNK - 1) / VB_CHUNK;
  {
    unsigned long long s = 0;
    for (uint32_t k = tid * per; k < min(nch, (tid + 1) * per); ++k) s += A.csum[J.csum_off + k];
    s_part[tid] = s;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long pot = 0;
    for (int t = 0; t < VB_CHUNK; ++t) pot += s_part[t];
    const double rv = 0.0 + ((double)pot - 0.0) * frac;
    unsigned long long base = 0;
    uint32_t chunk = 0xffffffffu;
    for (int t = 0; t < VB_CHUNK && chunk == 0xffffffffu; ++t) {
      if ((double)(base + s_part[t]) >= rv) {
        for (uint32_t k = t * per; k < min(nch, (t + 1) * per); ++k) {
          const unsigned long long v = A.csum[J.csum_off + k];
          if ((double)(base + v) >= rv) {
            chunk = k;
            break;
          }
          base += v;
        }
      } else {
        base += s_part[t];
      }
    }
    s_rv = rv;
    s_base = base;
    s_chunk = chunk;
    s_found = 0xffffffffu;
  }
  __syncthreads();
  const uint32_t chunk = s_chunk;
  if (chunk != 0xffffffffu) {
    // inclusive scan of the chunk's closest values on top of the prefix before it
    const uint32_t i = chunk * VB_CHUNK + tid;
    s_part[tid] = i < J.m ? (unsigned long long)A.closest[J.off + i] : 0ull;
    __syncthreads();
    for (int s = 1; s < VB_CHUNK; s <<= 1) {
      const unsigned long long add = tid >= s ? s_part[tid - s] : 0ull;
      __syncthreads();
      s_part[tid] += add;
      __syncthreads();
    }
    if (i < J.m && (double)(s_base + s_part[tid]) >= s_rv) atomicMin(&s_found, i);
    __syncthreads();
  }
  if (tid == 0) {
    uint32_t index = s_found;
    if (index > J.m - 1) index = J.m - 1;
    A.cidx[(size_t)slot * A.b + c] = (int32_t)index;
  }
  __syncthreads();
}

// ---- init: dcenters = double(seed points) (kmeans_index.h:573-579), every accumulator zero.  One block.
__device__ __forceinline__ void vb_init(const VbArgs& A, uint32_t slot) {
  const VbJob J = A.jobs[slot];
  const size_t cb = (size_t)slot * A.b;
  for (uint32_t e = threadIdx.x; e < (uint32_t)A.b * 128u; e += VB_CHUNK) {
    const uint32_t j = e >> 7, k = e & 127u;
    A.dcent[cb * 128 + e] = (double)A.desc[(size_t)A.idx[J.off + (uint32_t)A.cidx[cb + j]] * 128 + k];
    A.sums[cb * 128 + e] = 0ull;
  }
  for (uint32_t j = threadIdx.x; j < (uint32_t)A.b; j += VB_CHUNK) {
    A.counts[cb + j] = 0;
    A.radii[cb + j] = 0u;
  }
  if (threadIdx.x == 0) A.changed[slot] = 0;
}

// ---- assign (kmeans_index.h:586-601, 630-650): L2<uint8_t>::operator()(uint8_t*, double*) per centre in centre order
__device__ __forceinline__ void vb_assign(const VbArgs& A, uint32_t slot, uint32_t chunk, bool initial) {
  __shared__ double s_c[VB_TILE * 128];
  const VbJob J = A.jobs[slot];
  const size_t cb = (size_t)slot * A.b;
  const uint32_t i = chunk * VB_CHUNK + threadIdx.x;
  const bool valid = i < J.m;
  uint32_t a[32];
  load_row(A.desc + (size_t)A.idx[J.off + (valid ? i : 0u)] * 128, a);
  float sq = 0.0f;
  int best = 0;
  for (int tile = 0; tile < A.b; tile += VB_TILE) {
    const int nt = min(VB_TILE, A.b - tile);
    __syncthreads();
    for (int e = threadIdx.x; e < nt * 128; e += VB_CHUNK) s_c[e] = A.dcent[(cb + tile) * 128 + e];
    __syncthreads();
    for (int jj = 0; jj < nt; ++jj) {
      const double* cj = s_c + jj * 128;
      float result = 0.0f;
#pragma unroll
      for (int g = 0; g < 32; ++g) {
        const uint32_t w = a[g];
        const float d0 = (float)((double)(w & 255u) - cj[4 * g]);
        const float d1 = (float)((double)((w >> 8) & 255u) - cj[4 * g + 1]);
        const float d2 = (float)((double)((w >> 16) & 255u) - cj[4 * g + 2]);
        const float d3 = (float)((double)(w >> 24) - cj[4 * g + 3]);
        result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
      }
      if (tile + jj == 0) {
        sq = result;
      } else if (sq > result) {
        best = tile + jj;
        sq = result;
      }
    }
  }
  if (valid) {
    if (!initial && A.belongs[J.off + i] != best) atomicOr(A.changed + slot, 1);
    A.belongs[J.off + i] = best;
    if (sq > 0.0f) atomicMax(A.radii + cb + best, __float_as_uint(sq));  // if (sq_dist > radiuses[..]): a NaN never enters
    atomicAdd(A.counts + cb + best, 1);
  }
}

// ---- accumulate (kmeans_index.h:614-620): the centre sums are sums of integers, so their order does not matter
__device__ __forceinline__ void vb_accumulate(const VbArgs& A, uint32_t slot, uint32_t chunk) {
  const VbJob J = A.jobs[slot];
  const uint32_t i = chunk * VB_CHUNK + threadIdx.x;
  if (i >= J.m) return;
  uint32_t a[32];
  load_row(A.desc + (size_t)A.idx[J.off + i] * 128, a);
  unsigned long long* s = A.sums + ((size_t)slot * A.b + A.belongs[J.off + i]) * 128;
#pragma unroll
  for (int g = 0; g < 32; ++g) {
    const uint32_t w = a[g];
    atomicAdd(s + 4 * g, (unsigned long long)(w & 255u));
    atomicAdd(s + 4 * g + 1, (unsigned long long)((w >> 8) & 255u));
    atomicAdd(s + 4 * g + 2, (unsigned long long)((w >> 16) & 255u));
    atomicAdd(s + 4 * g + 3, (unsigned long long)(w >> 24));
  }
}

// ---- update (kmeans_index.h:610-627): centre = sum * (1.0 / cnt) from the counts the repair left; the accumulators of the
// coming assignment zero.  Elements first .. first + 256 of the job's b * 128.
__device__ __forceinline__ void vb_update(const VbArgs& A, uint32_t slot, uint32_t first) {
  const size_t cb = (size_t)slot * A.b;
  const uint32_t e = first + threadIdx.x;
  if (e < (uint32_t)A.b * 128u) {
    const uint32_t j = e >> 7;
    const int cnt = A.cnt_final[cb + j];
    const double div_factor = 1.0 / cnt;
    A.dcent[cb * 128 + e] = (double)ld_agent(A.sums + cb * 128 + e) * div_factor;
    A.sums[cb * 128 + e] = 0ull;
    if ((e & 127u) == 0) {
      A.counts[cb + j] = 0;
      A.radii[cb + j] = 0u;
    }
  }
  if (e == 0) A.changed[slot] = 0;
}

// ---- repair (kmeans_index.h:652-671) and the hand-over of the counts.  One block.
__device__ __forceinline__ void vb_repair(const VbArgs& A, uint32_t slot, bool repair) {
  __shared__ int s_j;
  __shared__ uint32_t s_k;
  const VbJob J = A.jobs[slot];
  const size_t cb = (size_t)slot * A.b;
  const int tid = threadIdx.x;
  int any = 0;
  for (int j = tid; j < A.b; j += VB_CHUNK) {
    const int cnt = ld_agent(A.counts + cb + j);
    A.cnt_final[cb + j] = cnt;
    any |= cnt == 0;
  }
  any = __syncthreads_or(any);
  __syncthreads();
  if (!any || !repair) return;
  for (int i = 0; i < A.b; ++i) {
    if (tid == 0) {
      int j = -1;
      if (A.cnt_final[cb + i] == 0) {
        j = (i + 1) % A.b;
        while (A.cnt_final[cb + j] <= 1) j = (j + 1) % A.b;
      }
      s_j = j;
      s_k = 0xffffffffu;
    }
    __syncthreads();
    const int j = s_j;
    if (j >= 0) {
      for (uint32_t k = tid; k < J.m; k += VB_CHUNK)
        if (A.belongs[J.off + k] == j) {
          atomicMin(&s_k, k);
          break;
        }
      __syncthreads();
      if (tid == 0 && s_k < J.m) {  // (a donor with count > 1 has a member)
        A.belongs[J.off + s_k] = i;
        A.cnt_final[cb + j] -= 1;
        A.cnt_final[cb + i] += 1;
        st_agent(A.changed + slot, 1);
      }
    }
    __syncthreads();
  }
}

// ---- the float centres (kmeans_index.h:675-683), elements first .. first + 256
__device__ __forceinline__ void vb_centf(const VbArgs& A, uint32_t slot, uint32_t first) {
  const uint32_t e = first + threadIdx.x;
  if (e < (uint32_t)A.b * 128u) A.centf[(size_t)slot * A.b * 128 + e] = (float)A.dcent[(size_t)slot * A.b * 128 + e];
}

// ---- distance of every point to its float centre: L2::operator()(float*, uint8_t*) (kmeans_index.h:518, 696)
__device__ __forceinline__ void vb_distance(const VbArgs& A, uint32_t slot, uint32_t chunk) {
  const VbJob J = A.jobs[slot];
  const uint32_t i = chunk * VB_CHUNK + threadIdx.x;
  if (i >= J.m) return;
  uint32_t a[32];
  load_row(A.desc + (size_t)A.idx[J.off + i] * 128, a);
  const float* cf = A.centf + ((size_t)slot * A.b + A.belongs[J.off + i]) * 128;
  float result = 0.0f;
#pragma unroll
  for (int g = 0; g < 32; ++g) {
    const uint32_t w = a[g];
    const float4 c4 = *reinterpret_cast<const float4*>(cf + 4 * g);
    const float d0 = c4.x - (float)(w & 255u);
    const float d1 = c4.y - (float)((w >> 8) & 255u);
    const float d2 = c4.z - (float)((w >> 16) & 255u);
    const float d3 = c4.w - (float)(w >> 24);
    result += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
  }
  A.dist[J.off + i] = result;
}

// whole-chip form: a launch per phase, job 0
__global__ __launch_bounds__(VB_CHUNK) void k_vb_seed(VbArgs A, int c) { vb_seed(A, 0, blockIdx.x, c); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_select(VbArgs A, int c) { vb_select(A, 0, c); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_init(VbArgs A) { vb_init(A, 0); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_assign(VbArgs A, int initial) { vb_assign(A, 0, blockIdx.x, initial != 0); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_accumulate(VbArgs A) { vb_accumulate(A, 0, blockIdx.x); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_update(VbArgs A) { vb_update(A, 0, blockIdx.x * VB_CHUNK); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_repair(VbArgs A, int repair) { vb_repair(A, 0, repair != 0); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_centf(VbArgs A) { vb_centf(A, 0, blockIdx.x * VB_CHUNK); }
__global__ __launch_bounds__(VB_CHUNK) void k_vb_distance(VbArgs A) { vb_distance(A, 0, blockIdx.x); }

// workgroup form: block = job, every phase in the block
__global__ __launch_bounds__(VB_CHUNK) void k_vb_node(VbArgs A) {
  const uint32_t slot = blockIdx.x;
  const uint32_t m = A.jobs[slot].m;
  const uint32_t nch = (m + VB_CHUNK - 1) / VB_CHUNK;
  const uint32_t nel = (uint32_t)A.b * 128u;
  for (int c = 0; c < A.b; ++c) {
    vb_select(A, slot, c);
    __syncthreads();
    if (c + 1 < A.b)
      for (uint32_t k = 0; k < nch; ++k) vb_seed(A, slot, k, c);
    __syncthreads();
  }
  vb_init(A, slot);
  __syncthreads();
  for (uint32_t k = 0; k < nch; ++k) vb_assign(A, slot, k, true);
  __syncthreads();
  vb_repair(A, slot, false);
  __syncthreads();
  bool converged = false;
  for (int it = 0; !converged && it < A.iterations; ++it) {
    for (uint32_t k = 0; k < nch; ++k) vb_accumulate(A, slot, k);
    __syncthreads();
    for (uint32_t e = 0; e < nel; e += VB_CHUNK) vb_update(A, slot, e);
    __syncthreads();
    for (uint32_t k = 0; k < nch; ++k) vb_assign(A, slot, k, false);
    __syncthreads();
    vb_repair(A, slot, true);
    __syncthreads();
    converged = ld_agent(A.changed + slot) == 0;
    __syncthreads();
  }
  for (uint32_t e = 0; e < nel; e += VB_CHUNK) vb_centf(A, slot, e);
  __syncthreads();
  for (uint32_t k = 0; k < nch; ++k) vb_distance(A, slot, k);
}

// ------------------------------------------------------------------------------------ Hamming embedding
// the exact nearest word, ties to the lower id (what dsm_retrieval_index assigns): argmin of |w|^2 - 2 d.w in exact integers
__global__ __launch_bounds__(VB_CHUNK) void k_vb_nearest_word(const uint8_t* __restrict__ desc, uint64_t n, const uint8_t* __restrict__ words,
                                                              uint32_t num_words, int32_t* __restrict__ wid) {
  __shared__ __attribute__((aligned(16))) uint8_t s_w[64 * 128];
  const uint64_t i = (uint64_t)blockIdx.x * VB_CHUNK + threadIdx.x;
  uint32_t a[32];
  load_row(desc + (i < n ? i : 0) * 128, a);
  const uint32_t aa = norm_u8(a);
  uint32_t best_d = 0xffffffffu;
  int best = 0;
  for (uint32_t tile = 0; tile < num_words; tile += 64) {
    const uint32_t nt = min(64u, num_words - tile);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < nt * 8; e += VB_CHUNK)
      reinterpret_cast<uint4*>(s_w)[e] = reinterpret_cast<const uint4*>(words + (size_t)tile * 128)[e];
    __syncthreads();
    for (uint32_t jj = 0; jj < nt; ++jj) {
      const uint32_t d = dist_u8(a, aa, s_w + jj * 128);
      if (d < best_d) {
        best_d = d;
        best = (int)(tile + jj);
      }
    }
  }
  if (i < n) wid[i] = best;
}

// proj[r][lane] = sum over the 128 dimensions, left to right in float: k_vocab_signature's sum (retrieval.hip), so that the
// trained thresholds and the query's signature bits come from the same numbers
__global__ __launch_bounds__(256) void k_vb_project(const uint8_t* __restrict__ desc, uint64_t n, const float* __restrict__ projT /*[128][64]*/,
                                                    float* __restrict__ proj /*[n][64]*/) {
  __shared__ float sP[128 * 64];
  __shared__ volatile float sD[4][128];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int e = tid; e < 128 * 64; e += 256) sP[e] = projT[e];
  __syncthreads();
  for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < n; r += (uint64_t)gridDim.x * 4) {
    const uint16_t two = *reinterpret_cast<const uint16_t*>(desc + r * 128 + lane * 2);
    sD[wave][2 * lane] = (float)(two & 0xffu);
    sD[wave][2 * lane + 1] = (float)((two >> 8) & 0xffu);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float s = 0.0f;
    for (int j = 0; j < 128; ++j) s = s + sP[j * 64 + lane] * sD[wave][j];
    proj[r * 64 + lane] = s;
    __builtin_amdgcn_wave_barrier();
  }
}

__device__ __forceinline__ uint32_t float_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// the k-th smallest (0-based) of column `lane` of the word's rows: a radix select from the top bit down
__device__ __forceinline__ float select_kth(const float* __restrict__ proj, const uint32_t* __restrict__ rows, uint32_t count, uint32_t k, int lane) {
  uint32_t prefix = 0;
  for (int bit = 31; bit >= 0; --bit) {
    const uint32_t high = bit == 31 ? 0u : (0xffffffffu << (bit + 1));
    uint32_t zeros = 0;
    for (uint32_t e = 0; e < count; ++e) {
      const uint32_t key = float_key(proj[(size_t)rows[e] * 64 + lane]);
      zeros += ((key & high) == prefix) && !((key >> bit) & 1u);
    }
    if (k >= zeros) {
      k -= zeros;
      prefix |= 1u << bit;
    }
  }
  return key_float(prefix);
}
// wave = word, lane = embedding dimension: Median (util/math.h:211-229) of the word's projected descriptors
__global__ __launch_bounds__(256) void k_vb_median(const float* __restrict__ proj, const uint32_t* __restrict__ rows, const uint32_t* __restrict__ seg,
                                                   uint32_t num_words, float* __restrict__ thr, uint8_t* __restrict__ has) {
  const int lane = threadIdx.x & 63;
  const uint32_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= num_words) return;
  const uint32_t s = seg[w], count = seg[w + 1] - s;
  float t = 0.0f;
  if (count >= 5) {  // kMinEntries (inverted_index.h:191)
    const uint32_t mid = count / 2;
    const float m1 = select_kth(proj, rows + s, count, mid, lane);
    if (count % 2 == 0) {
      const float m2 = select_kth(proj, rows + s, count, mid - 1, lane);
      t = (float)((double)(m1 + m2) / 2.0);
    } else {
      t = m1;
    }
  }
  thr[(size_t)w * 64 + lane] = t;
  if (lane == 0) has[w] = count >= 5 ? 1 : 0;
}

// ------------------------------------------------------------------------------------ host side
struct Pending {
  int32_t parent;
  uint32_t off, size;
  float radius, variance;
  std::vector<float> pivot;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

int std_rand(void*) { return rand(); }

}  // namespace

extern "C" void dsm_default_vocabulary_build_options(dsm_vocabulary_build_options* o) {
  if (!o) return;
  o->num_visual_words = 256 * 256;  // BuildOptions, visual_index.h:99-118
  o->branching = 256;
  o->num_iterations = 11;
  o->workgroup_node_max = 0;
}

extern "C" int dsm_retrieval_quantize(dsm_ctx* ctx, const dsm_vocabulary_build_options* options, const uint8_t* descriptors, uint64_t n,
                                      int (*rand_fn)(void*), void* user, uint32_t* num_words_out, uint8_t* words, float* centers) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_retrieval_quantize", msg); };
  dsm_vocabulary_build_options o;
  dsm_default_vocabulary_build_options(&o);
  if (options) o = *options;
  if (!descriptors || !num_words_out || !words) return fail("NULL argument");
  if (o.branching < 2) return fail("branching must be at least 2 (KMeansIndex::buildIndexImpl)");
  if (o.branching > VB_MAX_BRANCHING) return fail("branching above 4096");
  if (o.num_visual_words < o.branching) return fail("num_visual_words must be at least branching (CHECK_GE, visual_index.h:628)");
  if (n < (uint64_t)o.num_visual_words) return fail("fewer descriptors than num_visual_words (CHECK_GE, visual_index.h:629)");
  if (n > 2147483647ull) return fail("more than 2^31 - 1 descriptors");
  if (o.workgroup_node_max < 0) return fail("workgroup_node_max must not be negative");
  const int b = o.branching;
  const int iterations = o.num_iterations < 0 ? std::numeric_limits<int>::max() : o.num_iterations;  // kmeans_index.h:120-122
  const uint32_t wg_max = o.workgroup_node_max ? (uint32_t)o.workgroup_node_max : vb_default_workgroup_node_max(b);
  if (!rand_fn) rand_fn = std_rand;

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;

  // device memory of the call: descriptors, the permutation, three values per position, the per-job state
  const uint32_t nch_all = (uint32_t)((n + VB_CHUNK - 1) / VB_CHUNK);
  const size_t node_bytes = align256(VB_MAX_SLOTS * sizeof(VbJob)) + align256(((size_t)nch_all + VB_MAX_SLOTS) * 8) + align256(VB_MAX_SLOTS * 4) +
                            2 * align256((size_t)VB_MAX_SLOTS * b * 128 * 8) + align256((size_t)VB_MAX_SLOTS * b * 128 * 4) +
                            5 * align256((size_t)VB_MAX_SLOTS * b * 4);
  const uint64_t need = n * 128 + n * 4 + n * 12 + node_bytes;
  if (ctx->memory_budget && need > ctx->memory_budget) {
    ctx->err = "dsm_retrieval_quantize: the descriptors and the tree's state (" + std::to_string(need) + " bytes) exceed the memory budget";
    return DSM_ERR_OUT_OF_RANGE;
  }
  {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b + ctx->d_vb_desc.cap + ctx->d_vb_idx.cap + ctx->d_vb_point.cap + ctx->d_vb_node.cap) {
      ctx->err = "dsm_retrieval_quantize: the descriptors and the tree's state (" + std::to_string(need) + " bytes) do not fit the device's free memory";
      return DSM_ERR_OUT_OF_RANGE;
    }
  }
  struct Release {  // the call's device memory goes back at its end, however it ends
    dsm_ctx* c;
    ~Release() {
      c->d_vb_desc.release();
      c->d_vb_idx.release();
      c->d_vb_point.release();
      c->d_vb_node.release();
    }
  } release{ctx};
  HIPCHK(ctx, ctx->d_vb_desc.reserve(n * 128));
  HIPCHK(ctx, ctx->d_vb_idx.reserve(n * 4));
  HIPCHK(ctx, ctx->d_vb_point.reserve(n * 12));
  HIPCHK(ctx, ctx->d_vb_node.reserve(node_bytes));

  VbArgs A;
  A.desc = ctx->d_vb_desc.as<uint8_t>();
  A.idx = ctx->d_vb_idx.as<int32_t>();
  A.belongs = ctx->d_vb_point.as<int32_t>();
  A.closest = reinterpret_cast<uint32_t*>(A.belongs + n);
  A.dist = reinterpret_cast<float*>(A.closest + n);
  {
    uint8_t* p = ctx->d_vb_node.as<uint8_t>();
    auto carve = [&](size_t bytes) {
      uint8_t* r = p;
      p += align256(bytes);
      return r;
    };
    A.jobs = reinterpret_cast<VbJob*>(carve(VB_MAX_SLOTS * sizeof(VbJob)));
    A.csum = reinterpret_cast<unsigned long long*>(carve(((size_t)nch_all + VB_MAX_SLOTS) * 8));
    A.changed = reinterpret_cast<int32_t*>(carve(VB_MAX_SLOTS * 4));
    A.dcent = reinterpret_cast<double*>(carve((size_t)VB_MAX_SLOTS * b * 128 * 8));
    A.sums = reinterpret_cast<unsigned long long*>(carve((size_t)VB_MAX_SLOTS * b * 128 * 8));
    A.centf = reinterpret_cast<float*>(carve((size_t)VB_MAX_SLOTS * b * 128 * 4));
    A.draws = reinterpret_cast<int32_t*>(carve((size_t)VB_MAX_SLOTS * b * 4));
    A.cidx = reinterpret_cast<int32_t*>(carve((size_t)VB_MAX_SLOTS * b * 4));
    A.counts = reinterpret_cast<int32_t*>(carve((size_t)VB_MAX_SLOTS * b * 4));
    A.cnt_final = reinterpret_cast<int32_t*>(carve((size_t)VB_MAX_SLOTS * b * 4));
    A.radii = reinterpret_cast<uint32_t*>(carve((size_t)VB_MAX_SLOTS * b * 4));
  }
  A.b = b;
  A.iterations = iterations;
  VbJob* d_jobs = const_cast<VbJob*>(A.jobs);
  int32_t* d_draws = const_cast<int32_t*>(A.draws);
  int32_t* d_idx = const_cast<int32_t*>(A.idx);

  DevEvents<8> ev;
  HIPCHK(ctx, ev.create());
  double ms[DSM_VOCABULARY_BUILD_STAGES] = {0};
  auto add_ms = [&](int stage, int e0, int e1) {
    double t = 0;
    if (ev.ms(e0, e1, &t) == hipSuccess) ms[stage] += t;
  };

  // the tree of this call replaces the last one's
  ctx->vb_nodes.clear();
  ctx->vb_pivots.clear();
  ctx->vb_childs.clear();
  ctx->vb_indices.clear();
  ctx->vb_branching = b;
  std::vector<int32_t>& h_idx = ctx->vb_indices;
  h_idx.resize(n);
  for (uint64_t i = 0; i < n; ++i) h_idx[i] = (int32_t)i;
  HIPCHK(ctx, hipMemcpyAsync(const_cast<uint8_t*>(A.desc), descriptors, n * 128, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_idx, h_idx.data(), n * 4, hipMemcpyHostToDevice, st));

  std::vector<int32_t> h_belongs;
  std::vector<float> h_dist;
  std::vector<int32_t> h_counts((size_t)VB_MAX_SLOTS * b), h_draws((size_t)VB_MAX_SLOTS * b);
  std::vector<uint32_t> h_radii((size_t)VB_MAX_SLOTS * b);
  std::vector<float> h_centf((size_t)VB_MAX_SLOTS * b * 128);

  // ---- the root: computeNodeStatistics (kmeans_index.h:496-530).  The mean is one float chain per dimension, on the host; the
  // distances to it on the device, their sum again a chain.
  Pending root;
  root.parent = -1;
  root.off = 0;
  root.size = (uint32_t)n;
  root.pivot.assign(128, 0.0f);
  {
    const double t0 = now_ms();
    float* mean = root.pivot.data();
    for (uint64_t i = 0; i < n; ++i) {
      const uint8_t* vec = descriptors + i * 128;
      for (int j = 0; j < 128; ++j) mean[j] += vec[j];
    }
    const float div_factor = 1.0f / (float)n;
    for (int j = 0; j < 128; ++j) mean[j] *= div_factor;
    ms[3] += now_ms() - t0;
    const VbJob job{0u, (uint32_t)n, 0u, 0u};
    HIPCHK(ctx, hipMemcpyAsync(d_jobs, &job, sizeof(job), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(A.centf, mean, 128 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(A.belongs, 0, n * 4, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_vb_distance, dim3(nch_all), dim3(VB_CHUNK), 0, st, A);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    h_dist.resize(n);
    HIPCHK(ctx, hipMemcpyAsync(h_dist.data(), A.dist, n * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    add_ms(3, 0, 1);
    const double t1 = now_ms();
    float radius = 0.0f, variance = 0.0f;
    for (uint64_t i = 0; i < n; ++i) {
      const float dist = h_dist[i];
      if (dist > radius) radius = dist;
      variance += dist;
    }
    variance /= (float)n;
    root.radius = radius;
    root.variance = variance;
    ms[3] += now_ms() - t1;
  }

  // a node enters the tree when the depth-first walk reaches it
  auto add_node = [&](const Pending& p) {
    const int32_t id = (int32_t)ctx->vb_nodes.size();
    dsm_vocabulary_tree_node nd;
    nd.parent = p.parent;
    nd.first_child = -1;
    nd.size = (int32_t)p.size;
    memcpy(&nd.variance_bits, &p.variance, 4);
    memcpy(&nd.radius_bits, &p.radius, 4);
    ctx->vb_nodes.push_back(nd);
    ctx->vb_pivots.insert(ctx->vb_pivots.end(), p.pivot.begin(), p.pivot.end());
    ctx->vb_childs.emplace_back();
    if (p.parent >= 0) {
      if (ctx->vb_childs[p.parent].empty()) ctx->vb_nodes[p.parent].first_child = id;
      ctx->vb_childs[p.parent].push_back(id);
    }
    return id;
  };
  // the b draws of a clustered node, in the reference's order (center_chooser.h:232, 258)
  auto draw = [&](uint32_t slot) {
    for (int c = 0; c < b; ++c) h_draws[(size_t)slot * b + c] = rand_fn(user);
  };
  // A child that holds all the points of its parent would be clustered into the same children again, without end: the reference
  // recurses until its stack is gone.  Only without iterations (the repair of an iteration leaves no child empty).
  bool stuck = false;
  const char* const stuck_msg = "the clustering does not end: without iterations a node of identical points keeps all of them in one child";
  // kmeans_index.h:686-710 for one finished job: the swap partition of its range with the variance chains, the children
  auto partition = [&](uint32_t slot, const Pending& p, int32_t id, uint32_t span_off, std::vector<Pending>& children) {
    int32_t* idx = h_idx.data() + p.off;
    int32_t* bel = h_belongs.data() + (p.off - span_off);
    float* dist = h_dist.data() + (p.off - span_off);
    const int32_t* count = h_counts.data() + (size_t)slot * b;
    const uint32_t m = p.size;
    uint32_t start = 0, end = 0;
    children.resize(b);
    for (int c = 0; c < b; ++c) {
      const int s = count[c];
      float variance = 0.0f;
      int found = 0;
      for (uint32_t i = start; i < m && found < s; ++i) {
        if (bel[i] == c) {
          variance += dist[i];
          std::swap(idx[i], idx[end]);
          std::swap(bel[i], bel[end]);
          std::swap(dist[i], dist[end]);
          ++end;
          ++found;
        }
      }
      variance /= s;
      Pending& ch = children[c];
      ch.parent = id;
      ch.off = p.off + start;
      ch.size = end - start;
      memcpy(&ch.radius, &h_radii[(size_t)slot * b + c], 4);
      ch.variance = variance;
      ch.pivot.assign(h_centf.begin() + ((size_t)slot * b + c) * 128, h_centf.begin() + ((size_t)slot * b + c + 1) * 128);
      start = end;
      if (ch.size == m) stuck = true;
    }
  };
  // results of a batch of jobs back to the host: the per-position values of the span, the per-job values of every slot
  auto fetch = [&](uint32_t slots, uint32_t span_off, uint32_t span) -> int {
    h_belongs.resize(span);
    h_dist.resize(span);
    HIPCHK(ctx, hipMemcpyAsync(h_belongs.data(), A.belongs + span_off, (size_t)span * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h_dist.data(), A.dist + span_off, (size_t)span * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h_counts.data(), A.cnt_final, (size_t)slots * b * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h_radii.data(), A.radii, (size_t)slots * b * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h_centf.data(), A.centf, (size_t)slots * b * 128 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return DSM_OK;
  };
  // whole-chip form of one job (slot 0)
  auto run_chip = [&](const Pending& p) -> int {
    const uint32_t nch = (p.size + VB_CHUNK - 1) / VB_CHUNK;
    const uint32_t nel_blocks = ((uint32_t)b * 128u + VB_CHUNK - 1) / VB_CHUNK;
    const VbJob job{p.off, p.size, 0u, 0u};
    HIPCHK(ctx, hipMemcpyAsync(d_jobs, &job, sizeof(job), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_draws, h_draws.data(), (size_t)b * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    for (int c = 0; c < b; ++c) {
      hipLaunchKernelGGL(k_vb_select, dim3(1), dim3(VB_CHUNK), 0, st, A, c);
      if (c + 1 < b) hipLaunchKernelGGL(k_vb_seed, dim3(nch), dim3(VB_CHUNK), 0, st, A, c);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_vb_init, dim3(1), dim3(VB_CHUNK), 0, st, A);
    hipLaunchKernelGGL(k_vb_assign, dim3(nch), dim3(VB_CHUNK), 0, st, A, 1);
    hipLaunchKernelGGL(k_vb_repair, dim3(1), dim3(VB_CHUNK), 0, st, A, 0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[2], st));
    bool converged = false;
    bool first_iteration = true;
    for (int it = 0; !converged && it < iterations; ++it) {
      HIPCHK(ctx, hipEventRecord(ev[3], st));
      hipLaunchKernelGGL(k_vb_accumulate, dim3(nch), dim3(VB_CHUNK), 0, st, A);
      hipLaunchKernelGGL(k_vb_update, dim3(nel_blocks), dim3(VB_CHUNK), 0, st, A);
      HIPCHK(ctx, hipEventRecord(ev[4], st));
      hipLaunchKernelGGL(k_vb_assign, dim3(nch), dim3(VB_CHUNK), 0, st, A, 0);
      hipLaunchKernelGGL(k_vb_repair, dim3(1), dim3(VB_CHUNK), 0, st, A, 1);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipEventRecord(ev[5], st));
      int32_t changed = 0;
      HIPCHK(ctx, hipMemcpyAsync(&changed, A.changed, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      if (first_iteration) {
        add_ms(0, 0, 1);
        add_ms(1, 1, 2);
        first_iteration = false;
      }
      add_ms(2, 3, 4);
      add_ms(1, 4, 5);
      converged = changed == 0;
    }
    HIPCHK(ctx, hipEventRecord(ev[6], st));
    hipLaunchKernelGGL(k_vb_centf, dim3(nel_blocks), dim3(VB_CHUNK), 0, st, A);
    hipLaunchKernelGGL(k_vb_distance, dim3(nch), dim3(VB_CHUNK), 0, st, A);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[7], st));
    const int rc = fetch(1, p.off, p.size);
    if (rc != DSM_OK) return rc;
    if (first_iteration) {
      add_ms(0, 0, 1);
      add_ms(1, 1, 2);
    }
    add_ms(3, 6, 7);
    return DSM_OK;
  };

  // ---- computeClustering, depth first: the stack holds the unvisited nodes, the next one of the walk on top
  std::vector<Pending> stack;
  stack.push_back(std::move(root));
  std::vector<Pending> children, batch;
  std::vector<VbJob> h_jobs;
  std::vector<uint32_t> batch_slot;
  while (!stack.empty()) {
    Pending p = std::move(stack.back());
    stack.pop_back();
    if (p.size < (uint32_t)b) {  // a leaf (kmeans_index.h:548-556): no draws
      add_node(p);
      continue;
    }
    if (p.size > wg_max) {
      draw(0);
      const int rc = run_chip(p);
      if (rc != DSM_OK) return rc;
      const double t0 = now_ms();
      const int32_t id = add_node(p);
      partition(0, p, id, p.off, children);
      if (stuck) {
        ctx->vb_nodes.clear();  // no tree to hand out
        return fail(stuck_msg);
      }
      HIPCHK(ctx, hipMemcpyAsync(d_idx + p.off, h_idx.data() + p.off, (size_t)p.size * 4, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      for (int c = b - 1; c >= 0; --c) stack.push_back(std::move(children[c]));
      ms[4] += now_ms() - t0;
      continue;
    }
    // workgroup form.  A node of fewer than 2 * branching - 1 points has no child that reaches branching points: it draws
    // exactly branching values and nothing below it draws, so the nodes that follow it in the walk join its batch as long
    // as the same holds for them (leaves draw nothing and need no job).
    batch.clear();
    batch_slot.clear();
    h_jobs.clear();
    uint32_t csum_off = 0;
    auto add_job = [&](const Pending& q) {
      const uint32_t slot = (uint32_t)h_jobs.size();
      h_jobs.push_back(VbJob{q.off, q.size, csum_off, 0u});
      csum_off += (q.size + VB_CHUNK - 1) / VB_CHUNK;
      draw(slot);
      return slot;
    };
    const bool run = p.size < 2u * (uint32_t)b - 1u && iterations >= 1;  // (without an iteration no repair fills an empty child)
    batch_slot.push_back(add_job(p));
    batch.push_back(std::move(p));
    while (run && !stack.empty() && h_jobs.size() < VB_MAX_SLOTS) {
      const Pending& q = stack.back();
      if (q.size >= (uint32_t)b && (q.size >= 2u * (uint32_t)b - 1u || q.size > wg_max)) break;
      batch_slot.push_back(q.size < (uint32_t)b ? 0xffffffffu : add_job(q));
      batch.push_back(std::move(stack.back()));
      stack.pop_back();
    }
    const uint32_t slots = (uint32_t)h_jobs.size();
    uint32_t span_off = 0xffffffffu, span_end = 0;
    for (const VbJob& j : h_jobs) {
      span_off = std::min(span_off, j.off);
      span_end = std::max(span_end, j.off + j.m);
    }
    HIPCHK(ctx, hipMemcpyAsync(d_jobs, h_jobs.data(), slots * sizeof(VbJob), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_draws, h_draws.data(), (size_t)slots * b * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_vb_node, dim3(slots), dim3(VB_CHUNK), 0, st, A);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    const int rc = fetch(slots, span_off, span_end - span_off);
    if (rc != DSM_OK) return rc;
    add_ms(1, 0, 1);  // a workgroup job's phases are one kernel: its whole time is booked under the assignment
    const double t0 = now_ms();
    for (size_t k = 0; k < batch.size(); ++k) {
      const int32_t id = add_node(batch[k]);
      if (batch_slot[k] == 0xffffffffu) continue;
      partition(batch_slot[k], batch[k], id, span_off, children);
      if (stuck) {
        ctx->vb_nodes.clear();  // no tree to hand out
        return fail(stuck_msg);
      }
      if (run) {
        for (int c = 0; c < b; ++c) add_node(children[c]);  // all leaves: they follow their parent in the walk
      } else {
        for (int c = b - 1; c >= 0; --c) stack.push_back(std::move(children[c]));
      }
    }
    HIPCHK(ctx, hipMemcpyAsync(d_idx + span_off, h_idx.data() + span_off, (size_t)(span_end - span_off) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ms[4] += now_ms() - t0;
  }

  // ---- getMinVarianceClusters (kmeans_index.h:928-969) as written
  const std::vector<dsm_vocabulary_tree_node>& nodes = ctx->vb_nodes;
  auto fvar = [&](int32_t id) {
    float v;
    memcpy(&v, &nodes[id].variance_bits, 4);
    return v;
  };
  const int clusters_length = o.num_visual_words;
  std::vector<int32_t> clusters((size_t)clusters_length);
  int cluster_count = 1;
  clusters[0] = 0;
  float mean_variance = fvar(0) * nodes[0].size;
  while (cluster_count < clusters_length) {
    float min_variance = std::numeric_limits<float>::max();
    int split_index = -1;
    for (int i = 0; i < cluster_count; ++i) {
      const std::vector<int32_t>& ch = ctx->vb_childs[clusters[i]];
      if (!ch.empty()) {
        float variance = mean_variance - fvar(clusters[i]) * nodes[clusters[i]].size;
        for (int j = 0; j < b; ++j) variance += fvar(ch[j]) * nodes[ch[j]].size;
        if (variance < min_variance) {
          min_variance = variance;
          split_index = i;
        }
      }
    }
    if (split_index == -1) break;
    if ((b + cluster_count - 1) > clusters_length) break;
    mean_variance = min_variance;
    const std::vector<int32_t>& ch = ctx->vb_childs[clusters[split_index]];
    clusters[split_index] = ch[0];
    for (int i = 1; i < b; ++i) clusters[cluster_count++] = ch[i];
  }
  for (int i = 0; i < cluster_count; ++i) {
    const float* pivot = ctx->vb_pivots.data() + (size_t)clusters[i] * 128;
    for (int j = 0; j < 128; ++j) {
      if (centers) centers[(size_t)i * 128 + j] = pivot[j];
      const float r = std::round(pivot[j]);  // visual_index.h:651-657; the centre of an emptied cluster is a NaN: 0
      words[(size_t)i * 128 + j] = std::isnan(r) ? (uint8_t)0 : (uint8_t)(int)r;
    }
  }
  *num_words_out = (uint32_t)cluster_count;
  for (int s = 0; s < 5; ++s) ctx->vocabulary_build_ms[s] = ms[s];
  ctx->vocabulary_build_ready = true;
  return DSM_OK;
}

extern "C" int dsm_get_vocabulary_tree(dsm_ctx* ctx, uint32_t* num_nodes, dsm_vocabulary_tree_node* nodes, float* pivots, uint32_t node_capacity,
                                       int32_t* indices, uint64_t indices_capacity) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (ctx->vb_nodes.empty()) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_vocabulary_tree: no dsm_retrieval_quantize call has finished");
  if (num_nodes) *num_nodes = (uint32_t)ctx->vb_nodes.size();
  if (nodes || pivots) {
    if (node_capacity < ctx->vb_nodes.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_vocabulary_tree: node capacity too small");
    if (nodes) memcpy(nodes, ctx->vb_nodes.data(), ctx->vb_nodes.size() * sizeof(dsm_vocabulary_tree_node));
    if (pivots) memcpy(pivots, ctx->vb_pivots.data(), ctx->vb_pivots.size() * 4);
  }
  if (indices) {
    if (indices_capacity < ctx->vb_indices.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_vocabulary_tree: indices capacity too small");
    memcpy(indices, ctx->vb_indices.data(), ctx->vb_indices.size() * 4);
  }
  return DSM_OK;
}

extern "C" int dsm_retrieval_train_embedding(dsm_ctx* ctx, const uint8_t* descriptors, uint64_t n, const uint8_t* words, uint32_t num_words,
                                             const float* projection, const int32_t* word_ids, float* thresholds, uint8_t* has_embedding) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_retrieval_train_embedding", msg); };
  if ((n && !descriptors) || !words || !projection || !thresholds || !has_embedding) return fail("NULL argument");
  if (num_words == 0 || num_words > 0x7ffffffeu) return fail("num_words out of range");
  if (n > 0x7fffffffull) return fail("more than 2^31 - 1 descriptors");
  if (word_ids)
    for (uint64_t i = 0; i < n; ++i)
      if (word_ids[i] < 0 || (uint32_t)word_ids[i] >= num_words) return fail("a word id out of range (indices_per_word.at)");
  memset(thresholds, 0, (size_t)num_words * 64 * 4);
  memset(has_embedding, 0, num_words);
  ctx->vocabulary_build_ms[5] = 0.0;
  if (n == 0) {
    ctx->vocabulary_build_ready = true;
    return DSM_OK;
  }
  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  const size_t desc_b = align256(n * 128), words_b = align256((size_t)num_words * 128), proj_b = align256(n * 64 * 4), pt_b = align256(128 * 64 * 4);
  const size_t wid_b = align256(n * 4), seg_b = align256(((size_t)num_words + 1) * 4), thr_b = align256((size_t)num_words * 64 * 4), has_b = align256(num_words);
  const uint64_t need = desc_b + words_b + proj_b + pt_b + 2 * wid_b + seg_b + thr_b + has_b;
  if (ctx->memory_budget && need > ctx->memory_budget) {
    ctx->err = "dsm_retrieval_train_embedding: the descriptors and their projections (" + std::to_string(need) + " bytes) exceed the memory budget";
    return DSM_ERR_OUT_OF_RANGE;
  }
  struct Release {
    dsm_ctx* c;
    ~Release() { c->d_vb_embed.release(); }
  } release{ctx};
  HIPCHK(ctx, ctx->d_vb_embed.reserve(need));
  uint8_t* p = ctx->d_vb_embed.as<uint8_t>();
  uint8_t* d_desc = p;
  uint8_t* d_words = d_desc + desc_b;
  float* d_proj = reinterpret_cast<float*>(d_words + words_b);
  float* d_projT = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(d_proj) + proj_b);
  int32_t* d_wid = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(d_projT) + pt_b);
  uint32_t* d_rows = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(d_wid) + wid_b);
  uint32_t* d_seg = reinterpret_cast<uint32_t*>(reinterpret_cast<uint8_t*>(d_rows) + wid_b);
  float* d_thr = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(d_seg) + seg_b);
  uint8_t* d_has = reinterpret_cast<uint8_t*>(d_thr) + thr_b;

  DevEvents<2> ev;
  HIPCHK(ctx, ev.create());
  std::vector<float> projT(128 * 64);
  for (int i = 0; i < 64; ++i)
    for (int j = 0; j < 128; ++j) projT[j * 64 + i] = projection[i * 128 + j];
  HIPCHK(ctx, hipMemcpyAsync(d_desc, descriptors, n * 128, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_words, words, (size_t)num_words * 128, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_projT, projT.data(), 128 * 64 * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  const uint32_t blocks = (uint32_t)((n + VB_CHUNK - 1) / VB_CHUNK);
  std::vector<int32_t> ids(n);
  if (word_ids) {
    memcpy(ids.data(), word_ids, n * 4);
  } else {
    hipLaunchKernelGGL(k_vb_nearest_word, dim3(blocks), dim3(VB_CHUNK), 0, st, d_desc, n, d_words, num_words, d_wid);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ids.data(), d_wid, n * 4, hipMemcpyDeviceToHost, st));
  }
  hipLaunchKernelGGL(k_vb_project, dim3((uint32_t)std::min<uint64_t>((n + 3) / 4, 4096)), dim3(256), 0, st, d_desc, n, d_projT, d_proj);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipStreamSynchronize(st));
  // indices_per_word (inverted_index.h:194-197): the rows of every word, a counting sort on the host
  std::vector<uint32_t> seg((size_t)num_words + 1, 0u), rows(n);
  for (uint64_t i = 0; i < n; ++i) ++seg[(size_t)ids[i] + 1];
  for (uint32_t w = 0; w < num_words; ++w) seg[w + 1] += seg[w];
  {
    std::vector<uint32_t> fill(seg.begin(), seg.end() - 1);
    for (uint64_t i = 0; i < n; ++i) rows[fill[ids[i]]++] = (uint32_t)i;
  }
  HIPCHK(ctx, hipMemcpyAsync(d_rows, rows.data(), n * 4, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(d_seg, seg.data(), ((size_t)num_words + 1) * 4, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_vb_median, dim3((num_words + 3) / 4), dim3(256), 0, st, d_proj, d_rows, d_seg, num_words, d_thr, d_has);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  HIPCHK(ctx, hipMemcpyAsync(thresholds, d_thr, (size_t)num_words * 64 * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(has_embedding, d_has, num_words, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, ev.ms(0, 1, &ctx->vocabulary_build_ms[5]));
  ctx->vocabulary_build_ready = true;
  return DSM_OK;
}

extern "C" int dsm_get_vocabulary_build_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->vocabulary_build_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_vocabulary_build_time: no vocabulary call has finished");
  for (int s = 0; s < DSM_VOCABULARY_BUILD_STAGES; ++s) stage_ms[s] = ctx->vocabulary_build_ms[s];
  return DSM_OK;
}
