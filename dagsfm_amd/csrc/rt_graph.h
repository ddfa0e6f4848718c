// rt_graph.h -- the correspondence lists of CorrespondenceGraph::AddCorrespondences (src/base/correspondence_graph.cc:77-161) as
// CSR over the features, shared by retriangulation.hip and track_update.hip: after the duplicate
// rule (rt_dedup.h) the accepted matches are counted per feature, the counts scanned in fixed blocks, every match emitted as
// two directed entries, and each feature's segment sorted by pair index -- the reference's (pair, match) append order.
#ifndef DAGSFM_AMD_CSRC_RT_GRAPH_H_
#define DAGSFM_AMD_CSRC_RT_GRAPH_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rt_dedup.h"

namespace {

constexpr int RT_GRAPH_BLOCK = 256;  // the workgroup of the scan kernels: a scan block is four items per lane

// the accepted matches of a pair counted per feature (integer atomics: the counts do not depend on their order)
__global__ void k_rt_count(uint32_t n_pairs, const uint32_t* __restrict__ pair_img, const uint64_t* __restrict__ moff,
                           const uint32_t* __restrict__ matches, const uint8_t* __restrict__ acc, const uint32_t* __restrict__ img_foff,
                           uint32_t* __restrict__ cnt) {
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  const uint32_t fa = img_foff[pair_img[2 * k]], fb = img_foff[pair_img[2 * k + 1]];
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x)
    if (acc[m]) {
      atomicAdd(&cnt[fa + matches[2 * m]], 1u);
      atomicAdd(&cnt[fb + matches[2 * m + 1]], 1u);
    }
}

// exclusive scan of n counts in blocks of RT_GRAPH_BLOCK * 4; block totals to sums (scanned by the next level)
__global__ void k_rt_scan_block(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t* __restrict__ sums) {
  __shared__ uint32_t sh[RT_GRAPH_BLOCK];
  const uint32_t base = blockIdx.x * RT_GRAPH_BLOCK * 4 + threadIdx.x * 4;
  uint32_t v[4], t = 0;
  for (int i = 0; i < 4; ++i) {
    v[i] = base + i < n ? in[base + i] : 0u;
    t += v[i];
  }
  sh[threadIdx.x] = t;
  __syncthreads();
  for (int d = 1; d < RT_GRAPH_BLOCK; d *= 2) {
    const uint32_t x = threadIdx.x >= (uint32_t)d ? sh[threadIdx.x - d] : 0u;
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  uint32_t run = sh[threadIdx.x] - t;
  for (int i = 0; i < 4; ++i) {
    if (base + i < n) out[base + i] = run;
    run += v[i];
  }
  if (threadIdx.x == RT_GRAPH_BLOCK - 1) sums[blockIdx.x] = sh[threadIdx.x];
}

__global__ void k_rt_scan_add(uint32_t n, uint32_t* __restrict__ out, const uint32_t* __restrict__ sums) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] += sums[i / (RT_GRAPH_BLOCK * 4)];
}

// every accepted match as two directed entries, each at a slot of its source feature's segment (arrival order)
__global__ void k_rt_emit(uint32_t n_pairs, const uint32_t* __restrict__ pair_img, const uint64_t* __restrict__ moff,
                          const uint32_t* __restrict__ matches, const uint8_t* __restrict__ acc, const uint32_t* __restrict__ img_foff,
                          const uint32_t* __restrict__ goff, uint32_t* __restrict__ fill, uint32_t* __restrict__ epair,
                          uint32_t* __restrict__ eval) {
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  const uint32_t fa = img_foff[pair_img[2 * k]], fb = img_foff[pair_img[2 * k + 1]];
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x)
    if (acc[m]) {
      const uint32_t a = fa + matches[2 * m], b = fb + matches[2 * m + 1];
      const uint32_t sa = goff[a] + atomicAdd(&fill[a], 1u), sb = goff[b] + atomicAdd(&fill[b], 1u);
      epair[sa] = k;
      eval[sa] = b;
      epair[sb] = k;
      eval[sb] = a;
    }
}

// each feature's segment sorted by pair index (distinct inside a segment): the reference's (pair, match) append order
__global__ void k_rt_segsort(uint32_t F, const uint32_t* __restrict__ goff, uint32_t* __restrict__ epair, uint32_t* __restrict__ eval) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const uint32_t lo = goff[f], hi = goff[f + 1];
  for (uint32_t i = lo + 1; i < hi; ++i) {
    const uint32_t kp = epair[i], kv = eval[i];
    uint32_t j = i;
    while (j > lo && epair[j - 1] > kp) {
      epair[j] = epair[j - 1];
      eval[j] = eval[j - 1];
      --j;
    }
    epair[j] = kp;
    eval[j] = kv;
  }
}

}  // namespace

#endif  // DAGSFM_AMD_CSRC_RT_GRAPH_H_
