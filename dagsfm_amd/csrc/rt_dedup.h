// rt_dedup.h -- the duplicate rule of CorrespondenceGraph::AddCorrespondences (src/base/correspondence_graph.cc:77-161) as a
// kernel, shared by retriangulation.hip and initial_pair.hip: one workgroup per pair walks the
// pair's matches in match order over an LDS bitmap of the pair's two images (at most 262144 points2D each) and flags the matches
// the rule keeps -- a match is dropped when either of its features already has a correspondence in the pair's other image.
#ifndef DAGSFM_AMD_CSRC_RT_DEDUP_H_
#define DAGSFM_AMD_CSRC_RT_DEDUP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

__global__ void k_rt_dedup(uint32_t n_pairs, const uint32_t* __restrict__ pair_img, const uint64_t* __restrict__ moff,
                           const uint32_t* __restrict__ matches, const uint32_t* __restrict__ img_nfeat, uint8_t* __restrict__ acc) {
  __shared__ uint32_t bits[16384];
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  const uint32_t n1 = img_nfeat[pair_img[2 * k]], n2 = img_nfeat[pair_img[2 * k + 1]];
  const uint32_t words = (n1 + n2 + 31) / 32;
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) bits[w] = 0u;
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint64_t m = moff[k]; m < moff[k + 1]; ++m) {
    const uint32_t a = matches[2 * m], b = n1 + matches[2 * m + 1];
    const bool d1 = (bits[a >> 5] >> (a & 31)) & 1u, d2 = (bits[b >> 5] >> (b & 31)) & 1u;
    if (d1 || d2) {
      acc[m] = 0;
    } else {
      bits[a >> 5] |= 1u << (a & 31);
      bits[b >> 5] |= 1u << (b & 31);
      acc[m] = 1;
    }
  }
}

}  // namespace

#endif  // DAGSFM_AMD_CSRC_RT_DEDUP_H_
