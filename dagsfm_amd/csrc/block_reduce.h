// block_reduce.h -- fixed-order block reductions of the SfM stages (rotation averaging, cluster alignment, bundle adjustment).
// Every reduction is per-thread strided partials, then one halving LDS tree over the BS threads of the block: the same tree
// for every launch, so a result is the same bytes from run to run.  Every thread of the block calls these (they
// synchronise); sh holds K * BS doubles, column k at sh[k * BS .. k * BS + BS).
#ifndef DAGSFM_AMD_CSRC_BLOCK_REDUCE_H_
#define DAGSFM_AMD_CSRC_BLOCK_REDUCE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

// the K columns sh[k * BS + t] summed into sh[k * BS]
template <int BS>
__device__ inline void block_tree(double* sh, int K) {
  for (int s = BS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
      for (int k = 0; k < K; ++k) sh[k * BS + threadIdx.x] += sh[k * BS + threadIdx.x + s];
    __syncthreads();
  }
}
// the sums of v[0..K) over the block, back in v in every thread.  block_tree's tree written out: with K a constant from the
// start the column loop unrolls before the tree is scheduled (a call of block_tree compiles to other, if equivalent, code)
template <int BS, int K>
__device__ inline void block_sum(double* v, double* sh) {
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) sh[k * BS + t] = v[k];
  __syncthreads();
  for (int s = BS / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < K; ++k) sh[k * BS + t] += sh[k * BS + t + s];
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) v[k] = sh[k * BS];
  __syncthreads();
}
template <int BS>
__device__ inline double block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  block_tree<BS>(sh, 1);
  const double out = sh[0];
  __syncthreads();
  return out;
}
template <int BS>
__device__ inline double block_max(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = BS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
    __syncthreads();
  }
  const double out = sh[0];
  __syncthreads();
  return out;
}
// std::min(a, b) / std::max(a, b) as the C++ library defines them: b only where the comparison holds, so a NaN in b is never
// taken (fmin / fmax above would not take one in a either)
__device__ inline double std_min(double a, double b) { return (b < a) ? b : a; }
__device__ inline double std_max(double a, double b) { return (a < b) ? b : a; }
// the minima / maxima of v[0..K) over the block under std_min / std_max, back in v in every thread.  No order of the tree
// changes the result as long as no v is a NaN (up to the sign of a zero that ties with the other zero).
template <int BS, int K>
__device__ inline void block_std_min(double* v, double* sh) {
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) sh[k * BS + t] = v[k];
  __syncthreads();
  for (int s = BS / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < K; ++k) sh[k * BS + t] = std_min(sh[k * BS + t], sh[k * BS + t + s]);
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) v[k] = sh[k * BS];
  __syncthreads();
}
template <int BS, int K>
__device__ inline void block_std_max(double* v, double* sh) {
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) sh[k * BS + t] = v[k];
  __syncthreads();
  for (int s = BS / 2; s > 0; s >>= 1) {
    if (t < s)
      for (int k = 0; k < K; ++k) sh[k * BS + t] = std_max(sh[k * BS + t], sh[k * BS + t + s]);
    __syncthreads();
  }
  for (int k = 0; k < K; ++k) v[k] = sh[k * BS];
  __syncthreads();
}
// the K columns of n partials P[k * n + i] reduced by one block: thread t takes i = t, t + BS, ... in order, then the tree.
// Every block that calls it gets the same bytes.
template <int BS, int K, typename I>
__device__ inline void sum_partials(const double* __restrict__ P, I n, double* out, double* sh) {
  for (int k = 0; k < K; ++k) {
    double s = 0.0;
    for (I i = threadIdx.x; i < n; i += BS) s += P[(size_t)k * n + i];
    out[k] = s;
  }
  block_sum<BS, K>(out, sh);
}
template <int BS>
__device__ inline double sum_partials(const double* P, uint32_t n, double* sh) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += BS) s += P[i];
  return block_sum<BS>(s, sh);
}
// the maximum of P[0..n) and 0
template <int BS>
__device__ inline double max_partials(const double* P, uint32_t n, double* sh) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += BS) s = fmax(s, P[i]);
  return block_max<BS>(s, sh);
}
// the block sums of v[0..K) as this block's partials of a launch: P[k * gridDim.x + blockIdx.x]
template <int BS, int K>
__device__ inline void write_partials(double* v, double* sh, double* __restrict__ P) {
  block_sum<BS, K>(v, sh);
  if (threadIdx.x == 0)
    for (int k = 0; k < K; ++k) P[(size_t)k * gridDim.x + blockIdx.x] = v[k];
}

#endif  // DAGSFM_AMD_CSRC_BLOCK_REDUCE_H_
