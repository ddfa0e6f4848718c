// wave_reduce.h -- the xor butterfly over the 64 lanes of a wave: offsets 32, 16, ..., 1, every lane returns the result.
// The order is part of the results: a double sum by this butterfly is not the sum of block_reduce.h's LDS trees, and the
// stages that hold bit parity with a host restatement hold it to this order.  All 64 lanes must call.
// Inlined where they are called, before anything else is optimised: the kernels they replaced open-coded loops in keep their code.
#ifndef DAGSFM_AMD_CSRC_WAVE_REDUCE_H_
#define DAGSFM_AMD_CSRC_WAVE_REDUCE_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#define WAVE_DEV __device__ __forceinline__

WAVE_DEV uint32_t wave_sum(uint32_t v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
WAVE_DEV int wave_sum(int v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
WAVE_DEV uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o);
  return v;
}
WAVE_DEV double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// N sums side by side: one step of all N butterflies before the next
template <int N>
WAVE_DEV void wave_sum(double (&v)[N]) {
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int c = 0; c < N; ++c) v[c] += __shfl_xor(v[c], o);
  }
}
// fmin: a NaN lane is ignored
WAVE_DEV double wave_fmin(double v) {
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}
WAVE_DEV int wave_min(int v) {
  for (int o = 32; o > 0; o >>= 1) {
    const int other = __shfl_xor(v, o);
    v = other < v ? other : v;
  }
  return v;
}
// v = op(v, the partner lane's v): for a reduction none of the named forms covers (local_bundle.hip lb_reduce)
template <typename T, typename Op>
WAVE_DEV T wave_reduce(T v, Op op) {
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}

#endif  // DAGSFM_AMD_CSRC_WAVE_REDUCE_H_
