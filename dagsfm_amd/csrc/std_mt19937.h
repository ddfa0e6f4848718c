// std_mt19937.h -- std::mt19937 and libstdc++'s std::uniform_int_distribution<uint32_t> on it, for one lane.
//
// verify_kernels.hip keeps a generator of its own (MtState, mt_next, uniform_u32 there): that one counts its calls and has a
// wave-wide twist, and the verification's hot path is frozen.  It is not a third copy to merge into this header.
//
// Bit parity of absolute pose estimation and cluster alignment with their host references rests on this generator;
// std_mt19937_selftest.cpp (make mt-selftest) holds it to the standard library's.  Compiles for the host and the device;
// `static` without `inline`, so that the compiler weighs inlining the twist as it did for the kernels' own copies.
#ifndef DAGSFM_AMD_CSRC_STD_MT19937_H_
#define DAGSFM_AMD_CSRC_STD_MT19937_H_

#include <stdint.h>

#ifdef __HIPCC__
#define MT_HD static __host__ __device__
#else
#define MT_HD static
#endif

struct StdMt19937 {
  uint32_t mt[624];
  int mti;
};
MT_HD void std_mt19937_seed(StdMt19937* s, uint32_t seed) {
  s->mt[0] = seed;
  for (int i = 1; i < 624; ++i) s->mt[i] = 1812433253u * (s->mt[i - 1] ^ (s->mt[i - 1] >> 30)) + (uint32_t)i;
  s->mti = 624;
}
MT_HD uint32_t std_mt19937_next(StdMt19937* s) {
  if (s->mti >= 624) {
    uint32_t* mt = s->mt;
    for (int kk = 0; kk < 624; ++kk) {
      const uint32_t y = (mt[kk] & 0x80000000u) | (mt[(kk + 1) % 624] & 0x7fffffffu);
      mt[kk] = mt[(kk + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    s->mti = 0;
  }
  uint32_t y = s->mt[s->mti++];
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  return y;
}
// std::uniform_int_distribution<uint32_t>(a, b) on the draws of next(): Lemire's method on 32-bit draws, the engine's output as
// it is for the full range.  `next` is a parameter so that a kernel can keep its draw out of line (absolute_pose.hip).
template <typename Next>
MT_HD uint32_t std_uniform_u32(Next next, uint32_t a, uint32_t b) {
  const uint64_t urange = (uint64_t)b - (uint64_t)a;
  const uint32_t first = next();
  if (urange == 0xffffffffull) return first + a;
  const uint32_t range = (uint32_t)(urange + 1);
  uint64_t product = (uint64_t)first * (uint64_t)range;
  uint32_t low = (uint32_t)product;
  if (low < range) {
    const uint32_t threshold = (0u - range) % range;
    while (low < threshold) {
      product = (uint64_t)next() * (uint64_t)range;
      low = (uint32_t)product;
    }
  }
  return (uint32_t)(product >> 32) + a;
}
MT_HD uint32_t std_uniform_u32(StdMt19937* s, uint32_t a, uint32_t b) {
  return std_uniform_u32([s] { return std_mt19937_next(s); }, a, b);
}

#endif  // DAGSFM_AMD_CSRC_STD_MT19937_H_
