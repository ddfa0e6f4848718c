// std_mt19937_selftest.cpp -- a stand-alone program over std_mt19937.h (`make mt-selftest` builds and runs it under
// -fsanitize=address,undefined): the generator against std::mt19937, the draw against libstdc++'s
// std::uniform_int_distribution<uint32_t> on the same engine.  Exit status 0 when every output is equal.
#include <stdint.h>
#include <stdio.h>

#include <random>

#include "std_mt19937.h"

int main() {
  long wrong = 0, total = 0;
  // the first 2 000 outputs: three regenerations of the 624 words
  const uint32_t seeds[4] = {0u, 1u, 5489u, 0xffffffffu};
  for (uint32_t seed : seeds) {
    std::mt19937 ref(seed);
    StdMt19937 gen;
    std_mt19937_seed(&gen, seed);
    for (int i = 0; i < 2000; ++i, ++total) wrong += std_mt19937_next(&gen) != (uint32_t)ref();
  }
  // uniform_u32(a, b) for the range sizes 1, 2, 3, 7, 1 000, 2^31, 2^32 - 1 at two offsets each, and the full range
  const uint64_t sizes[7] = {1, 2, 3, 7, 1000, 1ull << 31, 0xffffffffull};
  for (uint64_t size : sizes)
    for (uint32_t a : {0u, 12345u}) {
      if ((uint64_t)a + size - 1 > 0xffffffffull) continue;
      const uint32_t b = (uint32_t)(a + size - 1);
      std::mt19937 ref(size == 1 ? 7u : (uint32_t)size);
      StdMt19937 gen;
      std_mt19937_seed(&gen, size == 1 ? 7u : (uint32_t)size);
      std::uniform_int_distribution<uint32_t> dist(a, b);
      for (int i = 0; i < 10000; ++i, ++total) wrong += std_uniform_u32(&gen, a, b) != dist(ref);
      wrong += std_mt19937_next(&gen) != (uint32_t)ref();  // both consumed the same number of draws
      ++total;
    }
  {
    std::mt19937 ref(99u);
    StdMt19937 gen;
    std_mt19937_seed(&gen, 99u);
    std::uniform_int_distribution<uint32_t> dist(0u, 0xffffffffu);
    for (int i = 0; i < 10000; ++i, ++total) wrong += std_uniform_u32(&gen, 0u, 0xffffffffu) != dist(ref);
  }
  printf("std_mt19937 selftest: %ld comparisons, %ld wrong\n", total, wrong);
  return wrong ? 1 : 0;
}
