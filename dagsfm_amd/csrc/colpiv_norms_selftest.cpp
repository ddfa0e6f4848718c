// colpiv_norms_selftest.cpp -- a stand-alone program over colpiv_norms_host.cpp (`make norms-selftest` builds and runs it under
// -fsanitize=address,undefined): random, rank-deficient, tied, badly scaled and non-finite 9 x M matrices through both traces.
// Exit status 0 when every certified trace equals the exact one; the sanitizers abort on anything else worth knowing.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" int dsm_cpn_trace_exact(const double* mats, int n, int m, int* pivots, int* recomputes, int* certain);
extern "C" int dsm_cpn_trace_certified(const double* mats, int n, int m, int* pivots, int* recomputes, int* certain);

static uint64_t state = 0x9e3779b97f4a7c15ull;
static double uniform() {  // xorshift64*, in (-1, 1)
  state ^= state >> 12;
  state ^= state << 25;
  state ^= state >> 27;
  return (double)((state * 0x2545f4914f6cdd1dull) >> 11) / 4503599627370496.0 - 1.0;
}

int main() {
  const int sizes[3] = {5, 7, 8};
  long certain_n = 0, total = 0, wrong = 0, recomputed = 0;
  for (int m : sizes) {
    const int n = 6000;
    std::vector<double> mats((size_t)n * 9 * m);
    for (int q = 0; q < n; ++q) {
      double* a = &mats[(size_t)q * 9 * m];
      for (int i = 0; i < 9 * m; ++i) a[i] = uniform();
      const int kind = q % 8;
      if (kind == 1) memcpy(a + 9 * (m - 1), a, 9 * sizeof(double));                                   // a tie
      if (kind == 2) for (int i = 0; i < 9; ++i) a[9 * (m - 1) + i] = a[i] + a[9 + i] + 1e-9 * uniform();  // nearly dependent
      if (kind == 3) for (int i = 0; i < 9; ++i) a[9 + i] *= ldexp(1.0, -20 - q % 30);                  // badly scaled
      if (kind == 4) for (int i = 0; i < 9 * m; ++i) a[i] *= ldexp(1.0, (q & 8) ? 251 : -251);         // at the guards
      if (kind == 5) a[q % (9 * m)] = (q & 8) ? NAN : INFINITY;
      if (kind == 6) memset(a + 9 * (q % m), 0, 9 * sizeof(double));                                   // a zero column
    }
    std::vector<int> pe((size_t)n * 8), re((size_t)n * 64), ce(n), pc((size_t)n * 8), rc((size_t)n * 64), cc(n);
    if (dsm_cpn_trace_exact(mats.data(), n, m, pe.data(), re.data(), ce.data()) != 0) return 2;
    if (dsm_cpn_trace_certified(mats.data(), n, m, pc.data(), rc.data(), cc.data()) != 0) return 2;
    for (int q = 0; q < n; ++q) {
      ++total;
      if (!cc[q]) continue;
      ++certain_n;
      if (memcmp(&pe[(size_t)q * 8], &pc[(size_t)q * 8], 8 * sizeof(int)) || memcmp(&re[(size_t)q * 64], &rc[(size_t)q * 64], 64 * sizeof(int))) ++wrong;
      for (int k = 0; k < 64; ++k) recomputed += re[(size_t)q * 64 + k];
    }
  }
  if (dsm_cpn_trace_exact(nullptr, 0, 6, nullptr, nullptr, nullptr) != -1) return 2;  // a refused size
  printf("colpiv_norms selftest: %ld matrices, %ld certain, %ld recomputes among them, %ld wrong\n", total, certain_n, recomputed, wrong);
  return wrong == 0 && certain_n > 0 && certain_n < total ? 0 : 1;
}
