// colpiv_norms_host.cpp -- the host build of colpiv_norms.h as a tiny shared object (../libdsm_colpiv_norms.so), so that
// tests/test_colpiv_norms_cpu.py can hold the certified tracker's decisions to the exact bookkeeping's without a device.
// Matrices are 9 x m column-major (m in {5, 7, 8}), n of them back to back; every one is copied, so the input is not changed.
// pivots: n x 8 ints, recomputes: n x 64 ints (step * 8 + column), certain: n ints.  Returns 0, or -1 for a refused size.
#include "colpiv_norms.h"

#include <string.h>

static int run(int certified, const double* mats, int n, int m, int* pivots, int* recomputes, int* certain) {
  if (!(m == 5 || m == 7 || m == 8) || n < 0) return -1;
  for (int q = 0; q < n; ++q) {
    double qr[72];
    memcpy(qr, mats + (size_t)q * 9 * m, sizeof(double) * 9 * m);
    int* pv = pivots + (size_t)q * 8;
    int* rc = recomputes + (size_t)q * 64;
    for (int k = 0; k < 8; ++k) pv[k] = -1;
    for (int k = 0; k < 64; ++k) rc[k] = 0;
    certain[q] = certified ? cpn_trace_certified(qr, m, pv, rc) : cpn_trace_exact(qr, m, pv, rc);
  }
  return 0;
}

extern "C" int dsm_cpn_trace_exact(const double* mats, int n, int m, int* pivots, int* recomputes, int* certain) {
  return run(0, mats, n, m, pivots, recomputes, certain);
}
extern "C" int dsm_cpn_trace_certified(const double* mats, int n, int m, int* pivots, int* recomputes, int* certain) {
  return run(1, mats, n, m, pivots, recomputes, certain);
}
extern "C" double dsm_cpn_margin() { return kCpnMargin; }
