// exact_exp_host.cpp -- the host build of exact_exp.h as a tiny shared object (../libdsm_exact_exp.so), so that
// tests/test_patch_match_cpu.py can hold dsm_exp to the host libm without a device: y[i] = (float)dsm_exp((double)x[i]).
#include <stdint.h>

#define DSM_XE static inline
#include "exact_exp.h"

extern "C" void dsm_host_exp_f32(const float* x, float* y, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) y[i] = (float)dsm_exp((double)x[i]);
}

extern "C" void dsm_host_exp_f64(const double* x, double* y, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) y[i] = dsm_exp(x[i]);
}
