// trust_region_host.cpp -- the host build of trust_region.h as a tiny shared object (../libdsm_trust_region.so), so that
// tests/test_trust_region_cpu.py can hold the rulings to DESIGN.md 12's formulas without a device.  State and options travel
// by pointer; the two sizes let the test check its ctypes mirror of the structs.
#include "trust_region.h"

extern "C" int dsm_tr_sizeof_state() { return (int)sizeof(TrState); }
extern "C" int dsm_tr_sizeof_options() { return (int)sizeof(TrOptions); }
extern "C" void dsm_tr_ceres_defaults(TrOptions* o) { *o = tr_ceres_defaults(); }
extern "C" void dsm_tr_init(TrState* s, double initial_radius) { tr_init(s, initial_radius); }
extern "C" double dsm_tr_margin(double a, double thr) { return tr_margin(a, thr); }
extern "C" int dsm_tr_decide(TrState* s, const TrOptions* o, int solved, double cand_cost, double model_cost_change, double step2,
                             double x2) {
  return tr_decide(s, *o, solved != 0, cand_cost, model_cost_change, step2, x2);
}
extern "C" void dsm_tr_end_iteration(TrState* s, const TrOptions* o, int fresh) { tr_end_iteration(s, *o, fresh != 0); }
