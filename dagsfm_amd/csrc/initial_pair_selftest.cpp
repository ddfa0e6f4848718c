// initial_pair_selftest.cpp -- `make initial-pair-selftest`: the host build of initial_pair.h as a stand-alone program under the
// address and undefined-behaviour sanitizers.  Random small scenes through both forms of the candidate order (the reference's
// nested loops and the device's packed keys), which must agree, a hand-written four-image answer, the argument errors, and the
// small exact pieces at their edges.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dagsfm_mi355x.h"

extern "C" {
double dsm_ip_host_acos(double q);
void dsm_ip_host_default_options(dsm_initial_pair_options* o);
double dsm_ip_host_tri_angle(const double* c1, const double* c2, const double* X);
double dsm_ip_host_median(const double* a, uint64_t n);
void dsm_ip_host_pose(const double* qvec, const double* tvec, double* P, double* center, double* minus_Rt_t);
int dsm_ip_host_accept(uint32_t num_inliers, double tz, double tri_angle, const dsm_initial_pair_options* o, double* margins);
int dsm_ip_host_point_gates(const double* qvec, const double* tvec, const double* X, double min_tri_angle_deg, double* angle, double* margins);
int dsm_ip_host_candidates(uint32_t, const uint32_t*, const uint8_t*, const uint32_t*, uint32_t, const uint32_t*, const uint64_t*, const uint32_t*,
                           uint32_t, const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, const uint64_t*, const uint32_t*,
                           const uint32_t*, const uint32_t*, const dsm_initial_pair_options*, int, uint64_t*, uint32_t*, uint64_t, uint32_t*,
                           const char**);
}

#define CHECK(c)                                                     \
  do {                                                               \
    if (!(c)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      exit(1);                                                       \
    }                                                                \
  } while (0)

struct Scene {
  std::vector<uint32_t> image_ids, poff{0}, pairs, matches, prob_off{0}, prob_ids, regs, trials, tried, seed1, seed2;
  std::vector<uint8_t> prior;
  std::vector<uint64_t> moff{0}, tried_off{0};
  void image(uint32_t id, bool has_prior, uint32_t n_points) {
    image_ids.push_back(id), prior.push_back(has_prior), poff.push_back(poff.back() + n_points);
  }
  void pair(uint32_t id1, uint32_t id2, uint32_t n, uint32_t duplicates = 0) {  // n distinct matches (i, i), then repeats of feature 0
    pairs.push_back(id1), pairs.push_back(id2);
    for (uint32_t i = 0; i < n; ++i) matches.push_back(i), matches.push_back(i);
    for (uint32_t i = 0; i < duplicates; ++i) matches.push_back(0), matches.push_back(n + i);
    moff.push_back(matches.size() / 2);
  }
  void problem(std::vector<uint32_t> ids, uint32_t s1 = DSM_NO_IMAGE, uint32_t s2 = DSM_NO_IMAGE) {
    prob_ids.insert(prob_ids.end(), ids.begin(), ids.end());
    prob_off.push_back(prob_ids.size());
    regs.resize(prob_ids.size(), 0), trials.resize(prob_ids.size(), 0);
    tried_off.push_back(tried.size() / 2);
    seed1.push_back(s1), seed2.push_back(s2);
  }
};

static int run(const Scene& s, const dsm_initial_pair_options& o, int sorted, std::vector<uint64_t>* off, std::vector<uint32_t>* out,
               const char** why = nullptr) {
  const uint32_t P = (uint32_t)s.seed1.size();
  off->assign(P + 1, 0);
  out->assign(2 * (s.pairs.size() / 2) * (size_t)P + 2, 0);
  const char* w = nullptr;
  const int rc = dsm_ip_host_candidates((uint32_t)s.image_ids.size(), s.image_ids.data(), s.prior.data(), s.poff.data(), (uint32_t)(s.pairs.size() / 2),
                                        s.pairs.data(), s.moff.data(), s.matches.data(), P, s.prob_off.data(), s.prob_ids.data(), s.regs.data(),
                                        s.trials.data(), s.tried_off.data(), s.tried.data(), s.seed1.data(), s.seed2.data(), &o, sorted, off->data(),
                                        out->data(), out->size() / 2, nullptr, &w);
  if (why) *why = w;
  if (rc == DSM_OK) out->resize(2 * off->back());
  return rc;
}

static void both_agree(const Scene& s, const dsm_initial_pair_options& o, std::vector<uint64_t>* off, std::vector<uint32_t>* out) {
  std::vector<uint64_t> off2;
  std::vector<uint32_t> out2;
  CHECK(run(s, o, 0, off, out) == DSM_OK);
  CHECK(run(s, o, 1, &off2, &out2) == DSM_OK);
  CHECK(*off == off2 && *out == out2);
}

static uint32_t rnd(uint64_t* st) {
  *st = *st * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(*st >> 33);
}

int main() {
  dsm_initial_pair_options o;
  dsm_ip_host_default_options(&o);
  CHECK(o.init_min_num_inliers == 100 && o.init_max_reg_trials == 2 && o.init_max_error == 4.0 && o.init_max_forward_motion == 0.95 &&
        o.init_min_tri_angle == 16.0 && o.user_seed == 0 && o.speculation_window >= 1);
  o.init_min_num_inliers = 30;
  std::vector<uint64_t> off;
  std::vector<uint32_t> out;
  {  // four images, 7 without a prior; NumCorrespondences 5: 104, 3: 90, 9: 85, 7: 129; (9, 5) keeps exactly 30, (5, 7) 29 of 33
    Scene s;
    s.image(5, true, 200), s.image(3, true, 200), s.image(9, true, 200), s.image(7, false, 200);
    s.pair(3, 5, 45), s.pair(9, 5, 30), s.pair(7, 3, 45), s.pair(9, 7, 55), s.pair(5, 7, 29, 4);
    s.problem({3, 5, 7, 9});
    both_agree(s, o, &off, &out);
    // 5: 3 (45), 9 (30), not 7 (29); 3: 5 again, then 7; 9: 5 again, then 7; 7 (no prior, so last): nothing new
    const std::vector<uint32_t> want = {5, 3, 5, 9, 3, 7, 9, 7};
    CHECK(out == want);
    s.tried = {7, 9}, s.tried_off.back() = 1;
    both_agree(s, o, &off, &out);
    CHECK((out == std::vector<uint32_t>{5, 3, 5, 9, 3, 7}));
    s.regs[0] = 1;  // image 3 is registered elsewhere: neither first nor second
    both_agree(s, o, &off, &out);
    CHECK((out == std::vector<uint32_t>{5, 9}));
    s.regs[0] = 0, s.trials[3] = 2;  // image 9 has used its trials: a second image only
    both_agree(s, o, &off, &out);
    CHECK((out == std::vector<uint32_t>{5, 3, 5, 9, 3, 7}));
    s.trials[3] = 0, s.tried.clear(), s.tried_off.back() = 0;
    s.seed2[0] = 7;  // one seed: the first list is image 7 alone
    both_agree(s, o, &off, &out);
    CHECK((out == std::vector<uint32_t>{7, 9, 7, 3}));
    s.seed1[0] = 5;  // both: that pair, although it keeps 29 matches only
    both_agree(s, o, &off, &out);
    CHECK((out == std::vector<uint32_t>{5, 7}));
    const char* why = nullptr;
    s.seed1[0] = 11;
    CHECK(run(s, o, 0, &off, &out, &why) == DSM_ERR_INVALID_ARGUMENT && why);
    s.seed1[0] = DSM_NO_IMAGE, s.prob_ids[1] = 3;
    CHECK(run(s, o, 0, &off, &out, &why) == DSM_ERR_INVALID_ARGUMENT && why);
    s.prob_ids[1] = 4;
    CHECK(run(s, o, 0, &off, &out, &why) == DSM_ERR_INVALID_ARGUMENT && why);
    s.prob_ids[1] = 5;
    dsm_initial_pair_options bad = o;
    bad.speculation_window = 0;
    CHECK(run(s, bad, 0, &off, &out, &why) == DSM_ERR_INVALID_ARGUMENT && why);
  }
  uint64_t st = 12345;
  for (int trial = 0; trial < 200; ++trial) {  // random scenes with ties everywhere: both forms agree
    Scene s;
    const uint32_t n = 2 + rnd(&st) % 9;
    for (uint32_t i = 0; i < n; ++i) s.image(100 + 7 * ((i * 5) % n) + (i * 5) / n, rnd(&st) % 4 != 0, 64);
    for (uint32_t a = 0; a < n; ++a)
      for (uint32_t b = a + 1; b < n; ++b)
        if (rnd(&st) % 3) {
          const uint32_t cnt = 28 + rnd(&st) % 5, dup = rnd(&st) % 3;
          if (rnd(&st) % 2)
            s.pair(s.image_ids[a], s.image_ids[b], cnt, dup);
          else
            s.pair(s.image_ids[b], s.image_ids[a], cnt, dup);
        }
    const uint32_t P = 1 + rnd(&st) % 3;
    for (uint32_t p = 0; p < P; ++p) {
      std::vector<uint32_t> ids;
      for (uint32_t i = 0; i < n; ++i)
        if (p == 0 || rnd(&st) % 3) ids.push_back(s.image_ids[n - 1 - i]);
      s.problem(ids);
      for (size_t i = s.prob_off[p]; i < s.prob_off[p + 1]; ++i) s.regs[i] = rnd(&st) % 8 == 0, s.trials[i] = rnd(&st) % 3;
      if (ids.size() >= 2 && rnd(&st) % 4 == 0) s.tried.push_back(ids[0]), s.tried.push_back(ids[1]);
      s.tried_off.back() = s.tried.size() / 2;
      if (!ids.empty() && rnd(&st) % 5 == 0) s.seed1.back() = ids[rnd(&st) % ids.size()];
    }
    s.tried.push_back(0), s.tried.push_back(0);  // (never read: data() of an empty vector may be NULL)
    o.init_min_num_inliers = 28 + (int32_t)(rnd(&st) % 4);
    both_agree(s, o, &off, &out);
  }
  // the exact pieces at their edges
  CHECK(dsm_ip_host_acos(1.0) == 0.0 && std::isnan(dsm_ip_host_acos(1.0000000000000002)));
  const double c1[3] = {0, 0, 0}, c2[3] = {1, 0, 0}, X[3] = {0.5, 0, 1};
  CHECK(std::fabs(dsm_ip_host_tri_angle(c1, c2, X) - 2 * std::atan(0.5)) < 1e-15);
  CHECK(dsm_ip_host_tri_angle(c1, c2, c1) == 0.0);  // a zero ray: the reference returns 0
  const double odd[5] = {0.5, 0.1, 0.9, 0.3, 0.7}, even[4] = {0.4, 0.1, 0.3, 0.2}, one[1] = {0.25};
  CHECK(dsm_ip_host_median(odd, 5) == 0.5 && dsm_ip_host_median(even, 4) == (0.3 + 0.2) / 2.0 && dsm_ip_host_median(one, 1) == 0.25);
  const double q[4] = {1, 0, 0, 0}, t[3] = {-1, 0, 0};
  double P[12], C[3], C2[3], mg[2], angle;
  dsm_ip_host_pose(q, t, P, C, C2);
  CHECK(P[0] == 1 && P[3] == -1 && C[0] == 1 && C[1] == 0 && C2[0] == 1);
  dsm_ip_host_default_options(&o);
  CHECK(dsm_ip_host_accept(100, 0.5, 0.3, &o, mg) == 1 && mg[0] > 0.4 && mg[1] > 0.05);
  CHECK(dsm_ip_host_accept(99, 0.5, 0.3, &o, mg) == 0 && std::isinf(mg[0]) && std::isinf(mg[1]));
  CHECK(dsm_ip_host_accept(100, -0.95, 0.3, &o, mg) == 0 && mg[0] == 0.0 && std::isinf(mg[1]));
  CHECK(dsm_ip_host_accept(100, 0.5, 16.0 * 0.0174532925199432954743716805978692718781530857086181640625, &o, mg) == 0 && mg[1] == 0.0);
  CHECK(dsm_ip_host_point_gates(q, t, X, 16.0, &angle, mg) == 1 && mg[0] > 1.0 && mg[1] > 0.9);
  const double behind[3] = {0.5, 0, -1};
  CHECK(dsm_ip_host_point_gates(q, t, behind, 16.0, &angle, mg) == 0);
  printf("initial_pair_selftest ok\n");
  return 0;
}
