// initial_pair_host.cpp -- the host build of initial_pair.h: the candidate order of FindInitialImagePair, the
// triangulation angle, Median, the acceptance tests and the point gates on one CPU thread from the text the kernels are built
// from.  What the CPU test holds to tests/initial_pair_ref.py bit for bit, the host half of the baseline of
// tools/bench_initial_pair.py, and what `make initial-pair-selftest` runs under the sanitizers.  Two forms of the candidate
// order: the reference's nested loops (ip_serial_order, the text of DSM_INITIAL_PAIR_SERIAL) and the device's schedule, the
// packed keys of the kernels under std::sort.  No HIP.
#include <cstring>

#define DSM_XT static inline
#define DSM_XT_CONST static const
#define IP_HD static inline
#define IP_D static inline
#include "initial_pair.h"

extern "C" double dsm_ip_host_acos(double q) { return dsm_acos(q); }
extern "C" void dsm_ip_host_default_options(dsm_initial_pair_options* o) { ip_default_options(o); }
extern "C" double dsm_ip_host_min_tri_angle_rad(double deg) { return deg * IP_DEG_TO_RAD; }
extern "C" double dsm_ip_host_tri_angle(const double* c1, const double* c2, const double* X) { return ip_tri_angle(c1, c2, X); }
extern "C" double dsm_ip_host_median(const double* a, uint64_t n) { return ip_median_serial(a, n); }
// image 2 through its quaternion: P [12] row-major, the centre of ProjectionCenterFromPose, and -R^T t of EstimateRelativePose
extern "C" void dsm_ip_host_pose(const double* qvec, const double* tvec, double* P, double* center, double* minus_Rt_t) {
  double R[9];
  ip_compose_P(qvec, tvec, P);
  ip_projection_center(qvec, tvec, center);
  ip_quat_to_R(qvec, R);
  ip_minus_Rt_t(R, tvec, minus_Rt_t);
}
// margins: forward, tri_angle (INFINITY where the && chain did not reach the test)
extern "C" int dsm_ip_host_accept(uint32_t num_inliers, double tz, double tri_angle, const dsm_initial_pair_options* o, double* margins) {
  IpMargins mg = {ip_inf(), ip_inf(), ip_inf(), ip_inf()};
  const bool ok = ip_accept(num_inliers, tz, tri_angle, o->init_min_num_inliers, o->init_max_forward_motion, o->init_min_tri_angle * IP_DEG_TO_RAD, &mg);
  margins[0] = mg.forward, margins[1] = mg.tri_angle;
  return ok;
}
// the gates of one triangulated point of the pair (identity, (qvec, tvec)); margins: angle, depth
extern "C" int dsm_ip_host_point_gates(const double* qvec, const double* tvec, const double* X, double min_tri_angle_deg, double* angle, double* margins) {
  const double P1[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, C1[3] = {0, 0, 0};
  double P2[12], C2[3];
  ip_compose_P(qvec, tvec, P2);
  ip_projection_center(qvec, tvec, C2);
  IpMargins mg = {ip_inf(), ip_inf(), ip_inf(), ip_inf()};
  *angle = ip_tri_angle(C1, C2, X);
  const bool ok = ip_point_gates(*angle, min_tri_angle_deg * IP_DEG_TO_RAD, P1, P2, X, &mg);
  margins[0] = mg.point_angle, margins[1] = mg.point_depth;
  return ok;
}

// Every problem's candidate list as image id pairs (image 1, image 2) in trial order: out_offsets [num_problems + 1], out_pairs
// with room for `capacity` pairs.  sorted != 0: the device's schedule.  pair_counts (or NULL) gets the kept matches of every
// pair.  0, or DSM_ERR_INVALID_ARGUMENT / DSM_ERR_OUT_OF_RANGE with *why.
extern "C" int dsm_ip_host_candidates(uint32_t num_images, const uint32_t* image_ids, const uint8_t* image_prior, const uint32_t* points2D_offsets,
                                      uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                      uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                                      const uint32_t* num_registrations, const uint32_t* init_num_reg_trials, const uint64_t* tried_offsets,
                                      const uint32_t* tried_pairs, const uint32_t* seed_image1, const uint32_t* seed_image2,
                                      const dsm_initial_pair_options* options, int sorted, uint64_t* out_offsets, uint32_t* out_pairs,
                                      uint64_t capacity, uint32_t* pair_counts, const char** why) {
  dsm_initial_pair_options o;
  if (options)
    o = *options;
  else
    ip_default_options(&o);
  IpSetup S;
  const char* bad = S.load(num_images, image_ids, image_prior, points2D_offsets, num_pairs, pair_image_ids, match_offsets, matches, num_problems,
                           problem_image_offsets, problem_image_ids, num_registrations, init_num_reg_trials, tried_offsets, tried_pairs, seed_image1,
                           seed_image2, o);
  if (!bad && !out_offsets) bad = "NULL argument";
  if (why) *why = bad;
  if (bad) return S.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> cnt(num_pairs);
  for (uint32_t k = 0; k < num_pairs; ++k)
    cnt[k] = ip_host_dedup(S.nfeat[S.pair_img[2 * k]], S.nfeat[S.pair_img[2 * k + 1]], matches ? matches + 2 * match_offsets[k] : nullptr,
                           match_offsets[k + 1] - match_offsets[k], nullptr);
  if (pair_counts && num_pairs) memcpy(pair_counts, cnt.data(), (size_t)num_pairs * 4);
  const uint32_t n_slots = (uint32_t)S.slot_img.size(), n_entries = (uint32_t)S.ent_pair.size();
  const IpOrderView v = {num_problems,      S.slot_off.data(),  S.slot_flags.data(), S.ent_off.data(), S.ent_pair.data(),
                         S.ent_slot.data(), S.ent_tried.data(), cnt.data(),          (uint32_t)std::max(o.init_min_num_inliers, 1)};
  std::vector<uint32_t> sum(n_slots + 1, 0), cand(2 * (size_t)n_entries + 1);
  std::vector<uint8_t> seen(n_entries + 1);
  uint64_t at = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    out_offsets[p] = at;
    auto emit = [&](uint32_t a, uint32_t b) {
      if (out_pairs && at < capacity) out_pairs[2 * at] = image_ids[a], out_pairs[2 * at + 1] = image_ids[b];
      ++at;
    };
    if (S.both_seed_entry[p] != -2) {
      emit(S.both_seed_img[2 * p], S.both_seed_img[2 * p + 1]);
      continue;
    }
    uint32_t n = 0;
    uint32_t* out = cand.data() + 2 * (size_t)S.ent_off[p];
    if (!sorted) {
      n = ip_serial_order(v, p, sum.data(), seen.data(), out);
    } else {  // k_ip_sums, k_ip_slot_rank, k_ip_entry_keys, k_ip_entry_rank
      const uint32_t s0 = S.slot_off[p], s1 = S.slot_off[p + 1], e0 = S.ent_off[p], e1 = S.ent_off[p + 1];
      for (uint32_t e = e0; e < e1; ++e) sum[S.ent_slot[2 * e]] += cnt[S.ent_pair[e]], sum[S.ent_slot[2 * e + 1]] += cnt[S.ent_pair[e]];
      std::vector<uint32_t> rank(s1 - s0);
      for (uint32_t s = s0; s < s1; ++s)
        for (uint32_t t = s0; t < s1; ++t) rank[s - s0] += ip_first_key(S.slot_flags[t], sum[t], t) < ip_first_key(S.slot_flags[s], sum[s], s);
      std::vector<uint64_t> key(2 * (size_t)(e1 - e0));
      for (uint32_t i = 0; i < key.size(); ++i) {
        const uint32_t e = e0 + (i >> 1), dir = i & 1u, first = S.ent_slot[2 * e + dir], other = S.ent_slot[2 * e + 1 - dir], c = cnt[S.ent_pair[e]];
        const bool ok = (S.slot_flags[first] & IP_SLOT_FIRST) && (S.slot_flags[other] & IP_SLOT_SECOND) && c >= v.min_count;
        key[i] = ok ? ((uint64_t)rank[first - s0] << 40) | ip_second_key(S.slot_flags[other], c, other) : IP_KEY_NONE;
      }
      std::vector<std::pair<uint64_t, uint32_t>> kept;
      for (uint32_t i = 0; i < key.size(); ++i)
        if (key[i] != IP_KEY_NONE && !S.ent_tried[e0 + (i >> 1)] && key[i] < key[i ^ 1u]) kept.push_back({key[i], 2 * e0 + i});
      std::sort(kept.begin(), kept.end());
      for (const auto& kv : kept) out[n++] = kv.second;
    }
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t e = out[i] >> 1, dir = out[i] & 1u, k = S.ent_pair[e];
      emit(S.pair_img[2 * (size_t)k + dir], S.pair_img[2 * (size_t)k + 1 - dir]);
    }
  }
  out_offsets[num_problems] = at;
  if (out_pairs && at > capacity) {
    if (why) *why = "out_pairs is too small";
    return DSM_ERR_OUT_OF_RANGE;
  }
  return DSM_OK;
}
