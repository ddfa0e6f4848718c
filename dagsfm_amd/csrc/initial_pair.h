// initial_pair.h -- the exact pieces of dsm_find_initial_pairs, written once for the kernels of initial_pair.hip
// and for the host build (initial_pair_host.cpp): the pose of image 2 through its quaternion, the triangulation angle, Median,
// the acceptance tests and the point gates with their margins, the reference's nested loops over one problem's images
// (ip_serial_order: the cross-check schedule DSM_INITIAL_PAIR_SERIAL, the host build and the selftest), and the host's set-up of
// a call (IpSetup: validation, the problems' slots and pair entries).  tests/initial_pair_ref.py is the normative restatement.
//
// Plain IEEE operations in a fixed order, no FMA (both builds use -ffp-contract=off).  The includer defines
//   IP_HD  qualifier of the pieces without acos   (host: `static inline`; device: `static __host__ __device__ inline`)
//   IP_D   qualifier of the pieces with acos      (host: `static inline`; device: `static __device__ inline`)
// and DSM_XT / DSM_XT_CONST for exact_acos.h.
#ifndef DAGSFM_AMD_CSRC_INITIAL_PAIR_H_
#define DAGSFM_AMD_CSRC_INITIAL_PAIR_H_

#include <float.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/dagsfm_mi355x.h"
#include "exact_acos.h"

#define IP_MAX_SLOTS 1048576u        // problem images of a call: a slot index fits 20 bits of a packed key
#define IP_MAX_COUNT 524287u         // kept matches of a pair: 19 bits of a packed key (an image holds at most 262144 points2D)
#define IP_MAX_POINTS2D 262144u      // per image: the duplicate rule's bitmap of a pair's two images fits 64 KiB
#define IP_KEY_NONE 0xffffffffffffffffull  // a directed entry that is no candidate: sorts behind every key
#define IP_DEG_TO_RAD 0.0174532925199432954743716805978692718781530857086181640625  // DegToRad, util/math.h:198-200
#define IP_PI 3.14159265358979323846

// slot flags
#define IP_SLOT_PRIOR 1u    // the image's camera has a prior focal length
#define IP_SLOT_FIRST 2u    // may be a first image: trials left and registered nowhere -- or, with one seed image, that image
#define IP_SLOT_SECOND 4u   // may be a second image: registered nowhere

struct IpMargins {
  double tri_angle, forward, point_angle, point_depth;
};

IP_HD double ip_inf() { return __builtin_inf(); }
IP_HD double ip_abs(double x) { return x < 0 ? -x : x; }
IP_HD double ip_max(double a, double b) { return a > b ? a : b; }
IP_HD void ip_take(double* m, double v) {
  if (v < *m) *m = v;
}

// NormalizeQuaternion + Eigen's toRotationMatrix (pose.cc:75-91): R row-major
IP_HD void ip_quat_to_R(const double* qv, double* R) {
  const double nq = __builtin_sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
  const double w = nq == 0 ? 1.0 : qv[0] / nq, x = nq == 0 ? qv[1] : qv[1] / nq, y = nq == 0 ? qv[2] : qv[2] / nq, z = nq == 0 ? qv[3] : qv[3] / nq;
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y,
               tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

// ComposeProjectionMatrix(qvec, tvec) (projection.cc): [R(qvec) | tvec], row-major 3 x 4
IP_HD void ip_compose_P(const double* qv, const double* tv, double* P) {
  double R[9];
  ip_quat_to_R(qv, R);
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) P[4 * r + k] = R[3 * r + k];
    P[4 * r + 3] = tv[r];
  }
}

// ProjectionCenterFromPose (pose.cc:164-171): the conjugate of the normalised quaternion applied to -tvec, Eigen's
// operator*(Quaternion, Vector3): uv = 2 (q.vec x v); v + w uv + q.vec x uv
IP_HD void ip_projection_center(const double* qv, const double* tv, double* C) {
  const double nq = __builtin_sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
  const double w = nq == 0 ? 1.0 : qv[0] / nq;
  const double q[3] = {-(nq == 0 ? qv[1] : qv[1] / nq), -(nq == 0 ? qv[2] : qv[2] / nq), -(nq == 0 ? qv[3] : qv[3] / nq)};
  const double v[3] = {-tv[0], -tv[1], -tv[2]};
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (int k = 0; k < 3; ++k) uv[k] += uv[k];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int k = 0; k < 3; ++k) C[k] = (v[k] + w * uv[k]) + c[k];
}

// -R^T t as EstimateRelativePose writes it (two_view_geometry.cc:216-217): every entry summed left to right
IP_HD void ip_minus_Rt_t(const double* R, const double* t, double* C) {
  for (int k = 0; k < 3; ++k) C[k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
}

// CalculateTriangulationAngle and one element of CalculateTriangulationAngles (triangulation.cc:122-181: the same operations)
IP_D double ip_tri_angle(const double* c1, const double* c2, const double* X) {
  double d0 = c1[0] - c2[0], d1 = c1[1] - c2[1], d2 = c1[2] - c2[2];
  const double b = (d0 * d0 + d1 * d1) + d2 * d2;
  d0 = X[0] - c1[0], d1 = X[1] - c1[1], d2 = X[2] - c1[2];
  const double r1 = (d0 * d0 + d1 * d1) + d2 * d2;
  d0 = X[0] - c2[0], d1 = X[1] - c2[1], d2 = X[2] - c2[2];
  const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
  const double den = 2.0 * __builtin_sqrt(r1 * r2);
  if (den == 0.0) return 0.0;
  const double a = dsm_acos(((r1 + r2) - b) / den);  // in [0, pi] or NaN: the reference's std::abs changes nothing
  if (!(a == a)) return a;
  const double o = IP_PI - a;
  return o < a ? o : a;
}

// Median (util/math.h:211-229) of n >= 1 angles: the element of rank n / 2, averaged with the element of rank n / 2 - 1 for an
// even n (the largest of the lower half after nth_element).  The elements are non-negative doubles or the quiet NaN, which
// order as their bits do; rank k by bisection on the bits: the largest v with |{x < v}| <= k.  `count_below(v)` counts.
template <typename CountBelow>
IP_HD uint64_t ip_select_bits(uint64_t k, CountBelow count_below) {
  uint64_t ans = 0;
  for (int b = 63; b >= 0; --b) {
    const uint64_t cand = ans | (1ull << b);
    if (count_below(cand) <= k) ans = cand;
  }
  return ans;
}
IP_HD uint64_t ip_double_bits(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return u;
}
IP_HD double ip_bits_double(uint64_t u) {
  double x;
  __builtin_memcpy(&x, &u, 8);
  return x;
}
IP_HD double ip_median_of(double mid, double below, uint64_t n) { return n % 2 == 0 ? (mid + below) / 2.0 : mid; }
// the element of rank k (0 .. n - 1) of n such elements: what nth_element leaves at position k (Median here, Percentile in
// next_images.h)
IP_HD double ip_rank_serial(const double* a, uint64_t n, uint64_t k) {
  auto count_below = [&](uint64_t v) {
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; ++i) c += ip_double_bits(a[i]) < v;
    return c;
  };
  return ip_bits_double(ip_select_bits(k, count_below));
}
IP_HD double ip_median_serial(const double* a, uint64_t n) {
  const double mid = ip_rank_serial(a, n, n / 2);
  const double below = n % 2 == 0 ? ip_rank_serial(a, n, n / 2 - 1) : 0.0;
  return ip_median_of(mid, below, n);
}

// EstimateInitialTwoViewGeometry's acceptance (incremental_mapper.cc:1166-1169) as its && chain runs: the margin of a test is
// recorded when the test is reached
IP_HD bool ip_accept(uint32_t num_inliers, double tz, double tri_angle, int32_t min_num_inliers, double max_forward, double min_tri_angle_rad,
                     IpMargins* mg) {
  if (!((int64_t)num_inliers >= (int64_t)min_num_inliers)) return false;
  const double az = ip_abs(tz);
  ip_take(&mg->forward, ip_abs(az - max_forward) / ip_max(max_forward, DBL_EPSILON));
  if (!(az < max_forward)) return false;
  ip_take(&mg->tri_angle, ip_abs(tri_angle - min_tri_angle_rad) / ip_max(min_tri_angle_rad, DBL_EPSILON));
  return tri_angle > min_tri_angle_rad;
}

// the gates of a triangulated correspondence (incremental_mapper.cc:330-334), the && chain as it runs; P row-major 3 x 4
IP_HD double ip_row2(const double* P, const double* X) { return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]; }
IP_HD bool ip_depth_ok(const double* P, const double* X, IpMargins* mg) {  // HasPointPositiveDepth (projection.cc:199-203)
  const double z = ip_row2(P, X);
  ip_take(&mg->point_depth, ip_abs(z - DBL_EPSILON) / ip_max(ip_abs(z), DBL_EPSILON));
  return z >= DBL_EPSILON;
}
IP_HD bool ip_point_gates(double angle, double min_angle_rad, const double* P1, const double* P2, const double* X, IpMargins* mg) {
  ip_take(&mg->point_angle, ip_abs(angle - min_angle_rad) / ip_max(min_angle_rad, DBL_EPSILON));
  if (!(angle >= min_angle_rad)) return false;
  if (!ip_depth_ok(P1, X, mg)) return false;
  return ip_depth_ok(P2, X, mg);
}

// ------------------------------------------------------------------ the candidate order
// One call's problems as the kernels read them.  Slots = the problems' images, problem by problem, ascending image id inside a
// problem; entries = the (problem, pair) incidences with both images in the problem, problem by problem.
struct IpOrderView {
  uint32_t n_problems;
  const uint32_t* slot_off;    // [n_problems + 1]
  const uint32_t* slot_flags;  // [slots] IP_SLOT_*
  const uint32_t* ent_off;     // [n_problems + 1]
  const uint32_t* ent_pair;    // [entries] the pair
  const uint32_t* ent_slot;    // [2 entries] the slots of the pair's images as the pair is written
  const uint8_t* ent_tried;    // [entries]
  const uint32_t* pair_cnt;    // [pairs] matches kept by the duplicate rule
  uint32_t min_count;          // max(init_min_num_inliers, 1): an image without a correspondence is not in the reference's map
};

// the key of a first image among its problem's slots and of a second image among a first image's partners: smaller = earlier
IP_HD uint64_t ip_first_key(uint32_t flags, uint32_t sum, uint32_t slot) {
  return ((uint64_t)((flags & IP_SLOT_PRIOR) ? 0u : 1u) << 52) | ((uint64_t)(~sum) << 20) | slot;
}
IP_HD uint64_t ip_second_key(uint32_t flags, uint32_t cnt, uint32_t slot) {
  return ((uint64_t)((flags & IP_SLOT_PRIOR) ? 0u : 1u) << 39) | ((uint64_t)(~cnt & IP_MAX_COUNT) << 20) | slot;
}

// FindInitialImagePair's nested loops (incremental_mapper.cc:170-193) over problem p without the estimation: every directed
// candidate in trial order as 2 * entry + direction (direction 1: the pair's second image is image 1).  `sum` [slots] and `seen`
// [entries] are work arrays.  Returns the number written to out (room for the problem's entries).
IP_HD uint32_t ip_serial_order(const IpOrderView& v, uint32_t p, uint32_t* sum, uint8_t* seen, uint32_t* out) {
  const uint32_t s0 = v.slot_off[p], s1 = v.slot_off[p + 1], e0 = v.ent_off[p], e1 = v.ent_off[p + 1];
  for (uint32_t s = s0; s < s1; ++s) sum[s] = 0;
  for (uint32_t e = e0; e < e1; ++e) {
    seen[e] = 0;
    sum[v.ent_slot[2 * e]] += v.pair_cnt[v.ent_pair[e]];
    sum[v.ent_slot[2 * e + 1]] += v.pair_cnt[v.ent_pair[e]];
  }
  uint32_t n = 0;
  bool have1 = false;
  for (uint64_t last1 = 0;;) {  // FindFirstInitialImage's list, one image at a time
    uint64_t best1 = IP_KEY_NONE;
    uint32_t first = 0;
    for (uint32_t s = s0; s < s1; ++s) {
      if (!(v.slot_flags[s] & IP_SLOT_FIRST)) continue;
      const uint64_t k = ip_first_key(v.slot_flags[s], sum[s], s);
      if ((!have1 || k > last1) && k < best1) best1 = k, first = s;
    }
    if (best1 == IP_KEY_NONE) break;
    last1 = best1, have1 = true;
    bool have2 = false;
    for (uint64_t last2 = 0;;) {  // FindSecondInitialImage's list of `first`
      uint64_t best2 = IP_KEY_NONE;
      uint32_t pick = 0;
      for (uint32_t e = e0; e < e1; ++e) {
        const uint32_t a = v.ent_slot[2 * e], b = v.ent_slot[2 * e + 1];
        if (a != first && b != first) continue;
        const uint32_t other = a == first ? b : a, cnt = v.pair_cnt[v.ent_pair[e]];
        if (!(v.slot_flags[other] & IP_SLOT_SECOND) || cnt < v.min_count) continue;
        const uint64_t k = ip_second_key(v.slot_flags[other], cnt, other);
        if ((!have2 || k > last2) && k < best2) best2 = k, pick = 2 * e + (b == first ? 1u : 0u);
      }
      if (best2 == IP_KEY_NONE) break;
      last2 = best2, have2 = true;
      const uint32_t e = pick >> 1;
      if (seen[e] || v.ent_tried[e]) continue;  // "Try every pair only once."
      seen[e] = 1;
      out[n++] = pick;
    }
  }
  return n;
}

// ------------------------------------------------------------------ the host's set-up of a call (host code only)
static inline void ip_default_options(dsm_initial_pair_options* o) {
  o->init_min_num_inliers = 100;  // IncrementalMapper::Options, incremental_mapper.h:68-81
  o->init_max_reg_trials = 2;
  o->init_max_error = 4.0;
  o->init_max_forward_motion = 0.95;
  o->init_min_tri_angle = 16.0;
  o->user_seed = 0;
  o->speculation_window = 64;  // the fastest of 1, 4, 16, 64 on 32 clusters of 60 images
}

static inline const char* ip_options_error(const dsm_initial_pair_options& o) {
  if (o.init_min_num_inliers < 0) return "init_min_num_inliers below 0";
  if (o.init_max_reg_trials < 1) return "init_max_reg_trials below 1";
  if (!(o.init_max_error > 0) || !std::isfinite(o.init_max_error)) return "init_max_error must be positive and finite";
  if (!(o.init_max_forward_motion >= 0 && o.init_max_forward_motion <= 1)) return "init_max_forward_motion outside [0, 1]";
  if (!(o.init_min_tri_angle >= 0) || !std::isfinite(o.init_min_tri_angle)) return "init_min_tri_angle must be finite and not negative";
  if (o.speculation_window < 1) return "speculation_window below 1";
  return nullptr;
}

// the duplicate rule of CorrespondenceGraph::AddCorrespondences for one pair in match order (the host's text of k_rt_dedup)
static inline uint32_t ip_host_dedup(uint32_t n1, uint32_t n2, const uint32_t* m, uint64_t n, uint8_t* acc) {
  std::vector<uint8_t> used((size_t)n1 + n2, 0);
  uint32_t kept = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t a = m[2 * i], b = n1 + m[2 * i + 1];
    const bool ok = !used[a] && !used[b];
    if (ok) used[a] = used[b] = 1;
    if (acc) acc[i] = ok;
    kept += ok;
  }
  return kept;
}

// indices 0 .. n - 1 in ascending key[index]: the one sort of the set-up (keys are unique wherever the order matters)
static __attribute__((noinline)) void ip_sort_indices(std::vector<uint32_t>& idx, uint32_t n, const uint64_t* key) {
  idx.resize(n);
  std::iota(idx.begin(), idx.end(), 0u);
  std::sort(idx.begin(), idx.end(), [key](uint32_t a, uint32_t b) { return key[a] < key[b]; });
}

struct IpSetup {
  std::vector<uint32_t> id_order;                 // image indices by ascending id
  std::vector<uint32_t> nfeat, pair_img;          // per image; 2 per pair (image indices as the pair is written)
  std::vector<uint32_t> slot_off, slot_img, slot_flags, ent_off, ent_pair, ent_slot;
  std::vector<uint8_t> ent_tried;
  std::vector<int64_t> both_seed_entry;           // per problem: -2 = a search; else the entry of (seed1, seed2), -1 = no such pair
  std::vector<uint32_t> both_seed_img;            // 2 per problem (image indices), where both seeds are given
  bool out_of_range = false;

  int64_t find_img(const uint32_t* image_ids, uint32_t id) const {
    auto it = std::lower_bound(id_order.begin(), id_order.end(), id, [&](uint32_t a, uint32_t v) { return image_ids[a] < v; });
    return (it != id_order.end() && image_ids[*it] == id) ? (int64_t)*it : -1;
  }

  // the message of the first invalid argument, or NULL.  image_prior [num_images]: the prior flag of every image's camera.
  const char* load(uint32_t num_images, const uint32_t* image_ids, const uint8_t* image_prior, const uint32_t* points2D_offsets,
                   uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                   uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                   const uint32_t* num_registrations, const uint32_t* init_num_reg_trials, const uint64_t* tried_offsets,
                   const uint32_t* tried_pairs, const uint32_t* seed_image1, const uint32_t* seed_image2, const dsm_initial_pair_options& o) {
    if (const char* bad = ip_options_error(o)) return bad;
    if ((num_images && (!image_ids || !image_prior)) || !points2D_offsets || !match_offsets || (num_pairs && !pair_image_ids) ||
        !problem_image_offsets || (!tried_offsets != !tried_pairs && tried_offsets && tried_offsets[num_problems]))
      return "NULL argument";
    std::vector<uint64_t> wide(image_ids, image_ids + num_images);
    ip_sort_indices(id_order, num_images, wide.data());
    for (uint32_t i = 0; i < num_images; ++i) {
      if (image_ids[i] == DSM_NO_IMAGE) return "an image id of 0xFFFFFFFF";
      if (i && image_ids[id_order[i]] == image_ids[id_order[i - 1]]) return "a repeated image id";
    }
    if (points2D_offsets[0] != 0) return "points2D offsets must start at 0";
    nfeat.resize(num_images);
    for (uint32_t i = 0; i < num_images; ++i) {
      if (points2D_offsets[i + 1] < points2D_offsets[i]) return "points2D offsets must be non-decreasing";
      nfeat[i] = points2D_offsets[i + 1] - points2D_offsets[i];
      if (nfeat[i] > IP_MAX_POINTS2D) return "more than 262144 points2D in one image";
    }
    if (match_offsets[0] != 0) return "match offsets must start at 0";
    pair_img.resize(2 * (size_t)num_pairs);
    std::vector<uint64_t> keys(num_pairs);
    for (uint32_t k = 0; k < num_pairs; ++k) {
      if (match_offsets[k + 1] < match_offsets[k]) return "match offsets must be non-decreasing";
      if (match_offsets[k + 1] > match_offsets[k] && !matches) return "NULL argument";
      const int64_t a = find_img(image_ids, pair_image_ids[2 * k]), b = find_img(image_ids, pair_image_ids[2 * k + 1]);
      if (a < 0 || b < 0) return "a pair on an unknown image id";
      if (a == b) return "a self-pair";
      pair_img[2 * k] = (uint32_t)a, pair_img[2 * k + 1] = (uint32_t)b;
      keys[k] = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
      for (uint64_t m = match_offsets[k]; m < match_offsets[k + 1]; ++m)
        if (matches[2 * m] >= nfeat[a] || matches[2 * m + 1] >= nfeat[b]) return "a match index out of range";
    }
    if (match_offsets[num_pairs] >= 0x20000000u) return "too many matches";
    std::vector<uint32_t> by_key;
    ip_sort_indices(by_key, num_pairs, keys.data());
    for (uint32_t k = 1; k < num_pairs; ++k)
      if (keys[by_key[k]] == keys[by_key[k - 1]]) return "a repeated pair";
    auto find_pair = [&](uint32_t a, uint32_t b) -> int64_t {
      const uint64_t key = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
      auto it = std::lower_bound(by_key.begin(), by_key.end(), key, [&](uint32_t x, uint64_t v) { return keys[x] < v; });
      return (it != by_key.end() && keys[*it] == key) ? (int64_t)*it : -1;
    };
    // the slots
    if (problem_image_offsets[0] != 0) return "problem image offsets must start at 0";
    for (uint32_t p = 0; p < num_problems; ++p)
      if (problem_image_offsets[p + 1] < problem_image_offsets[p]) return "problem image offsets must be non-decreasing";
    const uint32_t S = problem_image_offsets[num_problems];
    if (S && !problem_image_ids) return "NULL argument";
    if (S > IP_MAX_SLOTS || num_problems > IP_MAX_SLOTS) {
      out_of_range = true;
      return "more than 2^20 problem images";
    }
    slot_off.assign(problem_image_offsets, problem_image_offsets + num_problems + 1);
    slot_img.resize(S), slot_flags.resize(S);
    both_seed_entry.assign(num_problems, -2);
    both_seed_img.assign(2 * (size_t)num_problems, 0);
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> img_slots(num_images);  // per image: (problem, slot), ascending problem
    std::vector<uint32_t> order;
    for (uint32_t p = 0; p < num_problems; ++p) {
      const uint32_t s0 = slot_off[p], n = slot_off[p + 1] - s0;
      wide.assign(problem_image_ids + s0, problem_image_ids + s0 + n);
      ip_sort_indices(order, n, wide.data());
      const uint32_t sd1 = seed_image1 ? seed_image1[p] : DSM_NO_IMAGE, sd2 = seed_image2 ? seed_image2[p] : DSM_NO_IMAGE;
      if (sd1 != DSM_NO_IMAGE && sd1 == sd2) return "the same seed image twice";
      const bool both = sd1 != DSM_NO_IMAGE && sd2 != DSM_NO_IMAGE, one = !both && (sd1 != DSM_NO_IMAGE || sd2 != DSM_NO_IMAGE);
      const uint32_t the_seed = sd1 != DSM_NO_IMAGE ? sd1 : sd2;
      bool found1 = sd1 == DSM_NO_IMAGE, found2 = sd2 == DSM_NO_IMAGE;
      for (uint32_t j = 0; j < n; ++j) {
        const uint32_t src = s0 + order[j], id = problem_image_ids[src];
        if (j && id == problem_image_ids[s0 + order[j - 1]]) return "a repeated image inside a problem";
        const int64_t im = find_img(image_ids, id);
        if (im < 0) return "a problem image that is not an image of the scene";
        const uint32_t s = s0 + j, regs = num_registrations ? num_registrations[src] : 0, trials = init_num_reg_trials ? init_num_reg_trials[src] : 0;
        slot_img[s] = (uint32_t)im;
        uint32_t f = image_prior[im] ? IP_SLOT_PRIOR : 0u;
        if (one ? id == the_seed : (regs == 0 && (uint64_t)trials < (uint64_t)o.init_max_reg_trials)) f |= IP_SLOT_FIRST;
        if (regs == 0) f |= IP_SLOT_SECOND;
        slot_flags[s] = both ? 0u : f;
        if (id == sd1) found1 = true, both_seed_img[2 * p] = (uint32_t)im;
        if (id == sd2) found2 = true, both_seed_img[2 * p + 1] = (uint32_t)im;
        img_slots[im].push_back({p, s});
      }
      if (!found1 || !found2) return "a seed image outside its problem";
      if (both) both_seed_entry[p] = -1;
    }
    // the entries: a pair is in the problems both of its images are in
    std::vector<std::vector<uint32_t>> per_problem(num_problems);  // (pair, slot a, slot b) triples
    for (uint32_t k = 0; k < num_pairs; ++k) {
      const auto &A = img_slots[pair_img[2 * k]], &B = img_slots[pair_img[2 * k + 1]];
      for (size_t i = 0, j = 0; i < A.size() && j < B.size();) {
        if (A[i].first < B[j].first) {
          ++i;
        } else if (B[j].first < A[i].first) {
          ++j;
        } else {
          auto& t = per_problem[A[i].first];
          t.push_back(k), t.push_back(A[i].second), t.push_back(B[j].second);
          ++i, ++j;
        }
      }
    }
    ent_off.assign(num_problems + 1, 0);
    for (uint32_t p = 0; p < num_problems; ++p) {
      const uint64_t next = (uint64_t)ent_off[p] + per_problem[p].size() / 3;
      if (next > 0x7fffffffu) {
        out_of_range = true;
        return "more than 2^31 pairs over all problems";
      }
      ent_off[p + 1] = (uint32_t)next;
    }
    const uint32_t E = ent_off[num_problems];
    ent_pair.resize(E), ent_slot.resize(2 * (size_t)E), ent_tried.assign(E, 0);
    for (uint32_t p = 0; p < num_problems; ++p) {
      const auto& t = per_problem[p];
      for (size_t i = 0; i < t.size() / 3; ++i) {
        const uint32_t e = ent_off[p] + (uint32_t)i;
        ent_pair[e] = t[3 * i], ent_slot[2 * e] = t[3 * i + 1], ent_slot[2 * e + 1] = t[3 * i + 2];
      }
      auto entry_of = [&](uint32_t a, uint32_t b) -> int64_t {  // the problem's entry of the pair of images a, b; its pairs ascend
        const int64_t k = find_pair(a, b);
        if (k < 0) return -1;
        auto first = ent_pair.begin() + ent_off[p], last = ent_pair.begin() + ent_off[p + 1];
        auto it = std::lower_bound(first, last, (uint32_t)k);
        return (it != last && *it == (uint32_t)k) ? (int64_t)(it - ent_pair.begin()) : -1;
      };
      if (both_seed_entry[p] == -1) both_seed_entry[p] = entry_of(both_seed_img[2 * p], both_seed_img[2 * p + 1]);
      if (!tried_offsets) continue;
      if (p == 0 && tried_offsets[0] != 0) return "tried offsets must start at 0";
      if (tried_offsets[p + 1] < tried_offsets[p]) return "tried offsets must be non-decreasing";
      for (uint64_t i = tried_offsets[p]; i < tried_offsets[p + 1]; ++i) {  // a tried pair the problem does not hold changes nothing
        const int64_t a = find_img(image_ids, tried_pairs[2 * i]), b = find_img(image_ids, tried_pairs[2 * i + 1]);
        if (a < 0 || b < 0 || a == b) continue;
        const int64_t e = entry_of((uint32_t)a, (uint32_t)b);
        if (e >= 0) ent_tried[e] = 1;
      }
    }
    return nullptr;
  }
};

#endif  // DAGSFM_AMD_CSRC_INITIAL_PAIR_H_
