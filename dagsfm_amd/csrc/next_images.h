// next_images.h -- the exact pieces of dsm_find_next_images and dsm_find_local_bundles, written once for the kernels of next_images.hip and
// for the host build (next_images_host.cpp): the pyramid cell of a point2D, the visibility score from a 64 x 64 occupancy, the
// packed rank key, the sequential forms of the whole call (ni_serial_*: the cross-check schedule DSM_NEXT_IMAGES_SERIAL, the
// host build and the selftest) and the host's set-up of a call (NiSetup: validation, the problems' slots and pair entries);
// for the local bundles the percentile index, the overlap key, the selection chain (lb_select) and the sequential forms lb_serial_*.
// tests/next_images_ref.py is the normative restatement.
//   IncrementalMapper::FindNextImages, the three ranks      src/sfm/incremental_mapper.cc:202-256, 46-73
//   Image::Increment/DecrementCorrespondenceHasPoint3D      src/base/image.cc:113-137
//   VisibilityPyramid::SetPoint / ResetPoint / CellForPoint src/base/visibility_pyramid.cc:53-106
//
// Integer operations and two IEEE operations per coordinate in a fixed order.  The includer defines IP_HD, IP_D, DSM_XT and
// DSM_XT_CONST as initial_pair.h asks.
#ifndef DAGSFM_AMD_CSRC_NEXT_IMAGES_H_
#define DAGSFM_AMD_CSRC_NEXT_IMAGES_H_

#include "initial_pair.h"

#define NI_LEVELS 6                       // Image::kNumPoint3DVisibilityPyramidLevels (image.h)
#define NI_DIM 64u                        // 1 << NI_LEVELS: the cells of the finest level per axis
#define NI_KEY_NONE 0xffffffffffffffffull  // a slot that is not eligible: sorts behind every key (no image id is 0xFFFFFFFF)

// slot flags
#define NI_SLOT_REGISTERED 1u  // Image::IsRegistered
#define NI_SLOT_SECOND 2u      // filtered before, or tried before: the second bucket (:244-248)
#define NI_SLOT_EXHAUSTED 4u   // num_reg_trials >= max_reg_trials (:236-239)

// VisibilityPyramid::CellForPoint for one axis: Clip(size_t(64 * x / extent), 0, 63) with the product and the quotient rounded
// in double in that order.  x is finite and not negative (NiSetup::load), extent > 0; a quotient of 64 or more -- an infinite
// product included -- is the clipped cell 63
IP_HD uint32_t ni_cell(double x, uint64_t extent) {
  const double prod = 64.0 * x;
  const double q = prod / (double)extent;
  return q < 64.0 ? (uint32_t)q : NI_DIM - 1u;
}

// one row of the next coarser level from two rows of a level: a cell is occupied when one of its 2 x 2 children is; bit cx of
// the result is the OR of bits 2 cx and 2 cx + 1 of both rows
IP_HD uint64_t ni_coarsen(uint64_t row_a, uint64_t row_b) {
  uint64_t x = row_a | row_b;
  x = (x | (x >> 1)) & 0x5555555555555555ull;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0f0f0f0f0f0f0f0full;
  x = (x | (x >> 4)) & 0x00ff00ff00ff00ffull;
  x = (x | (x >> 8)) & 0x0000ffff0000ffffull;
  x = (x | (x >> 16)) & 0x00000000ffffffffull;
  return x;
}

// what an occupied cell of level l (0 .. 5) adds: level.size() = dim_l^2, dim_l = 2^(l + 1)
IP_HD uint64_t ni_level_weight(int level) { return 1ull << (2 * (level + 1)); }

// VisibilityPyramid::Score of the occupancy rows[cy] bit cx of the finest level: the sum over the levels of occupied cells x
// dim_l^2.  The reference's per-cell counts are multiplicities of this occupancy.  `rows` is overwritten.
IP_HD uint64_t ni_score(uint64_t* rows) {
  uint64_t score = 0;
  uint32_t dim = NI_DIM;
  for (int level = NI_LEVELS - 1; level >= 0; --level, dim /= 2) {
    uint32_t occupied = 0;
    for (uint32_t r = 0; r < dim; ++r) occupied += (uint32_t)__builtin_popcountll(rows[r]);
    score += occupied * ni_level_weight(level);
    for (uint32_t r = 0; r < dim / 2; ++r) rows[r] = ni_coarsen(rows[2 * r], rows[2 * r + 1]);
  }
  return score;
}

// the rank as the reference computes it, a float (incremental_mapper.cc:62-73).  Counts are at most 262144 and scores are
// multiples of 4 of at most 17895696 < 2^26: both casts are exact, only the quotient rounds
IP_HD float ni_rank(int32_t method, uint32_t num_visible, uint32_t num_observations, uint64_t score) {
  if (method == 0) return (float)num_visible;
  if (method == 1) return (float)num_visible / (float)num_observations;
  return (float)score;
}

// the packed key of a slot among its problem's slots, smaller = earlier: bucket, the rank descending, the image id ascending.
// An eligible image has a rank that is positive and finite, so its float's bits order as the floats do and fit 31 bits.
IP_HD uint64_t ni_key(uint32_t flags, bool eligible, float rank, uint32_t image_id) {
  if (!eligible) return NI_KEY_NONE;
  uint32_t bits;
  __builtin_memcpy(&bits, &rank, 4);
  return ((uint64_t)((flags & NI_SLOT_SECOND) ? 1u : 0u) << 63) | ((uint64_t)(0x7fffffffu - (bits & 0x7fffffffu)) << 32) | image_id;
}
IP_HD bool ni_eligible(uint32_t flags, uint32_t num_visible, uint32_t min_num_inliers) {
  return !(flags & (NI_SLOT_REGISTERED | NI_SLOT_EXHAUSTED)) && num_visible >= min_num_inliers;
}

// One call's (or one batch's) problems as the kernels read them.  Slots = the problems' images in the caller's order; entries =
// the (problem, pair) incidences with both images in the problem, problem by problem.
struct NiView {
  uint32_t n_problems, n_slots, n_entries;
  const uint32_t* slot_off;     // [n_problems + 1]
  const uint32_t* slot_img;     // [slots] the image's index
  const uint32_t* slot_id;      // [slots] the image's id
  const uint32_t* slot_flags;   // [slots] NI_SLOT_*
  const uint64_t* obs_off;      // [slots + 1] the slots' observations: one per point2D
  const int32_t* obs_point;     // the point of an observation, or -1
  const uint64_t* word_off;     // [slots + 1] the slots' bitmap words: one bit per point2D
  const uint32_t* ent_off;      // [n_problems + 1]
  const uint32_t* ent_pair;     // [entries] the pair
  const uint32_t* ent_slot;     // [2 entries] the slots of the pair's images as the pair is written
  const uint64_t* moff;         // the scene's pairs
  const uint32_t* matches;
  const uint8_t* acc;           // [matches] kept by the duplicate rule
  const uint32_t* row0;         // [images] the first point2D of an image
  const double* kp;             // points2D_xy
  const uint64_t* img_wh;       // [2 images] the camera's width and height
  uint32_t* vis;                // bitmap: a correspondence of the point2D has a point
  uint32_t* has;                // bitmap: the point2D has a correspondence in the problem
  uint32_t* num_visible;        // [slots]
  uint32_t* num_observations;   // [slots]
  uint64_t* score;              // [slots] 0 for a registered slot
  uint64_t* key;                // [slots]
  uint32_t* order;              // [slots] problem p's ranked image ids from slot_off[p]
  uint32_t* order_n;            // [n_problems]
  int32_t method;
  uint32_t min_num_inliers;
};

// ------------------------------------------------------------------ the sequential forms
// the bitmaps of problem p (zero before): ruling 1 of DESIGN.md 30 over the kept matches of the problem's pairs
IP_HD void ni_serial_visibility(const NiView& v, uint32_t p) {
  for (uint32_t e = v.ent_off[p]; e < v.ent_off[p + 1]; ++e) {
    const uint32_t k = v.ent_pair[e], sa = v.ent_slot[2 * e], sb = v.ent_slot[2 * e + 1];
    for (uint64_t m = v.moff[k]; m < v.moff[k + 1]; ++m) {
      if (!v.acc[m]) continue;
      const uint32_t a = v.matches[2 * m], b = v.matches[2 * m + 1];
      v.has[v.word_off[sa] + (a >> 5)] |= 1u << (a & 31);
      v.has[v.word_off[sb] + (b >> 5)] |= 1u << (b & 31);
      if (v.obs_point[v.obs_off[sa] + a] >= 0) v.vis[v.word_off[sb] + (b >> 5)] |= 1u << (b & 31);
      if (v.obs_point[v.obs_off[sb] + b] >= 0) v.vis[v.word_off[sa] + (a >> 5)] |= 1u << (a & 31);
    }
  }
}

// the counts, the score and the key of slot s from its bitmaps
IP_HD void ni_serial_slot(const NiView& v, uint32_t s) {
  const uint64_t w0 = v.word_off[s], w1 = v.word_off[s + 1];
  uint32_t nv = 0, no = 0;
  for (uint64_t w = w0; w < w1; ++w) nv += (uint32_t)__builtin_popcount(v.vis[w]), no += (uint32_t)__builtin_popcount(v.has[w]);
  const uint32_t flags = v.slot_flags[s], img = v.slot_img[s];
  uint64_t score = 0;
  if (!(flags & NI_SLOT_REGISTERED)) {
    uint64_t rows[NI_DIM];
    for (uint32_t r = 0; r < NI_DIM; ++r) rows[r] = 0;
    const uint32_t n = (uint32_t)(v.obs_off[s + 1] - v.obs_off[s]);
    for (uint32_t f = 0; f < n; ++f) {
      if (!((v.vis[w0 + (f >> 5)] >> (f & 31)) & 1u)) continue;
      const double* xy = v.kp + 2 * ((size_t)v.row0[img] + f);
      rows[ni_cell(xy[1], v.img_wh[2 * img + 1])] |= 1ull << ni_cell(xy[0], v.img_wh[2 * img]);
    }
    score = ni_score(rows);
  }
  v.num_visible[s] = nv, v.num_observations[s] = no, v.score[s] = score;
  v.key[s] = ni_key(flags, ni_eligible(flags, nv, v.min_num_inliers), ni_rank(v.method, nv, no, score), v.slot_id[s]);
}

// FindNextImages' two sorted buckets of problem p: the eligible slots by ascending key, one at a time
IP_HD void ni_serial_rank(const NiView& v, uint32_t p) {
  const uint32_t s0 = v.slot_off[p], s1 = v.slot_off[p + 1];
  uint32_t n = 0;
  bool have = false;
  for (uint64_t last = 0;;) {
    uint64_t best = NI_KEY_NONE;
    for (uint32_t s = s0; s < s1; ++s)
      if ((!have || v.key[s] > last) && v.key[s] < best) best = v.key[s];
    if (best == NI_KEY_NONE) break;
    last = best, have = true;
    v.order[s0 + n++] = (uint32_t)best;
  }
  v.order_n[p] = n;
}

IP_HD void ni_serial(const NiView& v) {
  for (uint32_t p = 0; p < v.n_problems; ++p) {
    ni_serial_visibility(v, p);
    for (uint32_t s = v.slot_off[p]; s < v.slot_off[p + 1]; ++s) ni_serial_slot(v, s);
    ni_serial_rank(v, p);
  }
}

// ------------------------------------------------------------------ the host's set-up of a call (host code only)
static inline void ni_default_options(dsm_next_images_options* o) {
  o->image_selection_method = DSM_NEXT_IMAGE_MIN_UNCERTAINTY;  // IncrementalMapper::Options, incremental_mapper.h:87-131
  o->abs_pose_min_num_inliers = 30;
  o->max_reg_trials = 3;
}

struct NiSetup {
  IpSetup S;
  std::vector<uint32_t> slot_off, slot_img, slot_id, slot_flags, ent_off, ent_pair, ent_slot, to_caller;
  std::vector<uint64_t> obs_off, word_off, img_wh;
  bool out_of_range = false;

  // the images, the pairs and the problems through IpSetup (the validation of dsm_find_initial_pairs)
  const char* load_graph(uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets, uint32_t num_pairs,
                                    const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches, uint32_t num_problems,
                                    const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids) {
    dsm_initial_pair_options ipo;
    ip_default_options(&ipo);
    const std::vector<uint8_t> prior(std::max<uint32_t>(num_images, 1), 0);
    const char* bad = S.load(num_images, image_ids, prior.data(), points2D_offsets, num_pairs, pair_image_ids, match_offsets, matches, num_problems,
                             problem_image_offsets, problem_image_ids, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ipo);
    out_of_range = S.out_of_range;
    return bad;
  }

  // the slots in the caller's order (IpSetup keeps a problem's slots by ascending image id) and the state of their observations;
  // num_points (or NULL) [num_problems + 1]: the CSR of the problems' points
  const char* load_state(uint32_t num_problems, const uint32_t* image_ids, const uint32_t* problem_image_ids,
                                    const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                                    const uint64_t* point_offsets) {
    if (!slot_obs_offsets) return "NULL argument";
    slot_off = S.slot_off;
    const uint32_t n_slots = slot_off[num_problems];
    if (n_slots && !slot_registered) return "NULL argument";
    slot_img.resize(n_slots), slot_id.resize(n_slots), slot_flags.resize(n_slots), to_caller.resize(n_slots);
    obs_off.assign((size_t)n_slots + 1, 0), word_off.assign((size_t)n_slots + 1, 0);
    for (uint32_t p = 0; p < num_problems; ++p) {
      const uint32_t s0 = slot_off[p], s1 = slot_off[p + 1];
      const int64_t n_points = point_offsets ? (int64_t)(point_offsets[p + 1] - point_offsets[p]) : INT64_MAX;
      for (uint32_t s = s0; s < s1; ++s) {
        const uint32_t id = problem_image_ids[s];
        auto it = std::lower_bound(S.slot_img.begin() + s0, S.slot_img.begin() + s1, id, [&](uint32_t im, uint32_t v) { return image_ids[im] < v; });
        to_caller[(uint32_t)(it - S.slot_img.begin())] = s;
        const uint32_t im = *it;
        slot_img[s] = im, slot_id[s] = id;
        if (slot_registered[s] > 1) return "slot_registered must be 0 or 1";
        slot_flags[s] = slot_registered[s] ? NI_SLOT_REGISTERED : 0u;
        if (slot_obs_offsets[s] != obs_off[s]) return "slot_obs_offsets must be the running sum of the images' point2D counts";
        obs_off[s + 1] = obs_off[s] + S.nfeat[im];
        word_off[s + 1] = word_off[s] + (S.nfeat[im] + 31) / 32;
        if (obs_off[s + 1] > obs_off[s] && !slot_obs_point3D) return "NULL argument";
        bool has_point = false;
        for (uint64_t i = obs_off[s]; i < obs_off[s + 1]; ++i) {
          if (slot_obs_point3D[i] < -1 || slot_obs_point3D[i] >= n_points) return "a point index out of range";
          has_point |= slot_obs_point3D[i] >= 0;
        }
        if (has_point && !slot_registered[s]) return "an observation with a point on an image that is not registered";
      }
    }
    if (slot_obs_offsets[n_slots] != obs_off[n_slots]) return "slot_obs_offsets must be the running sum of the images' point2D counts";
    if (obs_off[n_slots] > 0x7fffffffu) {
      out_of_range = true;
      return "more than 2^31 observations";
    }
    return nullptr;
  }

  // dsm_find_next_images: the message of the first invalid argument, or NULL
  const char* load(uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                              const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint32_t* points2D_offsets,
                              const double* points2D_xy, uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets,
                              const uint32_t* matches, uint32_t num_problems, const uint32_t* problem_image_offsets,
                              const uint32_t* problem_image_ids, const uint8_t* slot_registered, const uint64_t* slot_obs_offsets,
                              const int32_t* slot_obs_point3D, const uint32_t* slot_num_reg_trials, const uint8_t* slot_filtered,
                              const dsm_next_images_options& o) {
    if (o.image_selection_method < 0 || o.image_selection_method > 2) return "image_selection_method outside 0 .. 2";
    if (o.abs_pose_min_num_inliers <= 0) return "abs_pose_min_num_inliers must be positive";
    if (o.max_reg_trials < 1) return "max_reg_trials below 1";
    if ((num_cameras && (!camera_ids || !cameras)) || (num_images && (!image_ids || !image_camera_ids)) || !points2D_offsets || !match_offsets ||
        !problem_image_offsets)
      return "NULL argument";
    std::vector<uint32_t> cam_order;
    {
      const std::vector<uint64_t> wide(camera_ids, camera_ids + num_cameras);
      ip_sort_indices(cam_order, num_cameras, wide.data());
    }
    for (uint32_t c = 1; c < num_cameras; ++c)
      if (camera_ids[cam_order[c]] == camera_ids[cam_order[c - 1]]) return "a repeated camera id";
    img_wh.assign(2 * (size_t)num_images, 0);
    for (uint32_t i = 0; i < num_images; ++i) {
      auto it = std::lower_bound(cam_order.begin(), cam_order.end(), image_camera_ids[i], [&](uint32_t a, uint32_t v) { return camera_ids[a] < v; });
      if (it == cam_order.end() || camera_ids[*it] != image_camera_ids[i]) return "an image on an unknown camera id";
      img_wh[2 * (size_t)i] = cameras[*it].width, img_wh[2 * (size_t)i + 1] = cameras[*it].height;
    }
    if (const char* bad = load_graph(num_images, image_ids, points2D_offsets, num_pairs, pair_image_ids, match_offsets, matches, num_problems,
                                     problem_image_offsets, problem_image_ids))
      return bad;
    const uint64_t F = points2D_offsets[num_images];
    if (F && !points2D_xy) return "NULL argument";
    for (uint64_t i = 0; i < 2 * F; ++i)
      if (!std::isfinite(points2D_xy[i])) return "non-finite points2D xy";
    if (const char* bad = load_state(num_problems, image_ids, problem_image_ids, slot_registered, slot_obs_offsets, slot_obs_point3D, nullptr)) return bad;
    for (uint32_t s = 0; s < (uint32_t)slot_img.size(); ++s) {
      const uint32_t trials = slot_num_reg_trials ? slot_num_reg_trials[s] : 0, im = slot_img[s];
      if ((slot_filtered && slot_filtered[s]) || trials != 0) slot_flags[s] |= NI_SLOT_SECOND;
      if ((uint64_t)trials >= (uint64_t)o.max_reg_trials) slot_flags[s] |= NI_SLOT_EXHAUSTED;
      if (slot_registered[s]) continue;
      // a candidate: its pyramid is evaluated
      if (!img_wh[2 * (size_t)im] || !img_wh[2 * (size_t)im + 1]) return "a candidate image on a camera without width or height";
      for (uint64_t i = 2 * (uint64_t)points2D_offsets[im]; i < 2 * (uint64_t)points2D_offsets[im + 1]; ++i)
        if (points2D_xy[i] < 0) return "negative points2D xy on a candidate image";
    }
    ent_off = S.ent_off, ent_pair = S.ent_pair;
    ent_slot.resize(S.ent_slot.size());
    for (size_t i = 0; i < ent_slot.size(); ++i) ent_slot[i] = to_caller[S.ent_slot[i]];
    return nullptr;
  }
};

// ================================================================== dsm_find_local_bundles
//   IncrementalMapper::FindLocalBundle                     src/sfm/incremental_mapper.cc:932-1099
//   CalculateTriangulationAngles, Percentile               src/base/triangulation.cc:147-181, src/util/math.h:231-246
#define LB_NO_ANGLE 0xffffffffffffffffull  // a point2D without a point in an item's list of angle bits: above every angle

// Percentile's index for p = 75 over n >= 1 elements: round(75.0 / 100 * (n - 1)), std::round, clamped to 0 .. n - 1
IP_HD uint64_t lb_percentile_index(uint64_t n) {
  const double p = 75.0;
  const int idx = (int)__builtin_round(p / 100 * (double)(n - 1));
  const int last = (int)(n - 1);
  return (uint64_t)(idx < 0 ? 0 : idx > last ? last : idx);
}

// the key of an overlapping image among a query's: the shared count descending, the image id ascending
IP_HD uint64_t lb_overlap_key(uint32_t shared, uint32_t image_id) { return ((uint64_t)(~shared) << 32) | image_id; }

// does the chain of a query with n_points points2D with a point ever look at an image of this shared count: the loosest
// overlap threshold of :1001-1010
IP_HD bool lb_reachable(uint32_t shared, uint32_t n_points) { return !((double)shared < 0.1 * (double)n_points); }

struct LbChain {
  uint32_t n_out, n_filled;
  double margin;
};

// FindLocalBundle from the sorted overlap list on (:972-1098): ids, shared and tri_angle [n] in overlap order, tri_angle -1
// where none was computed (the chain then never reaches that image); `used` [n] is a work array; out has room for num_images.
IP_HD LbChain lb_select(uint32_t n, const uint32_t* ids, const uint32_t* shared, const double* tri_angle, uint32_t n_points, int32_t local_ba_num_images,
                        double min_tri_angle_deg, uint8_t* used, uint32_t* out) {
  LbChain r = {0, 0, ip_inf()};
  const uint32_t num_images = (uint32_t)(local_ba_num_images - 1), num_eff = num_images < n ? num_images : n;
  if (n == num_eff) {
    for (uint32_t i = 0; i < n; ++i) out[r.n_out++] = ids[i];
    return r;
  }
  const double rad = min_tri_angle_deg * IP_DEG_TO_RAD, np = (double)n_points;
  const double th_angle[8] = {rad / 1.0, rad / 1.5, rad / 2.0, rad / 2.5, rad / 3.0, rad / 4.0, rad / 5.0, rad / 6.0};
  const double th_shared[8] = {0.6 * np, 0.6 * np, 0.5 * np, 0.4 * np, 0.3 * np, 0.2 * np, 0.1 * np, 0.1 * np};
  for (uint32_t i = 0; i < n; ++i) used[i] = 0;
  for (int t = 0; t < 8 && r.n_out < num_eff; ++t) {
    for (uint32_t i = 0; i < n; ++i) {
      if ((double)shared[i] < th_shared[t]) break;
      if (used[i]) continue;
      ip_take(&r.margin, ip_abs(tri_angle[i] - th_angle[t]) / ip_max(th_angle[t], DBL_EPSILON));
      if (tri_angle[i] >= th_angle[t]) {
        out[r.n_out++] = ids[i];
        used[i] = 1;
        if (r.n_out >= num_eff) break;
      }
    }
  }
  if (r.n_out < num_eff)
    for (uint32_t i = 0; i < n; ++i)
      if (!used[i]) {
        out[r.n_out++] = ids[i];
        used[i] = 1;
        ++r.n_filled;
        if (r.n_out >= num_eff) break;
      }
  return r;
}

// One call's problems, points and queries as the kernels read them.  A row is one (query, image of the query's problem)
// incidence: query q's rows start at row_off[q], in the problem's slot order.
struct LbView {
  uint32_t n_problems, n_slots, n_queries;
  uint64_t n_obs, n_points;
  const uint32_t* slot_off;   // [n_problems + 1]
  const uint32_t* slot_id;    // [slots]
  const uint32_t* slot_flags; // [slots] NI_SLOT_REGISTERED
  const uint32_t* slot_prob;  // [slots]
  const uint64_t* obs_off;    // [slots + 1]
  const int32_t* obs_point;   // [observations]
  const uint64_t* point_off;  // [n_problems + 1]
  const double* point_xyz;
  const double* pose;         // [7 slots] qvec, tvec (registered slots)
  double* center;             // [3 slots]
  uint32_t* trk_start;        // [points + 1] the tracks' CSR (the histogram before the scan)
  uint32_t* trk_fill;         // [points]
  uint32_t* trk_slot;         // [observations with a point] the slot of a track element
  const uint32_t* q_slot;     // [queries]
  const uint64_t* row_off;    // [queries + 1]
  // a batch's arrays: they start at the batch's first query q0, query q's rows at row_off[q] - row_off[q0]
  uint32_t* shared;           // [rows] zero before
  uint32_t* q_points;         // [queries] NumPoints3D, zero before
  uint32_t* ov_slot;          // [rows] a query's overlapping slots in overlap order from its first row
  uint32_t* ov_n;             // [queries] zero before
};

// the sequential inversion of the observations into tracks: histogram, scan, scatter
IP_HD void lb_serial_tracks(const LbView& v) {
  for (uint64_t g = 0; g <= v.n_points; ++g) v.trk_start[g] = 0;
  for (uint32_t s = 0; s < v.n_slots; ++s)
    for (uint64_t i = v.obs_off[s]; i < v.obs_off[s + 1]; ++i)
      if (v.obs_point[i] >= 0) ++v.trk_start[v.point_off[v.slot_prob[s]] + v.obs_point[i]];
  uint32_t run = 0;
  for (uint64_t g = 0; g <= v.n_points; ++g) {
    const uint32_t c = v.trk_start[g];
    v.trk_start[g] = run;
    if (g < v.n_points) v.trk_fill[g] = 0;
    run += c;
  }
  for (uint32_t s = 0; s < v.n_slots; ++s)
    for (uint64_t i = v.obs_off[s]; i < v.obs_off[s + 1]; ++i)
      if (v.obs_point[i] >= 0) {
        const uint64_t g = v.point_off[v.slot_prob[s]] + v.obs_point[i];
        v.trk_slot[v.trk_start[g] + v.trk_fill[g]++] = s;
      }
}

// the shared counts of query q as the reference's loop counts them (:947-957), and its overlap list; shared, q_points, ov_slot
// and ov_n are a batch's arrays: they start at query q0
IP_HD void lb_serial_overlap(const LbView& v, uint32_t q, uint32_t q0) {
  const uint32_t qs = v.q_slot[q], p = v.slot_prob[qs], s0 = v.slot_off[p], n = v.slot_off[p + 1] - s0;
  const uint64_t r0 = v.row_off[q] - v.row_off[q0];
  uint32_t np = 0;
  for (uint64_t i = v.obs_off[qs]; i < v.obs_off[qs + 1]; ++i) {
    if (v.obs_point[i] < 0) continue;
    ++np;
    const uint64_t g = v.point_off[p] + v.obs_point[i];
    for (uint32_t t = v.trk_start[g]; t < v.trk_start[g + 1]; ++t)
      if (v.trk_slot[t] != qs) ++v.shared[r0 + (v.trk_slot[t] - s0)];
  }
  v.q_points[q - q0] = np;
  uint32_t m = 0;
  bool have = false;
  for (uint64_t last = 0;;) {
    uint64_t best = ~0ull;
    uint32_t pick = 0;
    for (uint32_t j = 0; j < n; ++j) {
      if (!v.shared[r0 + j]) continue;
      const uint64_t k = lb_overlap_key(v.shared[r0 + j], v.slot_id[s0 + j]);
      if ((!have || k > last) && k < best) best = k, pick = s0 + j;
    }
    if (best == ~0ull) break;
    last = best, have = true;
    v.ov_slot[r0 + m++] = pick;
  }
  v.ov_n[q - q0] = m;
}

// tri_angle of the query slot against another slot, sequentially: the angles of the query's points2D with a point in point2D
// order into `ang` (room for them), their percentile
IP_D double lb_serial_tri_angle(const LbView& v, uint32_t qs, uint32_t other, double* ang) {
  const uint32_t p = v.slot_prob[qs];
  uint64_t n = 0;
  for (uint64_t i = v.obs_off[qs]; i < v.obs_off[qs + 1]; ++i)
    if (v.obs_point[i] >= 0) ang[n++] = ip_tri_angle(v.center + 3 * (size_t)qs, v.center + 3 * (size_t)other, v.point_xyz + 3 * (v.point_off[p] + v.obs_point[i]));
  return ip_rank_serial(ang, n, lb_percentile_index(n));
}

static inline void lb_default_options(dsm_local_bundle_selection_options* o) {
  o->local_ba_num_images = 6;  // IncrementalMapper::Options, incremental_mapper.h:98-102
  o->local_ba_min_tri_angle = 6.0;
}

// the host's set-up of dsm_find_local_bundles
struct LbSetup {
  NiSetup N;
  std::vector<uint32_t> slot_prob, q_slot;
  std::vector<uint64_t> row_off;
  std::vector<double> pose;
  bool out_of_range = false;

  const char* load(uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets, uint32_t num_problems,
                              const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids, const uint8_t* slot_registered,
                              const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D, const double* slot_qvec, const double* slot_tvec,
                              const uint64_t* point_offsets, const double* point_xyz, uint32_t num_queries, const uint32_t* query_problem,
                              const uint32_t* query_image_id, const dsm_local_bundle_selection_options& o) {
    if (o.local_ba_num_images < 2) return "local_ba_num_images below 2";
    if (!(o.local_ba_min_tri_angle >= 0) || !std::isfinite(o.local_ba_min_tri_angle)) return "local_ba_min_tri_angle must be finite and not negative";
    if ((num_images && !image_ids) || !points2D_offsets || !problem_image_offsets || !point_offsets || (num_queries && (!query_problem || !query_image_id)))
      return "NULL argument";
    const uint64_t no_matches = 0;
    const char* bad = N.load_graph(num_images, image_ids, points2D_offsets, 0, nullptr, &no_matches, nullptr, num_problems, problem_image_offsets,
                                   problem_image_ids);
    if (!bad) {
      if (point_offsets[0] != 0) return "point offsets must start at 0";
      for (uint32_t p = 0; p < num_problems; ++p)
        if (point_offsets[p + 1] < point_offsets[p]) return "point offsets must be non-decreasing";
      if (point_offsets[num_problems] > 0x7fffffffu) {
        out_of_range = true;
        return "more than 2^31 points";
      }
      bad = N.load_state(num_problems, image_ids, problem_image_ids, slot_registered, slot_obs_offsets, slot_obs_point3D, point_offsets);
    }
    out_of_range = N.out_of_range;
    if (bad) return bad;
    const uint64_t P3 = point_offsets[num_problems];
    if (P3 && !point_xyz) return "NULL argument";
    for (uint64_t i = 0; i < 3 * P3; ++i)
      if (!std::isfinite(point_xyz[i])) return "a non-finite point";
    const uint32_t n_slots = (uint32_t)N.slot_img.size();
    slot_prob.resize(n_slots), pose.assign(7 * (size_t)n_slots, 0.0);
    for (uint32_t p = 0; p < num_problems; ++p)
      for (uint32_t s = N.slot_off[p]; s < N.slot_off[p + 1]; ++s) {
        slot_prob[s] = p;
        if (!slot_registered[s]) continue;
        if (!slot_qvec || !slot_tvec) return "NULL argument";
        for (int k = 0; k < 7; ++k) {
          const double x = k < 4 ? slot_qvec[4 * (size_t)s + k] : slot_tvec[3 * (size_t)s + k - 4];
          if (!std::isfinite(x)) return "a non-finite pose of a registered image";
          pose[7 * (size_t)s + k] = x;
        }
      }
    q_slot.resize(num_queries), row_off.assign((size_t)num_queries + 1, 0);
    for (uint32_t q = 0; q < num_queries; ++q) {
      const uint32_t p = query_problem[q];
      if (p >= num_problems) return "a query on an unknown problem";
      uint32_t s = N.slot_off[p];
      while (s < N.slot_off[p + 1] && N.slot_id[s] != query_image_id[q]) ++s;
      if (s == N.slot_off[p + 1]) return "a query image outside its problem";
      if (!slot_registered[s]) return "a query image that is not registered";
      q_slot[q] = s;
      row_off[q + 1] = row_off[q] + (N.slot_off[p + 1] - N.slot_off[p]);
    }
    if (row_off[num_queries] > 0x7fffffffu) {
      out_of_range = true;
      return "more than 2^31 (query, image) incidences";
    }
    return nullptr;
  }
};

#endif  // DAGSFM_AMD_CSRC_NEXT_IMAGES_H_
