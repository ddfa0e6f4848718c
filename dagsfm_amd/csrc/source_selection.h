// source_selection.h -- the exact pieces of dsm_select_source_images, written once for the kernels of
// source_selection.hip and for the host build (source_selection_host.cpp): the projection centre, the depth of a track element,
// the triangulation angle of an item, the percentile index, the depth indices, the decode of an item's triangular index, and the
// reference's loops on one lane (ss_serial_run: the cross-check schedule DSM_SOURCE_SELECTION_SERIAL and the selftest's second
// opinion).  tests/source_selection_ref.py is the normative restatement.
//
// Plain IEEE operations in a fixed order, no FMA (both builds use -ffp-contract=off).  The includer defines
//   SS_HD  qualifier of the pieces without acos   (host: `static inline`; device: `static __host__ __device__ inline`)
//   SS_D   qualifier of the pieces with acos      (host: `static inline`; device: `static __device__ inline`)
// and DSM_XT / DSM_XT_CONST for exact_acos.h.
#ifndef DAGSFM_AMD_CSRC_SOURCE_SELECTION_H_
#define DAGSFM_AMD_CSRC_SOURCE_SELECTION_H_

#include <stdint.h>

#include "../../include/dagsfm_mi355x.h"
#include "exact_acos.h"

#define SS_NAN_BITS 0x7fc00000u          // the angle of an item whose q left [-1, 1]: orders above every number as an integer
#define SS_MAX_IMAGES 65536u             // a pair key a * n_images + b and an image index next to a count fit 32 / 16 bits
#define SS_SENTINEL 0xffffffffffffffffull  // sorts behind every key

SS_HD uint32_t ss_float_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
SS_HD float ss_bits_float(uint32_t u) {
  float f;
  __builtin_memcpy(&f, &u, 4);
  return f;
}

// ComputeProjectionCenter (src/mvs/image.cc:125-130): C = -R^T T in float, every entry summed left to right, widened
SS_HD void ss_projection_center(const float* R, const float* T, double* C) {
  for (int i = 0; i < 3; ++i) {
    const float c = -((R[i] * T[0] + R[3 + i] * T[1]) + R[6 + i] * T[2]);
    C[i] = (double)c;
  }
}

// ComputeDepthRanges' depth of a track element (src/mvs/model.cc:182-184)
SS_HD float ss_depth(const float* R, const float* T, const float* X) { return ((R[6] * X[0] + R[7] * X[1]) + R[8] * X[2]) + T[2]; }

// image_depths[image_depths.size() * kPercentile] (model.cc:205-208): a FLOAT product, truncated
SS_HD uint64_t ss_depth_index(uint64_t size, float factor) {
  const uint64_t idx = (uint64_t)((float)size * factor);
  return idx < size ? idx : size - 1;  // never taken for factor < 1: (float)size * factor < size
}
SS_HD void ss_depth_range(float lo, float hi, float* out) {
  out[0] = lo * (1.0f - 0.25f);
  out[1] = hi * (1.0f + 0.25f);
}

// Percentile's index (src/util/math.h:237-239): round(p / 100 * (n - 1)) half away from zero, clamped; n >= 1, 0 <= p <= 100
SS_HD uint64_t ss_percentile_index(float percentile, uint64_t n) {
  const double x = (double)percentile / 100 * (double)(n - 1);
  double f = (double)(uint64_t)x;  // floor: x >= 0
  if (x - f >= 0.5) f += 1.0;
  const uint64_t idx = (uint64_t)f;
  return idx < n - 1 ? idx : n - 1;
}

// DegToRad (math.h:198-200) in double, narrowed as GetMaxOverlappingImages does (model.cc:123)
SS_HD float ss_min_angle_rad(double deg) { return (float)(deg * 0.0174532925199432954743716805978692718781530857086181640625); }

// item t of a track = the pair (i, j), j < i, of the reference's double loop: t = i (i - 1) / 2 + j.  The double square root is
// an estimate only; the integer steps make it exact up to the largest triangular number below 2^63.
SS_HD void ss_decode_item(uint64_t t, uint64_t* i, uint64_t* j) {
  uint64_t k = (uint64_t)__builtin_sqrt(2.0 * (double)t);
  if (k < 1) k = 1;
  if (k > 4294967295ull) k = 4294967295ull;
  while (k > 1 && (k & 1 ? k * ((k - 1) / 2) : (k / 2) * (k - 1)) > t) --k;
  while (k < 4294967295ull && ((k + 1) & 1 ? (k + 1) * (k / 2) : ((k + 1) / 2) * k) <= t) ++k;
  *i = k;
  *j = t - (k & 1 ? k * ((k - 1) / 2) : (k / 2) * (k - 1));
}
SS_HD uint64_t ss_encode_item(uint64_t i, uint64_t j) { return (i & 1 ? i * ((i - 1) / 2) : (i / 2) * (i - 1)) + j; }

// CalculateTriangulationAngle (src/base/triangulation.cc:122-145) narrowed to float (model.cc:253), as bits; SS_NAN_BITS where
// the quotient left [-1, 1] (ruling)
SS_D uint32_t ss_item_angle_bits(const double* c1, const double* c2, const float* Xf) {
  const double X[3] = {(double)Xf[0], (double)Xf[1], (double)Xf[2]};
  double d0 = c1[0] - c2[0], d1 = c1[1] - c2[1], d2 = c1[2] - c2[2];
  const double b = (d0 * d0 + d1 * d1) + d2 * d2;
  d0 = X[0] - c1[0], d1 = X[1] - c1[1], d2 = X[2] - c1[2];
  const double r1 = (d0 * d0 + d1 * d1) + d2 * d2;
  d0 = X[0] - c2[0], d1 = X[1] - c2[1], d2 = X[2] - c2[2];
  const double r2 = (d0 * d0 + d1 * d1) + d2 * d2;
  const double den = 2.0 * __builtin_sqrt(r1 * r2);
  if (den == 0.0) return 0u;
  const double q = ((r1 + r2) - b) / den;
  const double a = dsm_acos(q);  // in [0, pi]: the reference's std::abs changes nothing
  if (!(a == a)) return SS_NAN_BITS;
  const double o = 3.14159265358979323846 - a;
  return ss_float_bits((float)(o < a ? o : a));
}

// in-place heap sort of words (positive floats and the quiet NaN order as their bits do)
SS_HD void ss_sort_words(uint32_t* a, uint64_t n) {
  if (n < 2) return;
  for (uint64_t start = n / 2, end = n; end > 1;) {
    if (start > 0) {
      --start;
    } else {
      --end;
      const uint32_t t = a[end];
      a[end] = a[0];
      a[0] = t;
    }
    uint64_t root = start;
    for (;;) {
      uint64_t child = 2 * root + 1;
      if (child >= end) break;
      if (child + 1 < end && a[child] < a[child + 1]) ++child;
      if (a[root] >= a[child]) break;
      const uint32_t t = a[root];
      a[root] = a[child];
      a[child] = t;
      root = child;
    }
  }
}

struct SsModel {
  uint32_t n_images;
  uint64_t n_points;
  const float *R, *T, *xyz;
  const uint64_t* track_off;
  const uint32_t* track_img;
  const uint8_t* mask;  // or NULL
  int32_t max_num;
  float percentile, min_angle_rad;
};

// the storage of ss_serial_run
struct SsSerialWork {
  double* centers;        // [3 n]
  uint64_t* depth_off;    // [n + 1]
  uint64_t* depth_cur;    // [n]
  uint32_t* depths;       // [track elements]
  uint64_t* pair_off;     // [n n + 1]
  uint64_t* pair_cur;     // [n n]
  uint32_t* angles;       // [items]
  // results
  float* depth_ranges;        // [2 n]
  dsm_image_overlap* pairs;   // [pairs]
  uint64_t* list_off;         // [n + 1]
  uint32_t* list_img;         // [n min(max_num, n - 1)]
  uint64_t* counters;         // items, pairs, nan_items
};
#define SS_SERIAL_MAX_IMAGES 2048u

// The reference's loops, one after the other, with dense tables in place of its maps: ComputeDepthRanges, ComputeSharedPoints,
// ComputeTriangulationAngles, GetMaxOverlappingImages.  `count_only`: stop after the item and pair counts (pair_off holds the
// offsets), so that the caller can size angles and pairs.
SS_D void ss_serial_run(const SsModel& m, const SsSerialWork& w, bool count_only) {
  const uint64_t n = m.n_images;
  if (!count_only) {
    for (uint64_t a = 0; a < n; ++a) ss_projection_center(m.R + 9 * a, m.T + 3 * a, w.centers + 3 * a);
    // depths
    for (uint64_t a = 0; a <= n; ++a) w.depth_off[a] = 0;
    for (int pass = 0; pass < 2; ++pass) {
      for (uint64_t p = 0; p < m.n_points; ++p)
        for (uint64_t e = m.track_off[p]; e < m.track_off[p + 1]; ++e) {
          const uint32_t a = m.track_img[e];
          const float d = ss_depth(m.R + 9 * (uint64_t)a, m.T + 3 * (uint64_t)a, m.xyz + 3 * p);
          if (!(d > 0)) continue;
          if (pass == 0)
            w.depth_off[a + 1] += 1;
          else
            w.depths[w.depth_cur[a]++] = ss_float_bits(d);
        }
      if (pass == 0)
        for (uint64_t a = 0; a < n; ++a) {
          w.depth_off[a + 1] += w.depth_off[a];
          w.depth_cur[a] = w.depth_off[a];
        }
    }
    for (uint64_t a = 0; a < n; ++a) {
      const uint64_t size = w.depth_off[a + 1] - w.depth_off[a];
      uint32_t* d = w.depths + w.depth_off[a];
      if (!size) {
        w.depth_ranges[2 * a] = w.depth_ranges[2 * a + 1] = -1.0f;
        continue;
      }
      ss_sort_words(d, size);
      ss_depth_range(ss_bits_float(d[ss_depth_index(size, 0.01f)]), ss_bits_float(d[ss_depth_index(size, 0.99f)]), w.depth_ranges + 2 * a);
    }
  }
  // shared points and angles
  uint64_t items = 0, pairs = 0, nan_items = 0;
  for (int pass = 0; pass < (count_only ? 1 : 2); ++pass) {
    if (pass == 0)
      for (uint64_t k = 0; k <= n * n; ++k) w.pair_off[k] = 0;
    else
      for (uint64_t k = 0; k < n * n; ++k) w.pair_cur[k] = w.pair_off[k];
    for (uint64_t p = 0; p < m.n_points; ++p) {
      const uint64_t e0 = m.track_off[p], L = m.track_off[p + 1] - e0;
      for (uint64_t i = 0; i < L; ++i)
        for (uint64_t j = 0; j < i; ++j) {
          const uint32_t i1 = m.track_img[e0 + i], i2 = m.track_img[e0 + j];
          if (i1 == i2) continue;
          const uint64_t key = i1 < i2 ? i1 * n + i2 : i2 * n + i1;
          if (pass == 0) {
            w.pair_off[key + 1] += 1;
          } else {
            const uint32_t bits = ss_item_angle_bits(w.centers + 3 * (uint64_t)i1, w.centers + 3 * (uint64_t)i2, m.xyz + 3 * p);
            nan_items += bits == SS_NAN_BITS;
            w.angles[w.pair_cur[key]++] = bits;
          }
        }
    }
    if (pass == 0) {
      for (uint64_t k = 0; k < n * n; ++k) {
        pairs += w.pair_off[k + 1] != 0;
        w.pair_off[k + 1] += w.pair_off[k];
      }
      items = w.pair_off[n * n];
      w.counters[0] = items;
      w.counters[1] = pairs;
    }
  }
  if (count_only) return;
  w.counters[2] = nan_items;
  // the pair table: ascending (a, b), the count and the percentile angle
  uint64_t at = 0;
  for (uint64_t k = 0; k < n * n; ++k) {
    const uint64_t cnt = w.pair_off[k + 1] - w.pair_off[k];
    if (!cnt) continue;
    uint32_t* seg = w.angles + w.pair_off[k];
    ss_sort_words(seg, cnt);
    dsm_image_overlap o;
    o.a = (uint32_t)(k / n);
    o.b = (uint32_t)(k % n);
    o.count = (uint32_t)cnt;
    o.angle = ss_bits_float(seg[ss_percentile_index(m.percentile, cnt)]);
    w.pairs[at++] = o;
    seg[0] = ss_float_bits(o.angle);  // the pair's angle where the selection below finds it
  }
  // the lists: count descending, a tie to the lower index
  uint64_t out = 0;
  for (uint64_t a = 0; a < n; ++a) {
    w.list_off[a] = out;
    uint64_t prev_cnt = 0, prev_b = 0;
    bool have_prev = false;
    for (int64_t taken = 0; taken < (int64_t)m.max_num; ++taken) {
      uint64_t best_cnt = 0, best_b = 0;
      for (uint64_t b = 0; b < n; ++b) {
        if (b == a || (m.mask && !m.mask[b])) continue;
        const uint64_t k = a < b ? a * n + b : b * n + a;
        const uint64_t cnt = w.pair_off[k + 1] - w.pair_off[k];
        if (!cnt || !(ss_bits_float(w.angles[w.pair_off[k]]) >= m.min_angle_rad)) continue;
        if (have_prev && (cnt > prev_cnt || (cnt == prev_cnt && b <= prev_b))) continue;  // at or before the last one taken
        if (cnt > best_cnt) best_cnt = cnt, best_b = b;
      }
      if (!best_cnt) break;
      w.list_img[out++] = (uint32_t)best_b;
      prev_cnt = best_cnt, prev_b = best_b, have_prev = true;
    }
  }
  w.list_off[n] = out;
}

// what both drivers refuse, or NULL; *out_of_range tells DSM_ERR_OUT_OF_RANGE from DSM_ERR_INVALID_ARGUMENT
static inline const char* ss_validate(const dsm_source_selection_options& o, uint32_t n_images, const float* R, const float* T, uint64_t n_points,
                                      const float* xyz, const uint64_t* track_off, const uint32_t* track_img, bool* out_of_range) {
  *out_of_range = false;
  if (o.max_num_src_images < 0) return "max_num_src_images below 0";
  if (!(o.triangulation_angle_percentile >= 0.0f && o.triangulation_angle_percentile <= 100.0f)) return "triangulation_angle_percentile outside [0, 100]";
  if (!(o.min_triangulation_angle == o.min_triangulation_angle)) return "min_triangulation_angle is NaN";
  if (n_images && (!R || !T)) return "NULL R or T";
  if (n_points && (!xyz || !track_off)) return "NULL xyz or track_offsets";
  if (n_images > SS_MAX_IMAGES) {
    *out_of_range = true;
    return "more than 65536 images";
  }
  if (!n_points) return nullptr;
  if (track_off[0] != 0) return "track_offsets[0] is not 0";
  for (uint64_t p = 0; p < n_points; ++p) {
    if (track_off[p + 1] < track_off[p]) return "track_offsets decrease";
    if (track_off[p + 1] - track_off[p] > 4294967295ull) {
      *out_of_range = true;
      return "a track of 2^32 elements or more";
    }
  }
  if (track_off[n_points] && !track_img) return "NULL track_images";
  for (uint64_t e = 0; e < track_off[n_points]; ++e)
    if (track_img[e] >= n_images) return "a track names an image index out of range";
  return nullptr;
}

static inline void ss_default_options(dsm_source_selection_options* o) {
  o->max_num_src_images = 20;
  o->triangulation_angle_percentile = 75.0f;
  o->min_triangulation_angle = 1.0;
}

#endif  // DAGSFM_AMD_CSRC_SOURCE_SELECTION_H_
