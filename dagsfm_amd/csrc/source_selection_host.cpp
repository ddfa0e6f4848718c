// source_selection_host.cpp -- the host build of source_selection.h: the queries of mvs::Model on one CPU thread
// from the text the kernels are built from.  What the CPU test holds to tests/source_selection_ref.py bit for bit, the
// single-threaded baseline of tools/bench_source_selection.py, and what `make selection-selftest` runs under the sanitizers.
// Two drivers: the device's schedule with std::sort in place of the radix sorts (dsm_ss_host_run), and the reference's loops
// over dense tables (dsm_ss_host_run_serial, the text of DSM_SOURCE_SELECTION_SERIAL).  No HIP.
#include <algorithm>
#include <cstring>
#include <vector>

#define DSM_XT static inline
#define DSM_XT_CONST static const
#define SS_HD static inline
#define SS_D static inline
#include "source_selection.h"

static std::vector<uint64_t> g_list_off(1, 0);
static std::vector<uint32_t> g_list_img;
static std::vector<dsm_image_overlap> g_pairs;

extern "C" double dsm_ss_host_acos(double q) { return dsm_acos(q); }
extern "C" void dsm_ss_host_default_options(dsm_source_selection_options* o) { ss_default_options(o); }
extern "C" void dsm_ss_host_decode_item(uint64_t t, uint64_t* i, uint64_t* j) { ss_decode_item(t, i, j); }
extern "C" uint64_t dsm_ss_host_encode_item(uint64_t i, uint64_t j) { return ss_encode_item(i, j); }
extern "C" uint64_t dsm_ss_host_depth_index(uint64_t size, float factor) { return ss_depth_index(size, factor); }
extern "C" uint64_t dsm_ss_host_percentile_index(float percentile, uint64_t n) { return ss_percentile_index(percentile, n); }
extern "C" float dsm_ss_host_min_angle_rad(double deg) { return ss_min_angle_rad(deg); }
// the float angle of one item: the centres are float (widened here, as ComputeTriangulationAngles does), the point float
extern "C" uint32_t dsm_ss_host_angle_bits(const float* c1, const float* c2, const float* X) {
  const double a[3] = {c1[0], c1[1], c1[2]}, b[3] = {c2[0], c2[1], c2[2]};
  return ss_item_angle_bits(a, b, X);
}
extern "C" void dsm_ss_host_projection_center(const float* R, const float* T, double* C) { ss_projection_center(R, T, C); }

static int ss_host_begin(const dsm_source_selection_options* options, uint32_t n_images, const float* R, const float* T, uint64_t n_points, const float* xyz,
                         const uint64_t* track_off, const uint32_t* track_img, const uint8_t* mask, float* depth_ranges, const char** why, SsModel* m) {
  dsm_source_selection_options o;
  if (options)
    o = *options;
  else
    ss_default_options(&o);
  bool out_of_range = false;
  const char* bad = ss_validate(o, n_images, R, T, n_points, xyz, track_off, track_img, &out_of_range);
  if (!bad && n_images && !depth_ranges) bad = "NULL depth_ranges";
  if (why) *why = bad;
  if (bad) return out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  *m = SsModel{n_images, n_points, R, T, xyz, track_off, track_img, mask, o.max_num_src_images, o.triangulation_angle_percentile,
               ss_min_angle_rad(o.min_triangulation_angle)};
  return DSM_OK;
}

// counters: items, pairs, nan_items.  0, or DSM_ERR_INVALID_ARGUMENT / DSM_ERR_OUT_OF_RANGE with *why; the lists and the pair
// table stay for dsm_ss_host_get
extern "C" int dsm_ss_host_run(const dsm_source_selection_options* options, uint32_t n_images, const float* R, const float* T, uint64_t n_points,
                               const float* xyz, const uint64_t* track_off, const uint32_t* track_img, const uint8_t* mask, float* depth_ranges,
                               uint64_t* n_list_entries, uint64_t* n_pairs, uint64_t* counters, const char** why) {
  SsModel m;
  if (const int rc = ss_host_begin(options, n_images, R, T, n_points, xyz, track_off, track_img, mask, depth_ranges, why, &m)) return rc;
  const uint64_t n = n_images;
  std::vector<double> centers(3 * n);
  for (uint64_t a = 0; a < n; ++a) ss_projection_center(R + 9 * a, T + 3 * a, &centers[3 * a]);
  // depths: key = image << 32 | depth bits
  std::vector<uint64_t> keys;
  for (uint64_t p = 0; p < n_points; ++p)
    for (uint64_t e = track_off[p]; e < track_off[p + 1]; ++e) {
      const uint64_t a = track_img[e];
      const float depth = ss_depth(R + 9 * a, T + 3 * a, xyz + 3 * p);
      if (depth > 0) keys.push_back(a << 32 | ss_float_bits(depth));
    }
  std::sort(keys.begin(), keys.end());
  for (uint64_t a = 0; a < n; ++a) {
    const uint64_t lo = std::lower_bound(keys.begin(), keys.end(), a << 32) - keys.begin();
    const uint64_t size = (std::lower_bound(keys.begin(), keys.end(), (a + 1) << 32) - keys.begin()) - lo;
    if (!size) {
      depth_ranges[2 * a] = depth_ranges[2 * a + 1] = -1.0f;
      continue;
    }
    ss_depth_range(ss_bits_float((uint32_t)keys[lo + ss_depth_index(size, 0.01f)]), ss_bits_float((uint32_t)keys[lo + ss_depth_index(size, 0.99f)]),
                   depth_ranges + 2 * a);
  }
  // items: key = (a n + b) << 32 | angle bits, a < b
  keys.clear();
  uint64_t nan_items = 0;
  for (uint64_t p = 0; p < n_points; ++p) {
    const uint64_t e0 = track_off[p], L = track_off[p + 1] - e0;
    for (uint64_t i = 0; i < L; ++i)
      for (uint64_t j = 0; j < i; ++j) {
        const uint64_t i1 = track_img[e0 + i], i2 = track_img[e0 + j];
        if (i1 == i2) continue;
        const uint32_t bits = ss_item_angle_bits(&centers[3 * i1], &centers[3 * i2], xyz + 3 * p);
        nan_items += bits == SS_NAN_BITS;
        keys.push_back(((i1 < i2 ? i1 * n + i2 : i2 * n + i1) << 32) | bits);
      }
  }
  std::sort(keys.begin(), keys.end());
  g_pairs.clear();
  std::vector<uint64_t> edges;
  for (uint64_t lo = 0; lo < keys.size();) {
    uint64_t hi = lo + 1;
    while (hi < keys.size() && (keys[hi] >> 32) == (keys[lo] >> 32)) ++hi;
    const uint64_t cnt = hi - lo, key = keys[lo + ss_percentile_index(m.percentile, cnt)];
    if (cnt > 4294967295ull) {
      if (why) *why = "a pair shares 2^32 items or more";
      return DSM_ERR_OUT_OF_RANGE;
    }
    dsm_image_overlap o;
    o.a = (uint32_t)((key >> 32) / n);
    o.b = (uint32_t)((key >> 32) % n);
    o.count = (uint32_t)cnt;
    o.angle = ss_bits_float((uint32_t)key);
    g_pairs.push_back(o);
    if (o.angle >= m.min_angle_rad) {
      const uint64_t inv = (uint64_t)(~o.count) << 16;
      if (!mask || mask[o.b]) edges.push_back((uint64_t)o.a << 48 | inv | o.b);
      if (!mask || mask[o.a]) edges.push_back((uint64_t)o.b << 48 | inv | o.a);
    }
    lo = hi;
  }
  std::sort(edges.begin(), edges.end());
  g_list_off.assign(n + 1, 0);
  g_list_img.clear();
  uint64_t at = 0;
  for (uint64_t a = 0; a < n; ++a) {
    g_list_off[a] = g_list_img.size();
    for (uint64_t taken = 0; at < edges.size() && (edges[at] >> 48) == a; ++at, ++taken)
      if (taken < (uint64_t)m.max_num) g_list_img.push_back((uint32_t)(edges[at] & 0xffff));
  }
  g_list_off[n] = g_list_img.size();
  if (n_list_entries) *n_list_entries = g_list_img.size();
  if (n_pairs) *n_pairs = g_pairs.size();
  if (counters) counters[0] = keys.size(), counters[1] = g_pairs.size(), counters[2] = nan_items;
  return DSM_OK;
}

// the same results by the reference's loops over dense tables (at most SS_SERIAL_MAX_IMAGES images)
extern "C" int dsm_ss_host_run_serial(const dsm_source_selection_options* options, uint32_t n_images, const float* R, const float* T, uint64_t n_points,
                                      const float* xyz, const uint64_t* track_off, const uint32_t* track_img, const uint8_t* mask, float* depth_ranges,
                                      uint64_t* n_list_entries, uint64_t* n_pairs, uint64_t* counters, const char** why) {
  SsModel m;
  if (const int rc = ss_host_begin(options, n_images, R, T, n_points, xyz, track_off, track_img, mask, depth_ranges, why, &m)) return rc;
  if (n_images > SS_SERIAL_MAX_IMAGES) {
    if (why) *why = "the serial form holds dense tables: at most 2048 images";
    return DSM_ERR_OUT_OF_RANGE;
  }
  const uint64_t n = n_images, n_elems = n_points ? track_off[n_points] : 0;
  std::vector<double> centers(3 * n + 1);
  std::vector<uint64_t> depth_off(n + 1), depth_cur(n + 1), pair_off(n * n + 1), pair_cur(n * n + 1), c(3, 0);
  std::vector<uint32_t> depths(n_elems + 1);
  std::vector<float> ranges(2 * n + 1);
  SsSerialWork w = {centers.data(), depth_off.data(), depth_cur.data(), depths.data(), pair_off.data(), pair_cur.data(), nullptr, ranges.data(), nullptr,
                    nullptr,        nullptr,          c.data()};
  ss_serial_run(m, w, true);
  std::vector<uint32_t> angles(c[0] + 1);
  const uint64_t per_image = n ? std::min<uint64_t>((uint64_t)m.max_num, n - 1) : 0;
  g_pairs.assign(c[1] + 1, dsm_image_overlap());
  g_list_off.assign(n + 1, 0);
  g_list_img.assign(n * per_image + 1, 0);
  w.angles = angles.data();
  w.pairs = g_pairs.data();
  w.list_off = g_list_off.data();
  w.list_img = g_list_img.data();
  ss_serial_run(m, w, false);
  g_pairs.resize(c[1]);
  g_list_img.resize(g_list_off[n]);
  if (n) memcpy(depth_ranges, ranges.data(), 2 * n * sizeof(float));
  if (n_list_entries) *n_list_entries = g_list_img.size();
  if (n_pairs) *n_pairs = g_pairs.size();
  if (counters) memcpy(counters, c.data(), 24);
  return DSM_OK;
}

// the lists (n_images + 1 offsets, the indices) and the pair table of the last run; any pointer may be NULL
extern "C" void dsm_ss_host_get(uint64_t* list_off, uint32_t* list_img, dsm_image_overlap* pairs) {
  if (list_off) memcpy(list_off, g_list_off.data(), g_list_off.size() * sizeof(uint64_t));
  if (list_img && !g_list_img.empty()) memcpy(list_img, g_list_img.data(), g_list_img.size() * sizeof(uint32_t));
  if (pairs && !g_pairs.empty()) memcpy(pairs, g_pairs.data(), g_pairs.size() * sizeof(dsm_image_overlap));
}
