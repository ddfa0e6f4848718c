// source_selection.hip -- dsm_select_source_images: the queries of mvs::Model that make PatchMatch's problems
// (src/mvs/model.cc:119-274: GetMaxOverlappingImages, ComputeDepthRanges, ComputeSharedPoints, ComputeTriangulationAngles) on
// the device.  The exact pieces are source_selection.h, shared with the host build; this file is the schedule.
//
// Every result is an order statistic or a count, so the schedule is sorts of 64-bit keys (one rocPRIM instance serves all):
//   k_ss_depths     a lane per track element: key = image << 32 | depth bits (a kept depth is positive: its bits order as the
//                   floats do), the sentinel for a depth <= 0.  After the sort k_ss_depth_ranges reads the two order
//                   statistics of every image's segment.
//   k_ss_count_items / scan   L (L - 1) / 2 items per point, 64-bit offsets.
//   k_ss_items      a lane per item: its point by binary search in the offsets, (i, j) from the triangular index, the angle;
//                   key = (a n_images + b) << 32 | angle bits with a < b, the sentinel where the two images are equal.  A long
//                   track spreads over as many lanes as it has items.
//   sort            one pair's items are contiguous and ascending in angle (NaN last).
//   k_ss_heads / scan / k_ss_pair_begin   the first item of every pair, numbered.
//   k_ss_pair_stats a lane per pair: count, percentile element; the pair's two directed edges that pass the gate and the mask as
//                   keys image << 48 | ~count << 16 | neighbour, so that one more sort orders every image's candidates by
//                   count descending, neighbour ascending.
//   k_ss_list_counts / scan / k_ss_lists  the first max_num_src_images of every image's segment.
// No float is ever added across lanes and the only atomic is an integer counter, so two calls return the same bytes.
// The check build has the reference's loops on one lane as well (DSM_SOURCE_SELECTION_SERIAL).
#include <cstdio>
#include <cstring>

#include "ctx.h"

#include <rocprim/rocprim.hpp>

#define DSM_XT static __device__ __noinline__
#define DSM_XT_CONST __device__ const
#define SS_HD static __host__ __device__ inline
#define SS_D static __device__ inline
#include "source_selection.h"

#define SS_BLOCK 256
#define SS_MAX_GRID 1048576u  // blocks of a grid-stride kernel

struct SsDev {
  SsModel m;
  uint64_t n_elems, n_items;  // track elements; pairs of track elements (equal images included)
  double* centers;            // [3 n]
  float* depth_ranges;        // [2 n]
  uint64_t* item_off;         // [n_points + 1]
  uint64_t* counters;         // 0 nan_items, 1 a pair count beyond 32 bits
  uint64_t* list_off;         // [n + 1]
};

__device__ inline uint64_t ss_global_id() { return (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ inline uint64_t ss_global_stride() { return (uint64_t)gridDim.x * blockDim.x; }

// the first index in [0, n) with a[index] > v (a ascending), or n
__device__ inline uint64_t ss_upper_bound(const uint64_t* a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] > v)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}
// the first index in [0, n) with a[index] >= v, or n
__device__ inline uint64_t ss_lower_bound(const uint64_t* a, uint64_t n, uint64_t v) {
  uint64_t lo = 0, hi = n;
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo) / 2;
    if (a[mid] >= v)
      hi = mid;
    else
      lo = mid + 1;
  }
  return lo;
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_centers(SsDev d) {
  const uint64_t a = ss_global_id();
  if (a < d.m.n_images) ss_projection_center(d.m.R + 9 * a, d.m.T + 3 * a, d.centers + 3 * a);
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_depths(SsDev d, uint64_t* keys) {
  for (uint64_t e = ss_global_id(); e < d.n_elems; e += ss_global_stride()) {
    const uint64_t p = ss_upper_bound(d.m.track_off, d.m.n_points + 1, e) - 1;  // track_off[p] <= e < track_off[p + 1]
    const uint64_t a = d.m.track_img[e];
    const float depth = ss_depth(d.m.R + 9 * a, d.m.T + 3 * a, d.m.xyz + 3 * p);
    keys[e] = depth > 0 ? (a << 32 | ss_float_bits(depth)) : SS_SENTINEL;
  }
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_depth_ranges(SsDev d, const uint64_t* keys) {
  const uint64_t a = ss_global_id();
  if (a >= d.m.n_images) return;
  const uint64_t lo = ss_lower_bound(keys, d.n_elems, a << 32), hi = ss_lower_bound(keys, d.n_elems, (a + 1) << 32);
  const uint64_t size = hi - lo;
  if (!size) {
    d.depth_ranges[2 * a] = d.depth_ranges[2 * a + 1] = -1.0f;
    return;
  }
  ss_depth_range(ss_bits_float((uint32_t)keys[lo + ss_depth_index(size, 0.01f)]), ss_bits_float((uint32_t)keys[lo + ss_depth_index(size, 0.99f)]),
                 d.depth_ranges + 2 * a);
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_count_items(SsDev d) {
  for (uint64_t p = ss_global_id(); p <= d.m.n_points; p += ss_global_stride()) {
    const uint64_t L = p < d.m.n_points ? d.m.track_off[p + 1] - d.m.track_off[p] : 0;
    d.item_off[p] = ss_encode_item(L, 0);  // L (L - 1) / 2
  }
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_items(SsDev d, uint64_t* keys) {
  uint64_t nans = 0;
  for (uint64_t t = ss_global_id(); t < d.n_items; t += ss_global_stride()) {
    const uint64_t p = ss_upper_bound(d.item_off, d.m.n_points + 1, t) - 1;
    uint64_t i, j;
    ss_decode_item(t - d.item_off[p], &i, &j);
    const uint64_t e0 = d.m.track_off[p];
    const uint64_t i1 = d.m.track_img[e0 + i], i2 = d.m.track_img[e0 + j];
    uint64_t key = SS_SENTINEL;
    if (i1 != i2) {
      const uint32_t bits = ss_item_angle_bits(d.centers + 3 * i1, d.centers + 3 * i2, d.m.xyz + 3 * p);
      nans += bits == SS_NAN_BITS;
      key = ((i1 < i2 ? i1 * d.m.n_images + i2 : i2 * d.m.n_images + i1) << 32) | bits;
    }
    keys[t] = key;
  }
  if (nans) atomicAdd((unsigned long long*)&d.counters[0], (unsigned long long)nans);
}

// flag[t] = 1 where sorted item t is the first of its pair; flag[n_items] = 0 closes the scan
__global__ void __launch_bounds__(SS_BLOCK) k_ss_heads(const uint64_t* keys, uint64_t n, uint64_t* flag) {
  for (uint64_t t = ss_global_id(); t <= n; t += ss_global_stride())
    flag[t] = (t < n && keys[t] != SS_SENTINEL && (t == 0 || (keys[t - 1] >> 32) != (keys[t] >> 32))) ? 1 : 0;
}

// rank[t]: the exclusive scan of the flags.  begin[pair] = its first item; begin[n_pairs] = the number of items with two images
__global__ void __launch_bounds__(SS_BLOCK) k_ss_pair_begin(const uint64_t* keys, uint64_t n, const uint64_t* rank, uint64_t* begin) {
  for (uint64_t t = ss_global_id(); t <= n; t += ss_global_stride()) {
    const bool valid = t < n && keys[t] != SS_SENTINEL;
    if (valid && (t == 0 || (keys[t - 1] >> 32) != (keys[t] >> 32))) begin[rank[t]] = t;
    if (!valid && (t == 0 || keys[t - 1] != SS_SENTINEL)) begin[rank[t]] = t;  // the end of the last pair
  }
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_pair_stats(SsDev d, const uint64_t* keys, const uint64_t* begin, uint64_t n_pairs, dsm_image_overlap* pairs,
                                                            uint64_t* edges) {
  for (uint64_t k = ss_global_id(); k < n_pairs; k += ss_global_stride()) {
    const uint64_t lo = begin[k], cnt = begin[k + 1] - lo;
    const uint64_t key = keys[lo + ss_percentile_index(d.m.percentile, cnt)];
    const uint64_t a = (key >> 32) / d.m.n_images, b = (key >> 32) % d.m.n_images;
    if (cnt > 4294967295ull) d.counters[1] = 1;
    dsm_image_overlap o;
    o.a = (uint32_t)a;
    o.b = (uint32_t)b;
    o.count = (uint32_t)cnt;
    o.angle = ss_bits_float((uint32_t)key);
    pairs[k] = o;
    const bool pass = o.angle >= d.m.min_angle_rad;  // false for the NaN
    const uint64_t inv = (uint64_t)(~o.count) << 16;
    edges[2 * k] = pass && (!d.m.mask || d.m.mask[b]) ? (a << 48 | inv | b) : SS_SENTINEL;
    edges[2 * k + 1] = pass && (!d.m.mask || d.m.mask[a]) ? (b << 48 | inv | a) : SS_SENTINEL;
  }
}

// counts[a] = min(candidates of a, max_num); counts[n_images] = 0 closes the scan
__global__ void __launch_bounds__(SS_BLOCK) k_ss_list_counts(SsDev d, const uint64_t* edges, uint64_t n_edges, uint64_t* counts) {
  const uint64_t a = ss_global_id();
  if (a > d.m.n_images) return;
  uint64_t c = 0;
  if (a < d.m.n_images) {
    // (a + 1) << 48 wraps to 0 for a = 65535, whose segment ends where the sentinels begin
    const uint64_t hi = a == 65535 ? ss_lower_bound(edges, n_edges, SS_SENTINEL) : ss_lower_bound(edges, n_edges, (a + 1) << 48);
    c = hi - ss_lower_bound(edges, n_edges, a << 48);
    if (c > (uint64_t)d.m.max_num) c = (uint64_t)d.m.max_num;
  }
  counts[a] = c;
}

__global__ void __launch_bounds__(SS_BLOCK) k_ss_lists(SsDev d, const uint64_t* edges, uint64_t n_edges, uint32_t* list_img) {
  const uint64_t a = ss_global_id();
  if (a >= d.m.n_images) return;
  const uint64_t lo = ss_lower_bound(edges, n_edges, a << 48), out = d.list_off[a], c = d.list_off[a + 1] - out;
  for (uint64_t k = 0; k < c; ++k) list_img[out + k] = (uint32_t)(edges[lo + k] & 0xffff);
}

#ifdef DSM_CHECK_BUILD
// DSM_SOURCE_SELECTION_SERIAL: the reference's loops on one lane
__global__ void k_ss_serial(SsModel m, SsSerialWork w, bool count_only) { ss_serial_run(m, w, count_only); }
#endif

extern "C" void dsm_default_source_selection_options(dsm_source_selection_options* o) {
  if (o) ss_default_options(o);
}

static inline size_t ss_align(size_t x) { return (x + 255) & ~(size_t)255; }
// not dsm_grid (ctx.h): the grid of a grid-stride kernel, clamped to [1, SS_MAX_GRID] in 64 bits
static inline uint32_t ss_grid(uint64_t n) {
  const uint64_t g = (n + SS_BLOCK - 1) / SS_BLOCK;
  return (uint32_t)(g < 1 ? 1 : (g > SS_MAX_GRID ? SS_MAX_GRID : g));
}

static int ss_refuse(dsm_ctx* ctx, const char* what, uint64_t need, uint64_t allowance, bool budget) {
  char msg[256];
  snprintf(msg, sizeof(msg), "dsm_select_source_images: %s need %llu bytes, %s %llu bytes", what, (unsigned long long)need,
           budget ? "the memory budget is" : "the free device memory allows", (unsigned long long)allowance);
  return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, msg);
}

extern "C" int dsm_select_source_images(dsm_ctx* ctx, const dsm_source_selection_options* options, uint32_t n_images, const float* R, const float* T,
                                        uint64_t n_points, const float* xyz, const uint64_t* track_offsets, const uint32_t* track_images,
                                        const uint8_t* candidate_mask, float* depth_ranges, uint64_t* n_list_entries, uint64_t* n_pairs_out) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  dsm_source_selection_options o;
  if (options)
    o = *options;
  else
    ss_default_options(&o);
  bool out_of_range = false;
  if (const char* bad = ss_validate(o, n_images, R, T, n_points, xyz, track_offsets, track_images, &out_of_range)) {
    ctx->err = std::string("dsm_select_source_images: ") + bad;
    return out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  }
  if (n_images && !depth_ranges) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_select_source_images: NULL depth_ranges");
  bool serial = false;
#ifdef DSM_CHECK_BUILD
  if (const char* v = ctx->dbg("DSM_SOURCE_SELECTION_SERIAL")) serial = atoi(v) != 0;
  if (serial && n_images > SS_SERIAL_MAX_IMAGES)
    return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_select_source_images: DSM_SOURCE_SELECTION_SERIAL holds dense tables: at most 2048 images");
#endif
  double ms[DSM_SOURCE_SELECTION_STAGES] = {0};
  std::vector<uint64_t> list_off((size_t)n_images + 1, 0);
  std::vector<uint32_t> list_img;
  std::vector<dsm_image_overlap> pairs;
  std::vector<float> ranges(2 * (size_t)n_images, -1.0f);
  auto finish = [&]() {
    if (n_images) memcpy(depth_ranges, ranges.data(), ranges.size() * sizeof(float));
    ctx->ss_list_off.swap(list_off);
    ctx->ss_list_img.swap(list_img);
    ctx->ss_pairs.swap(pairs);
    memcpy(ctx->source_selection_ms, ms, sizeof(ms));
    ctx->source_selection_ready = true;
    if (n_list_entries) *n_list_entries = ctx->ss_list_img.size();
    if (n_pairs_out) *n_pairs_out = ctx->ss_pairs.size();
    return DSM_OK;
  };
  const uint64_t n_elems = n_points ? track_offsets[n_points] : 0;
  if (!n_images || !n_elems) return finish();

  // ---- the plan ----
  const uint64_t n = n_images;
  uint64_t n_items = 0;
  for (uint64_t p = 0; p < n_points; ++p) {
    const uint64_t L = track_offsets[p + 1] - track_offsets[p], c = ss_encode_item(L, 0);
    if (c > (1ull << 62) || n_items + c > (1ull << 62)) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_select_source_images: 2^62 items or more");
    n_items += c;
  }
  const size_t model_bytes = ss_align(n * 9 * 4) + ss_align(n * 3 * 4) + ss_align(n_points * 12) + ss_align((n_points + 1) * 8) + ss_align(n_elems * 4) +
                             ss_align(n) + ss_align(n * 24) + ss_align(n * 8) + ss_align((n_points + 1) * 8) + ss_align(64) + 2 * ss_align((n + 1) * 8);
  // two buffers of keys, each serving in turn the depth keys, the items (+ 1 for the scan's closing entry) and the edges
  const uint64_t key_slots = (n_items > n_elems ? n_items : n_elems) + 1;
  hipStream_t st = ctx->stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  size_t tmp_sort = 0, tmp_scan = 0;
  const uint64_t scan_slots = (key_slots > n_points + 1 ? key_slots : n_points + 1) + n + 1;  // at least every scan of the call
  HIPCHK(ctx, rocprim::radix_sort_keys(nullptr, tmp_sort, (uint64_t*)nullptr, (uint64_t*)nullptr, (size_t)key_slots, 0, 64, st));
  HIPCHK(ctx, rocprim::exclusive_scan(nullptr, tmp_scan, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, (size_t)scan_slots, rocprim::plus<uint64_t>(), st));
  const size_t tmp_bytes = ss_align(tmp_sort > tmp_scan ? tmp_sort : tmp_scan) + 256;
  size_t free_b = 0, total_b = 0;
  HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
  free_b += ctx->d_ss_model.cap + ctx->d_ss_keys.cap + ctx->d_ss_tmp.cap + ctx->d_ss_pairs.cap;  // what this call may reuse
  // the pair table and the edges are sized once the pairs are counted; the items are what grows
  uint64_t need = model_bytes + 2 * ss_align(key_slots * 8) + tmp_bytes;
  if (ctx->memory_budget && need > ctx->memory_budget) return ss_refuse(ctx, "the items and tables", need, ctx->memory_budget, true);
  if (need > (uint64_t)(free_b * 0.9)) return ss_refuse(ctx, "the items and tables", need, (uint64_t)(free_b * 0.9), false);

  DevEvents<7> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  HIPCHK(ctx, ctx->d_ss_model.reserve(model_bytes));
  SsDev d;
  memset(&d, 0, sizeof(d));
  uint64_t* counts = nullptr;  // [n + 1]
  {
    char* p = ctx->d_ss_model.as<char>();
    auto take = [&p](size_t bytes) {
      char* q = p;
      p += ss_align(bytes);
      return q;
    };
    float* dR = (float*)take(n * 9 * 4);
    float* dT = (float*)take(n * 3 * 4);
    float* dX = (float*)take(n_points * 12);
    uint64_t* dOff = (uint64_t*)take((n_points + 1) * 8);
    uint32_t* dImg = (uint32_t*)take(n_elems * 4);
    uint8_t* dMask = (uint8_t*)take(n);
    d.centers = (double*)take(n * 24);
    d.depth_ranges = (float*)take(n * 8);
    d.item_off = (uint64_t*)take((n_points + 1) * 8);
    d.counters = (uint64_t*)take(64);
    d.list_off = (uint64_t*)take((n + 1) * 8);
    counts = (uint64_t*)take((n + 1) * 8);
    HIPCHK(ctx, hipMemcpyAsync(dR, R, n * 9 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dT, T, n * 3 * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dX, xyz, n_points * 12, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dOff, track_offsets, (n_points + 1) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(dImg, track_images, n_elems * 4, hipMemcpyHostToDevice, st));
    if (candidate_mask) HIPCHK(ctx, hipMemcpyAsync(dMask, candidate_mask, n, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(d.counters, 0, 64, st));
    d.m.n_images = n_images;
    d.m.n_points = n_points;
    d.m.R = dR;
    d.m.T = dT;
    d.m.xyz = dX;
    d.m.track_off = dOff;
    d.m.track_img = dImg;
    d.m.mask = candidate_mask ? dMask : nullptr;
    d.m.max_num = o.max_num_src_images;
    d.m.percentile = o.triangulation_angle_percentile;
    d.m.min_angle_rad = ss_min_angle_rad(o.min_triangulation_angle);
  }
  d.n_elems = n_elems;
  d.n_items = n_items;
  uint64_t h_counters[8] = {0};
  uint64_t items_valid = 0, n_pairs = 0, n_list = 0;

  if (serial) {
#ifdef DSM_CHECK_BUILD
    // the dense tables of the one lane live in the keys' buffer; the pair table and the angles are sized after a counting pass
    const uint64_t list_cap = n * ((uint64_t)o.max_num_src_images < n - 1 ? (uint64_t)o.max_num_src_images : n - 1);
    const size_t fixed = ss_align((n + 1) * 8) + ss_align(n * 8) + ss_align(n_elems * 4) + ss_align((n * n + 1) * 8) + ss_align(n * n * 8) + ss_align(64) +
                         ss_align(list_cap * 4 + 4);
    const size_t serial_bytes = fixed + ss_align(n_items * 4 + 4) + ss_align((n_items < n * n ? n_items : n * n) * sizeof(dsm_image_overlap) + 16);
    if (ctx->memory_budget && model_bytes + serial_bytes > ctx->memory_budget)
      return ss_refuse(ctx, "the items and tables", model_bytes + serial_bytes, ctx->memory_budget, true);
    HIPCHK(ctx, ctx->d_ss_keys.reserve(serial_bytes));
    SsSerialWork w;
    char* p = ctx->d_ss_keys.as<char>();
    auto take = [&p](size_t bytes) {
      char* q = p;
      p += ss_align(bytes);
      return q;
    };
    w.centers = d.centers;
    w.depth_ranges = d.depth_ranges;
    w.list_off = d.list_off;
    w.depth_off = (uint64_t*)take((n + 1) * 8);
    w.depth_cur = (uint64_t*)take(n * 8);
    w.depths = (uint32_t*)take(n_elems * 4);
    w.pair_off = (uint64_t*)take((n * n + 1) * 8);
    w.pair_cur = (uint64_t*)take(n * n * 8);
    w.counters = (uint64_t*)take(64);
    w.list_img = (uint32_t*)take(list_cap * 4 + 4);
    w.angles = (uint32_t*)take(n_items * 4 + 4);
    w.pairs = (dsm_image_overlap*)take((n_items < n * n ? n_items : n * n) * sizeof(dsm_image_overlap) + 16);
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    hipLaunchKernelGGL(k_ss_serial, dim3(1), dim3(1), 0, st, d.m, w, false);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[2], st));
    HIPCHK(ctx, hipMemcpyAsync(h_counters, w.counters, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(list_off.data(), w.list_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ranges.data(), d.depth_ranges, n * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    items_valid = h_counters[0];
    n_pairs = h_counters[1];
    n_list = list_off[n];
    if (n_pairs > n * n || n_list > list_cap) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_select_source_images: the serial lane's counts are out of range");
    pairs.resize(n_pairs);
    list_img.resize(n_list);
    if (n_pairs) HIPCHK(ctx, hipMemcpyAsync(pairs.data(), w.pairs, n_pairs * sizeof(dsm_image_overlap), hipMemcpyDeviceToHost, st));
    if (n_list) HIPCHK(ctx, hipMemcpyAsync(list_img.data(), w.list_img, n_list * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipEventRecord(ev[3], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, ev.ms(0, 1, &ms[0]));
    HIPCHK(ctx, ev.ms(1, 2, &ms[2]));
    HIPCHK(ctx, ev.ms(2, 3, &ms[5]));
    ms[6] = (double)items_valid;
    ms[7] = (double)n_pairs;
    ms[8] = (double)h_counters[2];
    return finish();
#endif
  }

  if (ctx->d_ss_keys.reserve(2 * ss_align(key_slots * 8)) != hipSuccess || ctx->d_ss_tmp.reserve(tmp_bytes) != hipSuccess)
    return ss_refuse(ctx, "the items and tables", need, (uint64_t)(free_b * 0.9), false);
  uint64_t* keys_a = ctx->d_ss_keys.as<uint64_t>();
  uint64_t* keys_b = (uint64_t*)(ctx->d_ss_keys.as<char>() + ss_align(key_slots * 8));
  size_t tb = 0;
  HIPCHK(ctx, hipEventRecord(ev[1], st));

  // ---- depth ranges ----
  hipLaunchKernelGGL(k_ss_centers, dim3(ss_grid(n)), dim3(SS_BLOCK), 0, st, d);
  hipLaunchKernelGGL(k_ss_depths, dim3(ss_grid(n_elems)), dim3(SS_BLOCK), 0, st, d, keys_a);
  HIPCHK(ctx, hipGetLastError());
  tb = tmp_bytes;
  HIPCHK(ctx, rocprim::radix_sort_keys(ctx->d_ss_tmp.p, tb, keys_a, keys_b, (size_t)n_elems, 0, 64, st));
  hipLaunchKernelGGL(k_ss_depth_ranges, dim3(ss_grid(n)), dim3(SS_BLOCK), 0, st, d, (const uint64_t*)keys_b);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[2], st));

  // ---- items ----
  hipLaunchKernelGGL(k_ss_count_items, dim3(ss_grid(n_points + 1)), dim3(SS_BLOCK), 0, st, d);
  HIPCHK(ctx, hipGetLastError());
  tb = tmp_bytes;
  HIPCHK(ctx, rocprim::exclusive_scan(ctx->d_ss_tmp.p, tb, d.item_off, d.item_off, (uint64_t)0, (size_t)(n_points + 1), rocprim::plus<uint64_t>(), st));
  if (n_items) {
    hipLaunchKernelGGL(k_ss_items, dim3(ss_grid(n_items)), dim3(SS_BLOCK), 0, st, d, keys_a);
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  if (n_items) {
    tb = tmp_bytes;
    HIPCHK(ctx, rocprim::radix_sort_keys(ctx->d_ss_tmp.p, tb, keys_a, keys_b, (size_t)n_items, 0, 64, st));
  }
  HIPCHK(ctx, hipEventRecord(ev[4], st));

  // ---- pairs: keys_b holds the sorted items; keys_a becomes the flags, their ranks, and then the first items of the pairs ----
  hipLaunchKernelGGL(k_ss_heads, dim3(ss_grid(n_items + 1)), dim3(SS_BLOCK), 0, st, (const uint64_t*)keys_b, n_items, keys_a);
  HIPCHK(ctx, hipGetLastError());
  tb = tmp_bytes;
  HIPCHK(ctx, rocprim::exclusive_scan(ctx->d_ss_tmp.p, tb, keys_a, keys_a, (uint64_t)0, (size_t)(n_items + 1), rocprim::plus<uint64_t>(), st));
  HIPCHK(ctx, hipMemcpyAsync(&n_pairs, keys_a + n_items, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (n_pairs > n_items || n_pairs > n * n) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_select_source_images: more pairs than items");
  // begin [n_pairs + 1], the pair table and the edges with their second buffer: sized now
  const size_t begin_bytes = ss_align((n_pairs + 1) * 8), table_bytes = ss_align(n_pairs * sizeof(dsm_image_overlap) + 16), edge_bytes = ss_align(2 * n_pairs * 8 + 16);
  const uint64_t list_cap = 2 * n_pairs < n * (uint64_t)o.max_num_src_images ? 2 * n_pairs : n * (uint64_t)o.max_num_src_images;  // entries of all lists
  const size_t pair_bytes = begin_bytes + table_bytes + 2 * edge_bytes + ss_align(list_cap * 4 + 16);
  need += pair_bytes;
  if (ctx->memory_budget && need > ctx->memory_budget) return ss_refuse(ctx, "the items, tables and pairs", need, ctx->memory_budget, true);
  DevBuf& d_pairs = ctx->d_ss_pairs;
  if (d_pairs.reserve(pair_bytes) != hipSuccess) return ss_refuse(ctx, "the items, tables and pairs", need, (uint64_t)(free_b * 0.9), false);
  uint64_t* begin = d_pairs.as<uint64_t>();
  dsm_image_overlap* d_table = (dsm_image_overlap*)(d_pairs.as<char>() + begin_bytes);
  uint64_t* edges_a = (uint64_t*)(d_pairs.as<char>() + begin_bytes + table_bytes);
  uint64_t* edges_b = (uint64_t*)(d_pairs.as<char>() + begin_bytes + table_bytes + edge_bytes);
  uint32_t* d_list = (uint32_t*)(d_pairs.as<char>() + begin_bytes + table_bytes + 2 * edge_bytes);
  hipLaunchKernelGGL(k_ss_pair_begin, dim3(ss_grid(n_items + 1)), dim3(SS_BLOCK), 0, st, (const uint64_t*)keys_b, n_items, (const uint64_t*)keys_a, begin);
  HIPCHK(ctx, hipGetLastError());
  const uint64_t n_edges = 2 * n_pairs;
  if (n_pairs) {
    hipLaunchKernelGGL(k_ss_pair_stats, dim3(ss_grid(n_pairs)), dim3(SS_BLOCK), 0, st, d, (const uint64_t*)keys_b, (const uint64_t*)begin, n_pairs, d_table, edges_a);
    HIPCHK(ctx, hipGetLastError());
    tb = tmp_bytes;  // 2 n_pairs <= key_slots whenever there are at least 4 items; the query below covers the rest
    size_t tb_edges = 0;
    HIPCHK(ctx, rocprim::radix_sort_keys(nullptr, tb_edges, edges_a, edges_b, (size_t)n_edges, 0, 64, st));
    if (tb_edges > tmp_bytes) HIPCHK(ctx, ctx->d_ss_tmp.reserve(tb_edges));
    tb = tb_edges > tmp_bytes ? tb_edges : tmp_bytes;
    HIPCHK(ctx, rocprim::radix_sort_keys(ctx->d_ss_tmp.p, tb, edges_a, edges_b, (size_t)n_edges, 0, 64, st));
  }
  hipLaunchKernelGGL(k_ss_list_counts, dim3(ss_grid(n + 1)), dim3(SS_BLOCK), 0, st, d, (const uint64_t*)edges_b, n_edges, counts);
  HIPCHK(ctx, hipGetLastError());
  tb = ctx->d_ss_tmp.cap;
  HIPCHK(ctx, rocprim::exclusive_scan(ctx->d_ss_tmp.p, tb, counts, d.list_off, (uint64_t)0, (size_t)(n + 1), rocprim::plus<uint64_t>(), st));
  hipLaunchKernelGGL(k_ss_lists, dim3(ss_grid(n)), dim3(SS_BLOCK), 0, st, d, (const uint64_t*)edges_b, n_edges, d_list);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[5], st));

  // ---- download ----
  HIPCHK(ctx, hipMemcpyAsync(list_off.data(), d.list_off, (n + 1) * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(ranges.data(), d.depth_ranges, n * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(h_counters, d.counters, 16, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(&items_valid, begin + n_pairs, 8, hipMemcpyDeviceToHost, st));
  pairs.resize(n_pairs);
  if (n_pairs) HIPCHK(ctx, hipMemcpyAsync(pairs.data(), d_table, n_pairs * sizeof(dsm_image_overlap), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  n_list = list_off[n];
  if (n_list > list_cap) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_select_source_images: more list entries than edges");
  if (h_counters[1]) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_select_source_images: a pair shares 2^32 items or more");
  list_img.resize(n_list);
  if (n_list) HIPCHK(ctx, hipMemcpyAsync(list_img.data(), d_list, n_list * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[6], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int k = 0; k < 6; ++k) {
    HIPCHK(ctx, ev.ms(k, k + 1, &ms[k]));
  }
  ms[6] = (double)items_valid;
  ms[7] = (double)n_pairs;
  ms[8] = (double)h_counters[0];
  return finish();
}

extern "C" int dsm_get_source_images(dsm_ctx* ctx, uint64_t* list_offsets, uint32_t* list_images, uint64_t capacity) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->source_selection_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_source_images: no dsm_select_source_images call yet");
  if (list_offsets) memcpy(list_offsets, ctx->ss_list_off.data(), ctx->ss_list_off.size() * sizeof(uint64_t));
  if (list_images) {
    if (capacity < ctx->ss_list_img.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_source_images: capacity below the number of indices");
    if (!ctx->ss_list_img.empty()) memcpy(list_images, ctx->ss_list_img.data(), ctx->ss_list_img.size() * sizeof(uint32_t));
  }
  return DSM_OK;
}

extern "C" int dsm_get_image_overlap(dsm_ctx* ctx, dsm_image_overlap* pairs, uint64_t capacity) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->source_selection_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_image_overlap: no dsm_select_source_images call yet");
  if (pairs) {
    if (capacity < ctx->ss_pairs.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_image_overlap: capacity below the number of pairs");
    if (!ctx->ss_pairs.empty()) memcpy(pairs, ctx->ss_pairs.data(), ctx->ss_pairs.size() * sizeof(dsm_image_overlap));
  }
  return DSM_OK;
}

extern "C" int dsm_get_source_selection_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->source_selection_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_source_selection_time: no dsm_select_source_images call yet");
  memcpy(stage_ms, ctx->source_selection_ms, sizeof(ctx->source_selection_ms));
  return DSM_OK;
}
