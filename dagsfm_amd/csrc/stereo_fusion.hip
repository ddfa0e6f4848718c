// stereo_fusion.hip -- dsm_fuse_stereo: StereoFusion::Run (src/mvs/fusion.cc:169-293) with Fuse() (:295-473) on the device
// (DESIGN.md 26).  The traversal of one seed, the medians and the reference's own seed-after-seed loop are stereo_fusion.h,
// shared with the host build; this file is the schedule.
//
// The reference's global visited masks make every seed depend on all earlier ones.  Per image (the host knows the order of
// FindNextImage up front) every unmasked pixel with a positive depth is a pending seed whose rank is its raster index, and
// the work runs in rounds:
//   1. k_sf_traverse: every pending seed traverses against the COMMITTED masks, a seed per lane; the lane's accepted pixels
//      (its list) stand for the marks it would make; a traversal stands for the next rounds until one of its pixels gets
//      masked.  A lane whose storage is too small is re-run by k_sf_big in one of the
//      slots with room for max_num_pixels pixels, lowest ranks first (k_sf_scan numbers them).
//   2. k_sf_claim: claim[pixel] = min(rank) over the lists -- an integer atomicMin, the only atomic of this file.
//   3. k_sf_decide: a seed is free when every pixel of its list is claimed by itself; the barrier is the lowest rank among
//      the seeds that are not free and whose traversal order mattered (DSM_FUSION_LIMIT).
//   4. k_sf_commit: a free seed at or below the barrier marks its pixels and computes its point; every seed takes its
//      claims back.  A seed whose own pixel got masked dies at the next traversal.  Everything else stays pending.
// The points of an image leave in rank order through a scan of the per-seed flags, whatever round committed them.
// The check build has the direct form as well (DSM_FUSION_SERIAL): one lane, seed after seed, marks made at once.
#include <chrono>
#include <cstring>

#include "ctx.h"
#include "stereo_fusion.h"

#define SF_NONE 0xffffffffu
#define SF_FREE 4u
#define SF_BLOCK 256
#define SF_SCAN_THREADS 1024
#define SF_DEFAULT_LANE_CAPACITY 32u  // at least; 16 per image a pixel can lead to (the longest overlap list + 1: a disc of radius
                                      // max_reproj_error holds 13 pixels), at most 256
#define SF_STACK_FACTOR 4u  // queue entries per list entry of a lane: a pop pushes up to a whole overlap list
#define SF_BIG_SLOTS 1024u  // at most, and at most 1 GiB of them

// ctrl words
#define SF_BARRIER 0
#define SF_PROGRESS 1
#define SF_PENDING 2
#define SF_ANY_OVERFLOW 3
#define SF_TOTAL 4  // the scan's total
#define SF_CTRL_WORDS 8

struct SfDev {
  FusionScene sc;
  uint32_t* claim;  // [total pixels]
  // per pixel of the current image, by rank
  uint8_t* state;   // 0 pending, 1 settled (no seed, committed or dead)
  uint8_t* flags;   // DSM_FUSION_LIMIT | DSM_FUSION_OVERFLOW | SF_FREE of the round
  uint8_t* lane_flags;   // ... and of the lane's last traversal, which may stand for several rounds
  uint32_t* lane_count;  // its accepted pixels
  uint32_t* count;  // accepted pixels of the round
  uint32_t* slot;   // the big slot of the round, or SF_NONE
  uint32_t* has_point;
  uint32_t* traversals;
  uint32_t* scan;
  FusionPoint* seed_point;
  uint32_t* seed_vis;  // [vis_words][n_pix]
  uint32_t *lane_list, *lane_stack_pix, *lane_stack_depth;  // [capacity][n_pix]
  uint32_t *big_list, *big_stack_pix, *big_stack_depth;     // [slot][capacity]
  uint64_t *lane_seen, *big_seen;                           // [n_images][n_pix], [slot][n_images]
  FusionPoint* out_point;  // the image's points in rank order
  uint32_t* out_vis;       // [point][vis_words]
  uint32_t* ctrl;
  uint32_t lane_cap, lane_stack_cap, big_list_cap, big_stack_cap, big_slots, vis_words;
  uint32_t image, cur_pos, pix0, n_pix;
};

__device__ inline FusionStore sf_lane_store(const SfDev& d, uint32_t s) {
  FusionStore st = {d.lane_list + s, d.lane_stack_pix + s, d.lane_stack_depth + s, d.n_pix, d.lane_cap, d.lane_stack_cap, d.lane_seen + s};
  return st;
}
__device__ inline FusionStore sf_big_store(const SfDev& d, uint32_t slot) {
  const uint64_t plane = d.big_stack_cap > d.big_list_cap + 1 ? d.big_stack_cap : d.big_list_cap + 1;
  FusionStore st = {d.big_list + (uint64_t)slot * (d.big_list_cap + 1), d.big_stack_pix + slot * plane, d.big_stack_depth + slot * plane, 1, d.big_list_cap,
                    d.big_stack_cap, d.big_seen + (uint64_t)slot * d.sc.n_images};
  return st;
}
__device__ inline FusionStore sf_store_of(const SfDev& d, uint32_t s) { return d.slot[s] == SF_NONE ? sf_lane_store(d, s) : sf_big_store(d, d.slot[s]); }

__global__ void k_sf_image_begin(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix) return;
  const uint32_t g = d.pix0 + s;
  d.state[s] = (d.sc.mask[g] || !(d.sc.depth[g] > 0.0f)) ? 1 : 0;
  d.has_point[s] = 0;
  d.traversals[s] = 0;
}

__global__ void k_sf_round_begin(SfDev d) {
  d.ctrl[SF_BARRIER] = SF_NONE;
  d.ctrl[SF_PROGRESS] = 0;
  d.ctrl[SF_PENDING] = 0;
  d.ctrl[SF_ANY_OVERFLOW] = 0;
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_traverse(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || d.state[s]) return;
  const uint32_t g = d.pix0 + s;
  if (d.sc.mask[g]) {  // a committed seed took this pixel: the reference's raster loop skips it
    d.state[s] = 1;
    d.ctrl[SF_PROGRESS] = 1;
    return;
  }
  const FusionStore st = sf_lane_store(d, s);
  // Masked and rejected pixels act alike on a traversal, so the lane's last one -- complete or cut short by its storage --
  // stands until one of ITS pixels is masked.
  bool stands = d.traversals[s] != 0;
  if (stands) {
    const uint32_t n = d.lane_count[s];
    for (uint32_t k = 0; k < n && stands; ++k) stands = !d.sc.mask[st.list[k * st.stride]];
  }
  if (!stands) {
    uint32_t fl = 0;
    d.lane_count[s] = fusion_traverse<true>(d.sc, d.cur_pos, g, st, &fl);
    d.lane_flags[s] = (uint8_t)fl;
    d.traversals[s] += 1;
  }
  d.count[s] = d.lane_count[s];
  d.flags[s] = d.lane_flags[s];
  d.slot[s] = SF_NONE;
  if (d.flags[s] & DSM_FUSION_OVERFLOW) d.ctrl[SF_ANY_OVERFLOW] = 1;
}

// exclusive scan of val[0 .. n) (FLAG: of "pending and overflowed") by one workgroup; the total goes to ctrl[SF_TOTAL]
template <bool FLAG>
__global__ void __launch_bounds__(SF_SCAN_THREADS) k_sf_scan(SfDev d, const uint32_t* val) {
  if (FLAG && !d.ctrl[SF_ANY_OVERFLOW]) return;
  __shared__ uint32_t sums[SF_SCAN_THREADS];
  const uint32_t t = threadIdx.x, chunk = (d.n_pix + SF_SCAN_THREADS - 1) / SF_SCAN_THREADS;
  const uint32_t lo = t * chunk < d.n_pix ? t * chunk : d.n_pix, hi = lo + chunk < d.n_pix ? lo + chunk : d.n_pix;
  uint32_t sum = 0;
  for (uint32_t s = lo; s < hi; ++s) sum += FLAG ? (uint32_t)(!d.state[s] && (d.flags[s] & DSM_FUSION_OVERFLOW)) : val[s];
  sums[t] = sum;
  __syncthreads();
  for (uint32_t step = 1; step < SF_SCAN_THREADS; step *= 2) {
    const uint32_t add = t >= step ? sums[t - step] : 0;
    __syncthreads();
    sums[t] += add;
    __syncthreads();
  }
  uint32_t run = sums[t] - sum;
  for (uint32_t s = lo; s < hi; ++s) {
    d.scan[s] = run;
    run += FLAG ? (uint32_t)(!d.state[s] && (d.flags[s] & DSM_FUSION_OVERFLOW)) : val[s];
  }
  if (t == SF_SCAN_THREADS - 1) d.ctrl[SF_TOTAL] = sums[t];
}

// the overflowed seeds of the lowest ranks once more, each in a slot with room for max_num_pixels pixels and every push
__global__ void __launch_bounds__(SF_BLOCK) k_sf_big(SfDev d) {
  if (!d.ctrl[SF_ANY_OVERFLOW]) return;
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || d.state[s] || !(d.flags[s] & DSM_FUSION_OVERFLOW) || d.scan[s] >= d.big_slots) return;
  uint32_t fl = 0;
  const uint32_t n = fusion_traverse<true>(d.sc, d.cur_pos, d.pix0 + s, sf_big_store(d, d.scan[s]), &fl);
  d.count[s] = n;
  d.flags[s] = (uint8_t)fl;
  d.slot[s] = d.scan[s];
  d.traversals[s] += 1;
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_claim(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || d.state[s] || (d.flags[s] & DSM_FUSION_OVERFLOW)) return;  // an overflowed seed holds the barrier: its claims decide nothing
  const FusionStore st = sf_store_of(d, s);
  const uint32_t n = d.count[s];
  for (uint32_t k = 0; k < n; ++k) atomicMin(&d.claim[st.list[k * st.stride]], s);
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_decide(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || d.state[s]) return;
  const uint32_t fl = d.flags[s];
  bool is_free = !(fl & DSM_FUSION_OVERFLOW);
  if (is_free) {
    const FusionStore st = sf_store_of(d, s);
    const uint32_t n = d.count[s];
    for (uint32_t k = 0; k < n && is_free; ++k) is_free = d.claim[st.list[k * st.stride]] == s;
  }
  if (is_free)
    d.flags[s] = (uint8_t)(fl | SF_FREE);
  else if (fl & DSM_FUSION_LIMIT)
    atomicMin(&d.ctrl[SF_BARRIER], s);
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_commit(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || d.state[s]) return;
  const uint32_t fl = d.flags[s];
  if (fl & DSM_FUSION_OVERFLOW) {
    d.ctrl[SF_PENDING] = 1;
    return;
  }
  const FusionStore st = sf_store_of(d, s);
  const uint32_t n = d.count[s];
  for (uint32_t k = 0; k < n; ++k) d.claim[st.list[k * st.stride]] = SF_NONE;  // nobody reads a claim in this kernel
  if (!(fl & SF_FREE) || s > d.ctrl[SF_BARRIER]) {
    d.ctrl[SF_PENDING] = 1;
    return;
  }
  for (uint32_t k = 0; k < n; ++k) d.sc.mask[st.list[k * st.stride]] = 1;
  d.has_point[s] = fusion_finish(d.sc, st, n, &d.seed_point[s], d.seed_vis + s, d.n_pix, d.vis_words) ? 1 : 0;
  d.state[s] = 1;
  d.ctrl[SF_PROGRESS] = 1;
}

__global__ void __launch_bounds__(SF_BLOCK) k_sf_gather(SfDev d) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= d.n_pix || !d.has_point[s]) return;
  const uint32_t at = d.scan[s];
  d.out_point[at] = d.seed_point[s];
  for (uint32_t w = 0; w < d.vis_words; ++w) d.out_vis[(uint64_t)at * d.vis_words + w] = d.seed_vis[(uint64_t)w * d.n_pix + s];
}

#ifdef DSM_CHECK_BUILD
// DSM_FUSION_SERIAL: the reference's loop on one lane
__global__ void k_sf_serial(SfDev d, uint64_t* counters) {
  uint64_t n_points = 0, n_traversals = 0;
  fusion_serial_image(d.sc, d.image, sf_big_store(d, 0), d.out_point, d.out_vis, d.vis_words, &n_points, &n_traversals);
  counters[0] = n_points;
  counters[1] = n_traversals;
}
#endif

extern "C" void dsm_default_stereo_fusion_options(dsm_stereo_fusion_options* o) {
  if (o) fusion_default_options(o);
}

static inline size_t sf_align(size_t x) { return (x + 255) & ~(size_t)255; }

extern "C" int dsm_fuse_stereo(dsm_ctx* ctx, const dsm_stereo_fusion_options* options, uint32_t n_images, const dsm_fusion_image* images,
                               const uint64_t* overlap_offsets, const uint32_t* overlap_images, uint64_t* n_points) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!n_points) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_fuse_stereo: NULL n_points");
  dsm_stereo_fusion_options o;
  if (options)
    o = *options;
  else
    fusion_default_options(&o);
  FusionHostScene hs;
  bool out_of_range = false;
  if (const char* bad = fusion_prepare(o, n_images, images, overlap_offsets, overlap_images, &hs, &out_of_range)) {
    ctx->err = std::string("dsm_fuse_stereo: ") + bad;
    return out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  }
  bool serial = false;
#ifdef DSM_CHECK_BUILD
  if (const char* v = ctx->dbg("DSM_FUSION_SERIAL")) serial = atoi(v) != 0;
#endif
  double ms[DSM_STEREO_FUSION_STAGES] = {0};
  std::vector<dsm_fused_point> points;
  std::vector<uint64_t> vis_off(1, 0);
  std::vector<uint32_t> vis_images, image_rounds(2 * (size_t)n_images, 0);  // per image: its place in the order, its rounds
  auto finish = [&]() {
    ctx->sf_points.swap(points);
    ctx->sf_vis_off.swap(vis_off);
    ctx->sf_vis_images.swap(vis_images);
    memcpy(ctx->stereo_fusion_ms, ms, sizeof(ms));
    ctx->sf_rounds.swap(image_rounds);
    ctx->stereo_fusion_ready = true;
    *n_points = ctx->sf_points.size();
    return DSM_OK;
  };
  if (!hs.total_pixels) return finish();

  // ---- the plan: what is resident for the call, and the lanes' storage under what is left ----
  const uint64_t total = hs.total_pixels, n_max = hs.max_image_pixels;
  const uint32_t vis_words = (n_images + 31) / 32;
  const uint64_t big_list_cap = (uint64_t)o.max_num_pixels < total ? (uint64_t)o.max_num_pixels : total;
  const uint64_t big_stack_cap = big_list_cap * hs.max_list + 1;
  const uint64_t big_plane = big_stack_cap > big_list_cap + 1 ? big_stack_cap : big_list_cap + 1;
  const uint64_t slot_bytes = 4 * (big_list_cap + 1) + 8 * big_plane + 8 * (uint64_t)n_images + 8;
  if (big_stack_cap >= (1ull << 31)) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_fuse_stereo: max_num_pixels x the longest overlap list is 2^31 or more");
  const size_t resident = sf_align(total * 4) + sf_align(total * 12) + sf_align(total) + sf_align(total * 4) + sf_align(hs.rgb.size() + 16) +
                          sf_align(hs.views.size() * sizeof(FusionView)) + sf_align(hs.pix0.size() * 4) + sf_align(hs.overlap_off.size() * 8) +
                          sf_align(hs.overlap.size() * 4 + 16) + sf_align(SF_CTRL_WORDS * 4 + 16);
  // per pixel of the largest image: state, the flags and counts, slot, has_point, traversals, scan, the point and its
  // visibility, and those two once more for the points in rank order
  const size_t seed_bytes = sf_align(n_max) * 3 + sf_align(n_max * 4) * 6 + sf_align(n_max * sizeof(FusionPoint)) * 2 + sf_align(n_max * 4 * vis_words) * 2 + sf_align(n_max * 8 * n_images);
  size_t free_b = 0, total_b = 0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemGetInfo(&free_b, &total_b));
  free_b += ctx->d_sf_maps.cap + ctx->d_sf_lanes.cap;  // what this call may reuse
  const uint64_t allowance = ctx->memory_budget ? ctx->memory_budget : (uint64_t)(free_b * 0.8);
  const uint64_t lane_entry_bytes = 4 + 8 * SF_STACK_FACTOR;  // a list entry and its share of the queue
  const uint64_t need_min = resident + seed_bytes + slot_bytes + (serial ? 0 : n_max * lane_entry_bytes) + 4096;
  if (need_min > allowance || need_min > free_b)
    return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_fuse_stereo: the maps of all used images do not fit the memory budget or the free device memory");
  uint64_t big_slots = serial ? 1 : SF_BIG_SLOTS;
  while (big_slots > 1 && (big_slots * slot_bytes > (1ull << 30) || need_min + (big_slots - 1) * slot_bytes > allowance)) big_slots /= 2;
  uint64_t lane_cap = (uint64_t)o.lane_capacity;
  if (!lane_cap) {
    lane_cap = 16ull * (hs.max_list + 1);
    lane_cap = lane_cap < SF_DEFAULT_LANE_CAPACITY ? SF_DEFAULT_LANE_CAPACITY : (lane_cap > 256 ? 256 : lane_cap);
  }
  if (lane_cap > big_list_cap) lane_cap = big_list_cap;  // no seed accepts more
  {
    const uint64_t left = allowance - (need_min - n_max * lane_entry_bytes) - (big_slots - 1) * slot_bytes;
    const uint64_t fit = serial ? 1 : left / (n_max * lane_entry_bytes);
    const uint64_t cap_bytes = (16ull << 30) / (n_max * lane_entry_bytes);  // beyond 16 GiB of lanes the slots are the better place
    if (lane_cap > fit) lane_cap = fit;
    if (lane_cap > cap_bytes) lane_cap = cap_bytes;
    if (lane_cap < 1) lane_cap = 1;
  }
  const uint64_t lane_stack_cap = lane_cap * SF_STACK_FACTOR;

  // ---- upload ----
  hipStream_t st = ctx->stream;
  DevEvents<5> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  HIPCHK(ctx, ctx->d_sf_maps.reserve(resident));
  size_t lanes_bytes = seed_bytes + sf_align(big_slots * slot_bytes) + 3 * 256 + 64;
  if (!serial) lanes_bytes += sf_align(n_max * 4 * lane_cap) + 2 * sf_align(n_max * 4 * lane_stack_cap);
  HIPCHK(ctx, ctx->d_sf_lanes.reserve(lanes_bytes));
  SfDev d;
  memset(&d, 0, sizeof(d));
  d.sc = hs.scene;
  {
    char* p = ctx->d_sf_maps.as<char>();
    auto take = [&p](size_t bytes) {
      char* q = p;
      p += sf_align(bytes);
      return q;
    };
    float* depth = (float*)take(total * 4);
    float* normal = (float*)take(total * 12);
    uint8_t* mask = (uint8_t*)take(total);
    d.claim = (uint32_t*)take(total * 4);
    uint8_t* rgb = (uint8_t*)take(hs.rgb.size() + 16);
    FusionView* views = (FusionView*)take(hs.views.size() * sizeof(FusionView));
    uint32_t* pix0 = (uint32_t*)take(hs.pix0.size() * 4);
    uint64_t* ooff = (uint64_t*)take(hs.overlap_off.size() * 8);
    uint32_t* ov = (uint32_t*)take(hs.overlap.size() * 4 + 16);
    d.ctrl = (uint32_t*)take(SF_CTRL_WORDS * 4 + 16);
    HIPCHK(ctx, hipMemcpyAsync(depth, hs.depth.data(), total * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(normal, hs.normal.data(), total * 12, hipMemcpyHostToDevice, st));
    if (!hs.rgb.empty()) HIPCHK(ctx, hipMemcpyAsync(rgb, hs.rgb.data(), hs.rgb.size(), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(views, hs.views.data(), hs.views.size() * sizeof(FusionView), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(pix0, hs.pix0.data(), hs.pix0.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ooff, hs.overlap_off.data(), hs.overlap_off.size() * 8, hipMemcpyHostToDevice, st));
    if (!hs.overlap.empty()) HIPCHK(ctx, hipMemcpyAsync(ov, hs.overlap.data(), hs.overlap.size() * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(mask, 0, total, st));
    HIPCHK(ctx, hipMemsetAsync(d.claim, 0xff, total * 4, st));
    HIPCHK(ctx, hipMemsetAsync(d.ctrl, 0, SF_CTRL_WORDS * 4 + 16, st));
    d.sc.views = views;
    d.sc.pix0 = pix0;
    d.sc.overlap_off = ooff;
    d.sc.overlap = ov;
    d.sc.depth = depth;
    d.sc.normal = normal;
    d.sc.rgb = rgb;
    d.sc.mask = mask;
  }
  uint64_t* counters = nullptr;  // the serial lane's
  (void)counters;
  {
    char* p = ctx->d_sf_lanes.as<char>();
    auto take = [&p](size_t bytes) {
      char* q = p;
      p += sf_align(bytes);
      return q;
    };
    d.state = (uint8_t*)take(n_max);
    d.flags = (uint8_t*)take(n_max);
    d.lane_flags = (uint8_t*)take(n_max);
    d.lane_count = (uint32_t*)take(n_max * 4);
    d.count = (uint32_t*)take(n_max * 4);
    d.slot = (uint32_t*)take(n_max * 4);
    d.has_point = (uint32_t*)take(n_max * 4);
    d.traversals = (uint32_t*)take(n_max * 4);
    d.scan = (uint32_t*)take(n_max * 4);
    d.seed_point = (FusionPoint*)take(n_max * sizeof(FusionPoint));
    d.out_point = (FusionPoint*)take(n_max * sizeof(FusionPoint));
    d.seed_vis = (uint32_t*)take(n_max * 4 * vis_words);
    d.out_vis = (uint32_t*)take(n_max * 4 * vis_words);
    counters = (uint64_t*)take(64);
    d.lane_seen = (uint64_t*)take(n_max * 8 * n_images);
    char* big = take(big_slots * slot_bytes);
    d.big_list = (uint32_t*)big;
    d.big_stack_pix = d.big_list + big_slots * (big_list_cap + 1);
    d.big_stack_depth = d.big_stack_pix + big_slots * big_plane;
    d.big_seen = (uint64_t*)(big + ((big_slots * (4 * (big_list_cap + 1) + 8 * big_plane) + 7) & ~(uint64_t)7));
    if (!serial) {
      d.lane_list = (uint32_t*)take(n_max * 4 * lane_cap);
      d.lane_stack_pix = (uint32_t*)take(n_max * 4 * lane_stack_cap);
      d.lane_stack_depth = (uint32_t*)take(n_max * 4 * lane_stack_cap);
    }
  }
  d.lane_cap = (uint32_t)lane_cap;
  d.lane_stack_cap = (uint32_t)lane_stack_cap;
  d.big_list_cap = (uint32_t)big_list_cap;
  d.big_stack_cap = (uint32_t)big_stack_cap;
  d.big_slots = (uint32_t)big_slots;
  d.vis_words = vis_words;
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  double t = 0;
  HIPCHK(ctx, ev.ms(0, 1, &ms[0]));

  // ---- the images in the reference's order ----
  std::vector<dsm_fused_point> h_points;
  std::vector<uint32_t> h_vis;
  uint64_t rounds = 0, traversals = 0;
  for (uint32_t pos = 0; pos < hs.order.size(); ++pos) {
    const uint32_t image = hs.order[pos];
    const FusionView& v = hs.views[image];
    const uint32_t n_pix = (uint32_t)v.w * (uint32_t)v.h;
    if (!n_pix) continue;
    d.image = image;
    d.cur_pos = pos;
    d.pix0 = v.pix0;
    d.n_pix = n_pix;
    const uint32_t grid = (n_pix + SF_BLOCK - 1) / SF_BLOCK;
    uint64_t n_out = 0;
    const uint64_t rounds_before = rounds;
    if (serial) {
#ifdef DSM_CHECK_BUILD
      HIPCHK(ctx, hipEventRecord(ev[0], st));
      hipLaunchKernelGGL(k_sf_serial, dim3(1), dim3(1), 0, st, d, counters);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipEventRecord(ev[1], st));
      uint64_t h_counters[2] = {0, 0};
      HIPCHK(ctx, hipMemcpyAsync(h_counters, counters, sizeof(h_counters), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      HIPCHK(ctx, ev.ms(0, 1, &t));
      ms[1] += t;
      n_out = h_counters[0];
      traversals += h_counters[1];
      rounds += 1;
#endif
    } else {
      hipLaunchKernelGGL(k_sf_image_begin, dim3(grid), dim3(SF_BLOCK), 0, st, d);
      HIPCHK(ctx, hipGetLastError());
      // the lowest pending rank commits or dies in every round, so the seeds bound the rounds
      for (uint64_t round = 0;; ++round) {
        if (round > (uint64_t)n_pix + 1) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_fuse_stereo: more rounds than seeds");
        hipLaunchKernelGGL(k_sf_round_begin, dim3(1), dim3(1), 0, st, d);
        HIPCHK(ctx, hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(k_sf_traverse, dim3(grid), dim3(SF_BLOCK), 0, st, d);
        hipLaunchKernelGGL(k_sf_scan<true>, dim3(1), dim3(SF_SCAN_THREADS), 0, st, d, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(k_sf_big, dim3(grid), dim3(SF_BLOCK), 0, st, d);
        HIPCHK(ctx, hipEventRecord(ev[1], st));
        hipLaunchKernelGGL(k_sf_claim, dim3(grid), dim3(SF_BLOCK), 0, st, d);
        hipLaunchKernelGGL(k_sf_decide, dim3(grid), dim3(SF_BLOCK), 0, st, d);
        HIPCHK(ctx, hipEventRecord(ev[2], st));
        hipLaunchKernelGGL(k_sf_commit, dim3(grid), dim3(SF_BLOCK), 0, st, d);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipEventRecord(ev[3], st));
        uint32_t h_ctrl[4] = {0, 0, 0, 0};
        HIPCHK(ctx, hipMemcpyAsync(h_ctrl, d.ctrl, sizeof(h_ctrl), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        HIPCHK(ctx, ev.ms(0, 1, &t));
        ms[1] += t;
        HIPCHK(ctx, ev.ms(1, 2, &t));
        ms[2] += t;
        HIPCHK(ctx, ev.ms(2, 3, &t));
        ms[3] += t;
        ++rounds;
        if (!h_ctrl[SF_PENDING]) break;
        if (!h_ctrl[SF_PROGRESS]) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_fuse_stereo: a round without progress");
      }
      HIPCHK(ctx, hipEventRecord(ev[0], st));
      uint32_t h_total[2] = {0, 0};
      hipLaunchKernelGGL(k_sf_scan<false>, dim3(1), dim3(SF_SCAN_THREADS), 0, st, d, (const uint32_t*)d.traversals);
      HIPCHK(ctx, hipMemcpyAsync(&h_total[1], d.ctrl + SF_TOTAL, 4, hipMemcpyDeviceToHost, st));
      hipLaunchKernelGGL(k_sf_scan<false>, dim3(1), dim3(SF_SCAN_THREADS), 0, st, d, (const uint32_t*)d.has_point);
      hipLaunchKernelGGL(k_sf_gather, dim3(grid), dim3(SF_BLOCK), 0, st, d);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(&h_total[0], d.ctrl + SF_TOTAL, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      n_out = h_total[0];
      traversals += h_total[1];
    }
    image_rounds[2 * (size_t)image] = pos;
    image_rounds[2 * (size_t)image + 1] = (uint32_t)(rounds - rounds_before);
    if (n_out > n_pix) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_fuse_stereo: more points than pixels");
    if (serial) HIPCHK(ctx, hipEventRecord(ev[0], st));
    h_points.resize(n_out);
    h_vis.resize(n_out * vis_words);
    if (n_out) {
      HIPCHK(ctx, hipMemcpyAsync(h_points.data(), d.out_point, n_out * sizeof(dsm_fused_point), hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(h_vis.data(), d.out_vis, n_out * 4 * vis_words, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(ev[4], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, ev.ms(0, 4, &t));
    ms[4] += t;
    const auto h0 = std::chrono::steady_clock::now();
    points.insert(points.end(), h_points.begin(), h_points.end());
    for (uint64_t k = 0; k < n_out; ++k) {  // ascending image index: the reference's order is its unordered_set's
      for (uint32_t i = 0; i < n_images; ++i)
        if (h_vis[k * vis_words + i / 32] >> (i % 32) & 1u) vis_images.push_back(i);
      vis_off.push_back(vis_images.size());
    }
    ms[4] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
  }
  ms[5] = (double)rounds;
  ms[6] = (double)traversals;
  return finish();
}

extern "C" int dsm_get_fused_points(dsm_ctx* ctx, dsm_fused_point* points, uint64_t capacity, uint64_t* vis_offsets, uint32_t* vis_images,
                                    uint64_t vis_capacity) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->stereo_fusion_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_fused_points: no dsm_fuse_stereo call yet");
  if (points) {
    if (capacity < ctx->sf_points.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_fused_points: capacity below the number of points");
    if (!ctx->sf_points.empty()) memcpy(points, ctx->sf_points.data(), ctx->sf_points.size() * sizeof(dsm_fused_point));
  }
  if (vis_offsets) memcpy(vis_offsets, ctx->sf_vis_off.data(), ctx->sf_vis_off.size() * sizeof(uint64_t));
  if (vis_images) {
    if (vis_capacity < ctx->sf_vis_images.size()) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_fused_points: vis_capacity below the number of indices");
    if (!ctx->sf_vis_images.empty()) memcpy(vis_images, ctx->sf_vis_images.data(), ctx->sf_vis_images.size() * sizeof(uint32_t));
  }
  return DSM_OK;
}

extern "C" int dsm_get_stereo_fusion_rounds(dsm_ctx* ctx, uint32_t* order_pos, uint32_t* rounds, uint32_t capacity) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->stereo_fusion_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_stereo_fusion_rounds: no dsm_fuse_stereo call yet");
  const size_t n = ctx->sf_rounds.size() / 2;
  if ((order_pos || rounds) && capacity < n) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_get_stereo_fusion_rounds: capacity below the number of images");
  for (size_t i = 0; i < n; ++i) {
    if (order_pos) order_pos[i] = ctx->sf_rounds[2 * i];
    if (rounds) rounds[i] = ctx->sf_rounds[2 * i + 1];
  }
  return DSM_OK;
}

extern "C" int dsm_get_stereo_fusion_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->stereo_fusion_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_stereo_fusion_time: no dsm_fuse_stereo call yet");
  memcpy(stage_ms, ctx->stereo_fusion_ms, sizeof(ctx->stereo_fusion_ms));
  return DSM_OK;
}
