// ctx.h -- the context behind the C-ABI (shared by the library's .hip files; not part of the public header).
#ifndef DAGSFM_AMD_CSRC_CTX_H_
#define DAGSFM_AMD_CSRC_CTX_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../include/dagsfm_mi355x.h"

// a device allocation, freed when its owner goes out of scope (movable, not copyable)
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) {
    o.p = nullptr;
    o.cap = 0;
  }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p;
      cap = o.cap;
      o.p = nullptr;
      o.cap = 0;
    }
    return *this;
  }
  ~DevBuf() { release(); }
  hipError_t reserve(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
      e = hipMalloc(&p, bytes);
      want = bytes;
    }
    if (e == hipSuccess) cap = want;
    return e;
  }
  // reserve keeping the old contents (first `keep` bytes)
  hipError_t grow(size_t bytes, size_t keep, hipStream_t st) {
    if (bytes <= cap) return hipSuccess;
    void* np = nullptr;
    size_t want = bytes + bytes / 2 + 256;
    hipError_t e = hipMalloc(&np, want);
    if (e != hipSuccess) {
      want = bytes;
      e = hipMalloc(&np, want);
    }
    if (e != hipSuccess) return e;
    if (p && keep) {
      e = hipMemcpyAsync(np, p, keep, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (p) (void)hipFree(p);
    p = np;
    cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// host memory into a DevBuf of at least 16 bytes; nothing is copied for bytes == 0 or a null source
inline hipError_t dev_upload(DevBuf& b, const void* src, size_t bytes, hipStream_t st) {
  hipError_t e = b.reserve(std::max<size_t>(bytes, 16));
  if (e == hipSuccess && bytes && src) e = hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st);
  return e;
}
// a DevBuf of at least 16 bytes, all of them set to `byte`
inline hipError_t dev_fill(DevBuf& b, int byte, size_t bytes, hipStream_t st) {
  hipError_t e = b.reserve(std::max<size_t>(bytes, 16));
  if (e == hipSuccess) e = hipMemsetAsync(b.p, byte, std::max<size_t>(bytes, 16), st);
  return e;
}
// blocks of `block` threads that cover n items
inline uint32_t dsm_grid(uint64_t n, int block) { return (uint32_t)((n + block - 1) / block); }

// a hipEvent_t, destroyed when its owner goes out of scope (movable, not copyable); created by hipEventCreate(&ev.e)
struct DevEvent {
  hipEvent_t e = nullptr;
  DevEvent() = default;
  DevEvent(const DevEvent&) = delete;
  DevEvent& operator=(const DevEvent&) = delete;
  DevEvent(DevEvent&& o) noexcept : e(o.e) { o.e = nullptr; }
  ~DevEvent() {
    if (e) (void)hipEventDestroy(e);
  }
  operator hipEvent_t() const { return e; }
};

// the events around a driver's stages: ev[i] is event i; ms(i, j, &out) is the time from event i to event j as a double
hipError_t dev_events_create(DevEvent* ev, size_t n);                        // capi.hip
hipError_t dev_events_ms(const DevEvent& a, const DevEvent& b, double* ms);  // capi.hip
template <int N>
struct DevEvents {
  DevEvent ev[N];
  hipError_t create() { return dev_events_create(ev, N); }
  hipError_t ms(int i, int j, double* out) const { return dev_events_ms(ev[i], ev[j], out); }
  DevEvent& operator[](int i) { return ev[i]; }
};
// the same with a size known at run time (one event per round)
struct DevEventList {
  std::vector<DevEvent> ev;
  explicit DevEventList(size_t n) : ev(n) {}
  hipError_t create() { return dev_events_create(ev.data(), ev.size()); }
  hipError_t ms(size_t i, size_t j, double* out) const { return dev_events_ms(ev[i], ev[j], out); }
  DevEvent& operator[](size_t i) { return ev[i]; }
};

// a hipStream_t, destroyed when its owner goes out of scope; created by hipStreamCreateWithFlags(&st.s, ...)
struct DevStream {
  hipStream_t s = nullptr;
  DevStream() = default;
  DevStream(const DevStream&) = delete;
  DevStream& operator=(const DevStream&) = delete;
  ~DevStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

// pinned host memory, freed when its owner goes out of scope; allocated by hipHostMalloc(&h.p, ...)
struct HostBuf {
  void* p = nullptr;
  HostBuf() = default;
  HostBuf(const HostBuf&) = delete;
  HostBuf& operator=(const HostBuf&) = delete;
  ~HostBuf() {
    if (p) (void)hipHostFree(p);
  }
  template <typename T>
  T* as() const { return reinterpret_cast<T*>(p); }
};

// One lane of dsm_verify_pairs: a share of the pair list runs through the whole E -> F -> H pipeline on the lane's own
// stream, driven by its own host thread, with its own chunk-local buffers.  The rounds of one lane are a serial chain
// of small launches and host round trips (its length is set by the slowest pair); lanes fill each other's bubbles.
struct VerifyLane {
  hipStream_t stream = nullptr;  // what the lane runs on: lane 0 borrows the context's stream, the others their own_stream
  DevStream own_stream;
  DevEvent done;
  DevBuf samples, draws_end, nmodels, vcounts, vsums, models, ework, active, vscratch;
  DevBuf lo_queue, lo_work, lo_models, lo_slots, lo_ework;  // batched local optimisation
  DevBuf tail_items, tail_n, lo_jobs, job_list;             // item passes (TailItem, LoJob)
  DevBuf hyp_map;                                           // the round's hypotheses of all pairs for the compact solver grids (verify_kernels.hip hyp_of_lane)
  uint32_t rounds[3] = {0, 0, 0}, lo_iters[3] = {0, 0, 0};
  uint32_t dbg[32] = {0};
  uint32_t dbg_norms[8] = {0};  // DSM_VERIFY_DEBUG: wave-solves that ran the exact pivot norms, E / F / H, then all wave-solves, E / F / H
  HostBuf host_ctr;  // pinned read-back target of the lane's counters
  std::string err;
  int rc = 0;

  // every DevBuf of the lane, exactly once (all of them are chunk scratch: dsm_ctx::for_each_buffer)
  template <typename F>
  void for_each_buffer(F f) {
    for (DevBuf* b : {&samples, &draws_end, &nmodels, &vcounts, &vsums, &models, &ework, &active, &vscratch, &lo_queue, &lo_work, &lo_models,
                      &lo_slots, &lo_ework, &tail_items, &tail_n, &lo_jobs, &job_list, &hyp_map})
      f(*b);
  }
};
#define DSM_VERIFY_MAX_LANES 4

struct dsm_ctx {
  int device = 0;
  DevStream stream;
  std::string err;

  // resident images
  uint32_t n_images = 0;
  uint64_t total_rows = 0;
  std::vector<uint32_t> nfeat, row0, rows;
  std::vector<dsm_camera> cameras;
  bool have_kp = false;
  DevBuf d_desc, d_rterm, d_kp, d_img_row0, d_img_rows, d_lut;
  // hand-over of pageable host buffers (capi.hip: staged_upload): two pinned host slots, their device mirror for the descriptor
  // rows on their way through k0_prepare, one event per slot; allocated by the first upload that needs them
  HostBuf h_stage;
  DevBuf d_stage;
  DevEvent stage_ev[2];

  // last dsm_match_pairs
  bool matched = false;
  uint32_t n_pairs = 0;
  std::vector<uint32_t> pairs;  // n_pairs x 2
  DevBuf d_dpairs, d_doutoff, d_pair_dir, d_m, d_counts, d_offsets, d_matches, d_total;
  uint64_t total_matches = 0;
  double k1_ms = 0.0;
  double k1b_ms = 0.0;  // k1_resolve_index
  double k1t_ms = 0.0;  // after pass 2: its k1_resolve_index + the compaction of the mutual matches (host wait for the total included)
  double k1g_ms = 0.0;  // k1_best_rows<GATHER> (pass 2 of the cross-check)
  DevBuf d_order, d_dpairs2, d_ecnt, d_eoff, d_etotal, d_entries, d_out2, d_ms, d_out2s;
  // the packed gathered pass: the chunk's runs (first pair of each + sentinel), their block counts and the scan of those, the
  // block table of the grid, and the descriptor row of every entry
  DevBuf d_runs, d_run_blocks, d_run_blkoff, d_gblocks, d_egrow;
  uint32_t k1_launches = 0;
  std::vector<DevEvent> ev;

  // last dsm_verify_pairs
  bool verified = false;
  DevBuf d_cams, d_pairs_dev, d_seeds, d_tvg, d_inl, d_inl_counts, d_inl_off, d_inl_compact, d_vscratch, d_inl_total;
  DevBuf d_nt_table, d_nt_off, d_nt_off_t, d_pair_state, d_pts_px, d_pts_norm, d_pts_f32, d_reports, d_masks;
  DevBuf d_fam_state, d_sidx, d_lo_inl;
  DevBuf d_nt_table_t, d_wm_redo, d_wm_total, d_wm_count, d_lo_inl_pool, d_pose_jobs;
  VerifyLane lanes[DSM_VERIFY_MAX_LANES];
  uint32_t verify_lanes = 1;  // lanes of the last call
  uint32_t verify_lo_iters[3] = {0, 0, 0};
  DevBuf d_g_nfeat, d_g_dpairs, d_g_doff, d_g_pdir, d_g_params, d_g_m, d_g_counts, d_g_offsets, d_g_total, d_g_matches,
      d_g_plan, d_g_inl, d_g_inl_off;  // guided matching
  DevBuf d_mm_matches[2], d_mm_off[2], d_mm_counts, d_mm_state, d_mm_first, d_mm_acc, d_mm_keep, d_mm_total;  // EstimateMultiple
  uint32_t verify_rounds[3] = {0, 0, 0};
  uint64_t total_inliers = 0;
  double verify_ms = 0.0;
  // cache of the tabulated RANSAC::ComputeNumTrials (host libm), keyed by confidence
  double nt_confidence = -1.0;
  std::vector<uint32_t> nt_table;        // E / F / H tables of the match counts seen so far, back to back
  std::vector<uint64_t> nt_off;          // per N (0 = absent; offsets are stored +1)
  std::vector<uint32_t> nt_table_t;      // translation tables of the inlier counts that needed one (built on demand)
  std::vector<uint64_t> nt_off_t;        // per N (0 = absent; offsets are stored +1)
  bool nt_dirty = true, nt_dirty_t = true;
  DevEvent vev0, vev1;

  dsm_ctx* leaf = nullptr;  // private context of the one-shot leaf entry points

  // dsm_set_debug_option: switches of THIS context (none changes a result).  The library never reads the process
  // environment: a host application's environment cannot change schedules.
  // Two builds of the same sources (Makefile):
  //   libdagsfm_mi355x.so        the product: only the scheduling knobs a deployer could want (dsm_product_debug_keys);
  //                              the cross-check schedules are not compiled in
  //   libdagsfm_mi355x_check.so  -DDSM_CHECK_BUILD: additionally the independent schedules of the same results that
  //                              tools/check_schedules.py and the schedule-parametrised tests compare the product with
  //                              (legacy one-kernel LO-RANSAC, fused / LDS forms of the 5-point root finder,
  //                              the v_dot4 K1 and word assignment, the two-kernel K1 + k1_resolve_index,
  //                              the minimal solvers' exact pivot-norm bookkeeping in every wave (DSM_NORMS_EXACT),
  //                              counters of DSM_VERIFY_DEBUG / DSM_SCORE_PREFILTER=check)
  std::map<std::string, std::string> debug_options;
  const char* dbg(const char* key) const {
    const auto it = debug_options.find(key);
    return it == debug_options.end() ? nullptr : it->second.c_str();
  }

  // dsm_ctx_set_memory_budget: bytes the chunk planners of dsm_match_pairs / dsm_verify_pairs may spend on their transient
  // scratch (0: the default policy -- 8 GiB of K1 output per chunk, 40 % of the free memory, 4 .. 96 GiB, for the verifier)
  uint64_t memory_budget = 0;

  struct RetrievalState* retrieval = nullptr;  // vocabulary-tree retrieval (retrieval.hip), created on first use
  struct CovSiftState* covsift = nullptr;      // the scale space and the last result of dsm_extract_covariant_sift (covariant_sift.hip), created on first use
  struct SiftState* sift = nullptr;            // the scratch of dsm_extract_sift (sift_extraction.hip), created on first use, reused across calls

  // undistortion.hip: the border pixels of dsm_undistort_cameras, the points of dsm_undistort_points2D, a chunk of source and
  // target images of dsm_warp_images and its map of source points; the HIP-event times of the last call of each
  DevBuf d_ud_border, d_ud_points, d_ud_src, d_ud_dst, d_ud_map;
  bool undistortion_ready = false;
  double undistortion_ms[DSM_UNDISTORTION_STAGES] = {0};

  // patch_match.hip: the image table, the tables and every map of one chunk of problems of dsm_patch_match; the HIP-event
  // times of the last call
  DevBuf d_pm;
  bool patch_match_ready = false;
  double patch_match_ms[DSM_PATCH_MATCH_STAGES] = {0};

  // stereo_fusion.hip: the maps, masks and claims of all used images of dsm_fuse_stereo with the bitmaps and the tables
  // (d_sf_maps), the per-seed state, the lanes' lists and queues and the big slots (d_sf_lanes); the fused points of the last
  // call with their visibility lists (dsm_get_fused_points) and its times
  DevBuf d_sf_maps, d_sf_lanes;
  std::vector<dsm_fused_point> sf_points;
  std::vector<uint64_t> sf_vis_off;
  std::vector<uint32_t> sf_vis_images, sf_rounds;
  bool stereo_fusion_ready = false;
  double stereo_fusion_ms[DSM_STEREO_FUSION_STAGES] = {0};

  // source_selection.hip: the model and the tables (d_ss_model), the keys of the items and their second buffer, reused for
  // the depth keys (d_ss_keys), rocPRIM's temporary storage (d_ss_tmp), the first items of the pairs, the pair table, the edges
  // and the lists on the device (d_ss_pairs); the lists, the pair table and the times of the last dsm_select_source_images
  DevBuf d_ss_model, d_ss_keys, d_ss_tmp, d_ss_pairs;
  std::vector<uint64_t> ss_list_off;
  std::vector<uint32_t> ss_list_img;
  std::vector<dsm_image_overlap> ss_pairs;
  bool source_selection_ready = false;
  double source_selection_ms[DSM_SOURCE_SELECTION_STAGES] = {0};

  // vocabulary_build.hip: the descriptors, the indices permutation, the per-position values and the per-job state of a
  // dsm_retrieval_quantize call, the buffers of dsm_retrieval_train_embedding -- all released when the call ends; the tree of the
  // last dsm_retrieval_quantize in depth-first order (dsm_get_vocabulary_tree) and the HIP-event times of the last calls
  DevBuf d_vb_desc, d_vb_idx, d_vb_point, d_vb_node, d_vb_embed;
  std::vector<dsm_vocabulary_tree_node> vb_nodes;
  std::vector<float> vb_pivots;
  std::vector<std::vector<int32_t>> vb_childs;
  std::vector<int32_t> vb_indices;
  int32_t vb_branching = 0;
  bool vocabulary_build_ready = false;
  double vocabulary_build_ms[DSM_VOCABULARY_BUILD_STAGES] = {0};

  // the final Ritz values and the k Ritz vectors ([images][k]) of the last dsm_view_graph_cluster that ran the eigen-solver
  // (view_graph_clustering.hip)
  std::vector<double> cluster_ritz, cluster_vectors;
  uint32_t cluster_rows = 0, cluster_cols = 0;

  // Every DevBuf of the context and of its lanes, exactly once, with its class: f(buf, scratch).  Scratch is the transient
  // chunk memory dsm_ctx_set_memory_budget governs; resident is the images and the last calls' inputs / results / per-pair
  // state (include/dagsfm_mi355x.h, dsm_ctx_memory_footprint).  tests/test_ctx_buffers.py holds this list to the declarations.
  template <typename F>
  void for_each_buffer(F f) {
    for (DevBuf* b : {&d_desc, &d_rterm, &d_kp, &d_img_row0, &d_img_rows, &d_lut, &d_stage, &d_counts, &d_offsets, &d_matches, &d_total, &d_etotal,
                      &d_cams, &d_pairs_dev, &d_seeds, &d_tvg, &d_inl, &d_inl_counts, &d_inl_off, &d_inl_compact, &d_inl_total, &d_nt_table,
                      &d_nt_off, &d_nt_off_t, &d_pair_state, &d_pts_px, &d_pts_norm, &d_pts_f32, &d_reports, &d_masks, &d_fam_state, &d_sidx, &d_lo_inl,
                      &d_nt_table_t, &d_wm_redo, &d_wm_total, &d_wm_count, &d_lo_inl_pool, &d_pose_jobs,
                      &d_g_nfeat, &d_g_dpairs, &d_g_doff, &d_g_pdir, &d_g_params, &d_g_m, &d_g_counts, &d_g_offsets, &d_g_total, &d_g_matches,
                      &d_g_plan, &d_g_inl, &d_g_inl_off,
                      &d_mm_matches[0], &d_mm_matches[1], &d_mm_off[0], &d_mm_off[1], &d_mm_counts, &d_mm_state, &d_mm_first, &d_mm_acc,
                      &d_mm_keep, &d_mm_total, &d_vb_desc, &d_vb_idx})
      f(*b, false);
    for (DevBuf* b : {&d_m, &d_ms, &d_entries, &d_out2, &d_out2s, &d_dpairs, &d_dpairs2, &d_doutoff, &d_pair_dir, &d_order, &d_ecnt, &d_eoff,
                      &d_runs, &d_run_blocks, &d_run_blkoff, &d_gblocks, &d_egrow,
                      &d_vscratch, &d_ud_border, &d_ud_points, &d_ud_src, &d_ud_dst, &d_ud_map, &d_pm, &d_vb_point, &d_vb_node, &d_vb_embed, &d_sf_maps, &d_sf_lanes,
                      &d_ss_model, &d_ss_keys, &d_ss_tmp, &d_ss_pairs})
      f(*b, true);
    for (VerifyLane& L : lanes) L.for_each_buffer([&f](DevBuf& b) { f(b, true); });
  }
};
void dsm_retrieval_destroy(dsm_ctx* ctx);     // retrieval.hip
void dsm_retrieval_invalidate(dsm_ctx* ctx);  // retrieval.hip: the resident images changed
void dsm_sift_destroy(dsm_ctx* ctx);          // sift_extraction.hip
void dsm_covariant_sift_destroy(dsm_ctx* ctx);  // covariant_sift.hip
// capi.hip: verify_core_plain on the leaf context (device arrays but `counts`); the results stay on the leaf until its next use
int dsm_verify_on_leaf(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* d_pairs, const uint64_t* d_match_off, const uint32_t* d_matches,
                       uint64_t total_matches, const std::vector<uint32_t>& counts, const double* d_kp, const uint32_t* d_img_row0,
                       const dsm_camera* d_cams, const dsm_two_view_options* o, const uint32_t* d_seeds, const dsm_two_view_geometry** d_tvg,
                       const uint64_t** d_inl_off, const uint32_t** d_inl, uint64_t* total_inliers, double* kernel_ms);

// keys dsm_set_debug_option accepts (an unknown key is an error, so a check-only switch fails loudly on the product build)
static const char* const dsm_product_debug_keys[] = {"DSM_MATCH_CHUNK_ROWS", "DSM_VERIFY_CHUNK_PAIRS", "DSM_VERIFY_LANES", "DSM_VERIFY_INLINE_LO",
                                                     "DSM_VERIFY_ITEM_MODE", "DSM_LO_TAIL", "DSM_LO_TAIL_MODE", "DSM_VERIFY_GRID_DIV"};
#ifdef DSM_CHECK_BUILD
static const char* const dsm_check_debug_keys[] = {"DSM_K1_DOT4", "DSM_K1_RESOLVE_KERNEL", "DSM_VERIFY_DEBUG", "DSM_SAMPLER_SERIAL", "DSM_LO_PREPARE_WAVE", "DSM_LO_JACOBI_GROUPS",
                                                   "DSM_ROOTS_LDS", "DSM_FINAL_WAVES", "DSM_VERIFY_LEGACY", "DSM_VERIFY_FIXED_BATCH", "DSM_VERIFY_LANE_SPLIT",
                                                   "DSM_DEBUG_SAMPLER_MODE", "DSM_VOCAB_ASSIGN_VALU", "DSM_VERIFY_HOST_LOOP", "DSM_SCORE_PREFILTER",
                                                   "DSM_VERIFY_REPLAY_GRID", "DSM_REPLAY_LEGACY", "DSM_FLANN_GROUP", "DSM_FLANN_STATS", "DSM_ELU_LDS", "DSM_HYP_GRID", "DSM_SPEC_MARGIN",
                                                   "DSM_POSE_FULL", "DSM_PATCH_MATCH_LANES", "DSM_NORMS_EXACT", "DSM_FUSION_SERIAL",
                                                   "DSM_SOURCE_SELECTION_SERIAL", "DSM_INITIAL_PAIR_SERIAL", "DSM_NEXT_IMAGES_SERIAL", "DSM_TRACK_UPDATE_SERIAL",
                                                   "DSM_COMPLETE_IMAGE_SERIAL"};
#endif

// ---- the failure paths, out of line (capi.hip): a site costs a compare and a call, no string is built inline
// "<file>:<line>: <hipGetErrorString>", the message of every failed HIP runtime call
std::string dsm_hip_message(hipError_t e, const char* file, int line);
// ctx->err = dsm_hip_message(...); returns DSM_ERR_HIP
int dsm_hip_fail(dsm_ctx* ctx, hipError_t e, const char* file, int line);
// ctx->err = "<entry>: <msg>"; returns code / DSM_ERR_INVALID_ARGUMENT
int dsm_fail(dsm_ctx* ctx, int code, const char* entry, const char* msg);
int dsm_invalid(dsm_ctx* ctx, const char* entry, const char* msg);
int dsm_invalid(dsm_ctx* ctx, const char* entry, const std::string& msg);

#define HIPCHK(ctx, call)                                                                  \
  do {                                                                                     \
    const hipError_t e_ = (call);                                                          \
    if (e_ != hipSuccess) return dsm_hip_fail((ctx), e_, __FILE_NAME__, __LINE__);         \
  } while (0)

// the sticky form for a driver with a single exit: the first failing call is recorded in ctx->err and in the local int rc,
// later calls still run (and later failures are not recorded)
#define HIPTRY(call)                                                                               \
  do {                                                                                             \
    const hipError_t e_ = (call);                                                                  \
    if (e_ != hipSuccess && rc == DSM_OK) rc = dsm_hip_fail(ctx, e_, __FILE_NAME__, __LINE__);     \
  } while (0)

static inline int dsm_fail(dsm_ctx* ctx, int code, const char* msg) {
  if (ctx) ctx->err = msg;
  return code;
}

#endif  // DAGSFM_AMD_CSRC_CTX_H_
