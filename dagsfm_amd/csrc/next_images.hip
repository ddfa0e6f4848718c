// next_images.hip -- the next images and the local bundles of a batch of reconstructions on the device.
//   IncrementalMapper::FindNextImages and its three ranks                  src/sfm/incremental_mapper.cc:202-256, 46-73
//   Image::IncrementCorrespondenceHasPoint3D / Decrement...                src/base/image.cc:113-137
//   VisibilityPyramid::SetPoint / ResetPoint / CellForPoint                src/base/visibility_pyramid.cc:53-106
// The reference keeps NumVisiblePoints3D, NumObservations and the pyramid of every image incrementally; here they are computed
// from the scene arrays and the observations' points in one stateless call: the duplicate rule per pair (k_rt_dedup), a bit per
// point2D of every slot set by the kept matches of the problem's pairs (k_ni_visibility: integer atomicOr, idempotent), the
// counts by popcount and the score from the 64 x 64 occupancy of the visible points2D in LDS (k_ni_slot: a one-wave workgroup
// per slot, the five coarser levels by OR-ing 2 x 2 blocks), a packed key per slot and its place by counting inside the
// problem (k_ni_rank).
//   IncrementalMapper::FindLocalBundle                                     src/sfm/incremental_mapper.cc:932-1099
//   CalculateTriangulationAngles, Percentile                               src/base/triangulation.cc:147-181, src/util/math.h:231-246
// dsm_find_local_bundles, the second call of this file, is stateless in the same way: the observations' points are inverted into
// tracks (k_lb_track_hist, k_lb_scan), a workgroup per query counts the shared observations of its problem's images
// (k_lb_shared), the overlap lists are placed by counting (k_lb_overlap_rank), tri_angle of every (query, image) a threshold can
// reach is the rank of Percentile's index among the correctly rounded angles by bisection on their bits (k_lb_tri_angle), and
// the host runs the selection chain (lb_select).
// No floating-point atomics; every result is the same bytes for any batch and any memory budget.  The check build runs the
// sequential forms of next_images.h on one lane as well (DSM_NEXT_IMAGES_SERIAL).
#include <hip/hip_runtime.h>
#include <math.h>

#include <chrono>
#include <cstdlib>
#include <cstring>

#include "ctx.h"
#include "rt_dedup.h"
#include "verify_camera.h"

#define IP_HD static __host__ __device__ inline
#define IP_D static __device__ inline
#include "next_images.h"
#include "wave_reduce.h"

namespace {

constexpr int NI_BLOCK = 256;

// a lane per match of a (problem, pair) incidence: the kept ones mark both points2D as observed in the problem, and the other
// side of an observation with a point as visible
__global__ void __launch_bounds__(NI_BLOCK) k_ni_visibility(NiView v) {
  const uint32_t e = blockIdx.x;
  if (e >= v.n_entries) return;
  const uint32_t k = v.ent_pair[e], sa = v.ent_slot[2 * e], sb = v.ent_slot[2 * e + 1];
  const uint64_t wa = v.word_off[sa], wb = v.word_off[sb], oa = v.obs_off[sa], ob = v.obs_off[sb];
  for (uint64_t m = v.moff[k] + threadIdx.x; m < v.moff[k + 1]; m += NI_BLOCK) {
    if (!v.acc[m]) continue;
    const uint32_t a = v.matches[2 * m], b = v.matches[2 * m + 1];
    const uint32_t bit_a = 1u << (a & 31), bit_b = 1u << (b & 31);
    atomicOr(&v.has[wa + (a >> 5)], bit_a);
    atomicOr(&v.has[wb + (b >> 5)], bit_b);
    if (v.obs_point[oa + a] >= 0) atomicOr(&v.vis[wb + (b >> 5)], bit_b);
    if (v.obs_point[ob + b] >= 0) atomicOr(&v.vis[wa + (a >> 5)], bit_a);
  }
}

// the counts, the score and the key of one slot per one-wave workgroup: lane r owns row r of the occupancy
__global__ void __launch_bounds__(64) k_ni_slot(NiView v) {
  __shared__ uint32_t occ[2 * NI_DIM];  // the finest level: 64 rows of 64 bits, 512 bytes
  __shared__ uint64_t rows[NI_DIM];
  const uint32_t s = blockIdx.x, lane = threadIdx.x;
  if (s >= v.n_slots) return;
  const uint64_t w0 = v.word_off[s], w1 = v.word_off[s + 1];
  uint32_t nv = 0, no = 0;
  for (uint64_t w = w0 + lane; w < w1; w += 64) nv += __popc(v.vis[w]), no += __popc(v.has[w]);
  nv = wave_sum(nv), no = wave_sum(no);
  const uint32_t flags = v.slot_flags[s], img = v.slot_img[s];
  uint64_t score = 0;
  if (!(flags & NI_SLOT_REGISTERED)) {  // (uniform over the workgroup)
    occ[lane] = 0u, occ[lane + 64] = 0u;
    __syncthreads();
    const uint32_t n = (uint32_t)(v.obs_off[s + 1] - v.obs_off[s]);
    const uint64_t width = v.img_wh[2 * img], height = v.img_wh[2 * img + 1];
    for (uint32_t f = lane; f < n; f += 64) {
      if (!((v.vis[w0 + (f >> 5)] >> (f & 31)) & 1u)) continue;
      const double* xy = v.kp + 2 * ((size_t)v.row0[img] + f);
      const uint32_t cx = ni_cell(xy[0], width), cy = ni_cell(xy[1], height);
      atomicOr(&occ[2 * cy + (cx >> 5)], 1u << (cx & 31));
    }
    __syncthreads();
    uint64_t row = (uint64_t)occ[2 * lane] | ((uint64_t)occ[2 * lane + 1] << 32);
    uint32_t dim = NI_DIM;
    for (int level = NI_LEVELS - 1; level >= 0; --level, dim /= 2) {
      const uint32_t occupied = wave_sum(lane < dim ? (uint32_t)__popcll(row) : 0u);
      score += occupied * ni_level_weight(level);
      rows[lane] = row;
      __syncthreads();
      row = lane < dim / 2 ? ni_coarsen(rows[2 * lane], rows[2 * lane + 1]) : 0ull;
      __syncthreads();
    }
  }
  if (lane == 0) {
    v.num_visible[s] = nv, v.num_observations[s] = no, v.score[s] = score;
    v.key[s] = ni_key(flags, ni_eligible(flags, nv, v.min_num_inliers), ni_rank(v.method, nv, no, score), v.slot_id[s]);
  }
}

// an eligible slot's place in its problem's list: the number of the problem's keys below its own (keys are unique: the image
// id is part of them)
__global__ void __launch_bounds__(NI_BLOCK) k_ni_rank(NiView v, const uint32_t* __restrict__ slot_prob) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= v.n_slots) return;
  const uint64_t mine = v.key[s];
  if (mine == NI_KEY_NONE) return;
  const uint32_t p = slot_prob[s], s0 = v.slot_off[p], s1 = v.slot_off[p + 1];
  uint32_t r = 0;
  for (uint32_t t = s0; t < s1; ++t) r += v.key[t] < mine;
  v.order[s0 + r] = v.slot_id[s];
  atomicAdd(&v.order_n[p], 1u);
}

#ifdef DSM_CHECK_BUILD
// DSM_NEXT_IMAGES_SERIAL: the sequential forms, problem after problem, on one lane
__global__ void k_ni_serial(NiView v) {
  if (blockIdx.x || threadIdx.x) return;
  ni_serial(v);
}
#endif

// ================================================================== dsm_find_local_bundles
__global__ void __launch_bounds__(NI_BLOCK) k_lb_centers(LbView v) {
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= v.n_slots) return;
  double C[3] = {0.0, 0.0, 0.0};
  if (v.slot_flags[s] & NI_SLOT_REGISTERED) ip_projection_center(v.pose + 7 * (size_t)s, v.pose + 7 * (size_t)s + 4, C);
  v.center[3 * (size_t)s] = C[0], v.center[3 * (size_t)s + 1] = C[1], v.center[3 * (size_t)s + 2] = C[2];
}

// the tracks: a lane per observation counts into its point (integer atomics), one workgroup scans, a lane per observation takes
// its place in its point's list -- the order inside a list is free, only counts are read from it
__global__ void __launch_bounds__(NI_BLOCK) k_lb_track_hist(LbView v, const uint32_t* __restrict__ obs_slot, int scatter) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= v.n_obs || v.obs_point[i] < 0) return;
  const uint32_t s = obs_slot[i];
  const uint64_t g = v.point_off[v.slot_prob[s]] + v.obs_point[i];
  if (!scatter)
    atomicAdd(&v.trk_start[g], 1u);
  else
    v.trk_slot[v.trk_start[g] + atomicAdd(&v.trk_fill[g], 1u)] = s;
}
__global__ void __launch_bounds__(NI_BLOCK) k_lb_scan(uint32_t* __restrict__ a, uint64_t n) {  // exclusive, in place; a[n] = the total
  __shared__ uint32_t sh[NI_BLOCK];
  if (blockIdx.x) return;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < n; base += NI_BLOCK) {
    const uint64_t i = base + threadIdx.x;
    const uint32_t x = i < n ? a[i] : 0u;
    sh[threadIdx.x] = x;
    __syncthreads();
    for (int d = 1; d < NI_BLOCK; d *= 2) {
      const uint32_t y = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0u;
      __syncthreads();
      sh[threadIdx.x] += y;
      __syncthreads();
    }
    if (i < n) a[i] = carry + sh[threadIdx.x] - x;
    carry += sh[NI_BLOCK - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) a[n] = carry;
}

// the shared counts of one query per workgroup: a lane per point2D of the query walks its point's track (:947-957)
__global__ void __launch_bounds__(NI_BLOCK) k_lb_shared(LbView v, uint32_t q0, uint32_t nq) {
  const uint32_t q = q0 + blockIdx.x;
  if (blockIdx.x >= nq) return;
  const uint32_t qs = v.q_slot[q], p = v.slot_prob[qs], s0 = v.slot_off[p];
  const uint64_t r0 = v.row_off[q] - v.row_off[q0];
  uint32_t np = 0;
  for (uint64_t i = v.obs_off[qs] + threadIdx.x; i < v.obs_off[qs + 1]; i += NI_BLOCK) {
    if (v.obs_point[i] < 0) continue;
    ++np;
    const uint64_t g = v.point_off[p] + v.obs_point[i];
    for (uint32_t t = v.trk_start[g]; t < v.trk_start[g + 1]; ++t) {
      const uint32_t s = v.trk_slot[t];
      if (s != qs) atomicAdd(&v.shared[r0 + (s - s0)], 1u);
    }
  }
  if (np) atomicAdd(&v.q_points[q - q0], np);
}

// an overlapping image's place in its query's list: the number of the query's overlap keys below its own
__global__ void __launch_bounds__(NI_BLOCK) k_lb_overlap_rank(LbView v, uint32_t q0, uint64_t n_rows, const uint32_t* __restrict__ row_query) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows || !v.shared[r]) return;
  const uint32_t q = row_query[r], qs = v.q_slot[q], p = v.slot_prob[qs], s0 = v.slot_off[p], n = v.slot_off[p + 1] - s0;
  const uint64_t r0 = v.row_off[q] - v.row_off[q0];
  const uint64_t mine = lb_overlap_key(v.shared[r], v.slot_id[s0 + (uint32_t)(r - r0)]);
  uint32_t place = 0;
  for (uint32_t j = 0; j < n; ++j) place += v.shared[r0 + j] && lb_overlap_key(v.shared[r0 + j], v.slot_id[s0 + j]) < mine;
  v.ov_slot[r0 + place] = s0 + (uint32_t)(r - r0);
  atomicAdd(&v.ov_n[q - q0], 1u);
}

struct LbItems {
  uint32_t n;
  const uint32_t* slots;   // [2 n] the query's slot, the other slot
  const uint64_t* off;     // [n + 1] the items' lists of angle bits: one per point2D of the query
  const uint32_t* count;   // [n] the query's NumPoints3D
  uint64_t* bits;
  double* tri_angle;       // [n]
};

// tri_angle of one (query, overlapping image) per one-wave workgroup: the angle of every point2D of the query with a point, the
// rank of Percentile's index by bisection on the bits (ip_select_bits, as k_ip_relative_pose takes its median)
__global__ void __launch_bounds__(64) k_lb_tri_angle(LbView v, LbItems it) {
  const uint32_t c = blockIdx.x, lane = threadIdx.x;
  if (c >= it.n) return;
  const uint32_t qs = it.slots[2 * c], other = it.slots[2 * c + 1], p = v.slot_prob[qs];
  const uint64_t o0 = v.obs_off[qs], n = v.obs_off[qs + 1] - o0;
  uint64_t* bits = it.bits + it.off[c];
  const double* c1 = v.center + 3 * (size_t)qs;
  const double* c2 = v.center + 3 * (size_t)other;
  for (uint64_t f = lane; f < n; f += 64) {
    const int32_t pt = v.obs_point[o0 + f];
    bits[f] = pt >= 0 ? ip_double_bits(ip_tri_angle(c1, c2, v.point_xyz + 3 * (v.point_off[p] + (uint64_t)pt))) : LB_NO_ANGLE;
  }
  __syncthreads();
  auto count_below = [&](uint64_t x) {
    uint32_t cnt = 0;
    for (uint64_t f = lane; f < n; f += 64) cnt += bits[f] < x;
    return (uint64_t)wave_sum(cnt);
  };
  const uint64_t sel = ip_select_bits(lb_percentile_index(it.count[c]), count_below);
  if (lane == 0) it.tri_angle[c] = ip_bits_double(sel);
}

#ifdef DSM_CHECK_BUILD
// DSM_NEXT_IMAGES_SERIAL: the sequential forms on one lane
__global__ void k_lb_serial_tracks(LbView v) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t s = 0; s < v.n_slots; ++s) {
    double C[3] = {0.0, 0.0, 0.0};
    if (v.slot_flags[s] & NI_SLOT_REGISTERED) ip_projection_center(v.pose + 7 * (size_t)s, v.pose + 7 * (size_t)s + 4, C);
    v.center[3 * (size_t)s] = C[0], v.center[3 * (size_t)s + 1] = C[1], v.center[3 * (size_t)s + 2] = C[2];
  }
  lb_serial_tracks(v);
}
__global__ void k_lb_serial_overlap(LbView v, uint32_t q0, uint32_t nq) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t q = q0; q < q0 + nq; ++q) lb_serial_overlap(v, q, q0);
}
__global__ void k_lb_serial_tri_angle(LbView v, LbItems it) {
  if (blockIdx.x || threadIdx.x) return;
  for (uint32_t c = 0; c < it.n; ++c)
    it.tri_angle[c] = lb_serial_tri_angle(v, it.slots[2 * c], it.slots[2 * c + 1], reinterpret_cast<double*>(it.bits + it.off[c]));
}
#endif

struct LbBufs {
  DevBuf slot_off, slot_id, slot_flags, slot_prob, obs_off, obs_point, obs_slot, point_off, point_xyz, pose, center, trk_start, trk_fill, trk_slot;
  DevBuf q_slot, row_off, row_query, shared, q_points, ov_slot, ov_n, it_slots, it_off, it_count, it_bits, it_angle;
};

struct NiBufs {
  DevBuf pair_img, moff, matches, nfeat, acc, kp, row0, img_wh;
  DevBuf slot_off, slot_img, slot_id, slot_flags, slot_prob, obs_off, obs_point, word_off, ent_off, ent_pair, ent_slot;
  DevBuf bits, num_visible, num_observations, score, key, order, order_n;
};

}  // namespace

extern "C" void dsm_default_next_images_options(dsm_next_images_options* o) { ni_default_options(o); }

extern "C" int dsm_find_next_images(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                               uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                               const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                                               const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                               uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                                               const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                                               const uint32_t* slot_num_reg_trials, const uint8_t* slot_filtered,
                                               const dsm_next_images_options* options, uint64_t* next_offsets, uint32_t* next_image_ids,
                                               uint64_t next_capacity, uint32_t* slot_num_visible, uint32_t* slot_num_observations,
                                               uint64_t* slot_score, dsm_next_images_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](int code, const char* msg) { return dsm_fail(ctx, code, "dsm_find_next_images", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  dsm_next_images_options o;
  if (options)
    o = *options;
  else
    ni_default_options(&o);
  if (num_cameras && !cameras) return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  for (uint32_t c = 0; c < num_cameras; ++c) {
    if (!cam_model_exists(cameras[c].model_id)) return fail(DSM_ERR_INVALID_ARGUMENT, "an unknown camera model");
    for (int i = 0; i < cam_num_params(cameras[c].model_id); ++i)
      if (!std::isfinite(cameras[c].params[i])) return fail(DSM_ERR_INVALID_ARGUMENT, "non-finite camera parameters");
  }
  NiSetup N;
  if (const char* bad = N.load(num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, points2D_offsets, points2D_xy, num_pairs,
                               pair_image_ids, match_offsets, matches, num_problems, problem_image_offsets, problem_image_ids, slot_registered,
                               slot_obs_offsets, slot_obs_point3D, slot_num_reg_trials, slot_filtered, o))
    return fail(N.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT, bad);
  if (num_problems && (!next_offsets || !next_image_ids)) return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  const uint64_t F = points2D_offsets[num_images], NM = match_offsets[num_pairs];
  const uint32_t n_slots = (uint32_t)N.slot_img.size();
  dsm_next_images_report rep{};
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  bool serial = false;
#ifdef DSM_CHECK_BUILD
  if (const char* dv = ctx->dbg("DSM_NEXT_IMAGES_SERIAL")) serial = atoi(dv) != 0;
#endif

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  NiBufs d;
  DevEvents<3> ev;
  DevEvents<4> bev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, bev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));

  // ------------------------------------------------------------ the scene and the duplicate rule
  HIPCHK(ctx, dev_upload(d.nfeat, N.S.nfeat.data(), (size_t)num_images * 4, st));
  HIPCHK(ctx, dev_upload(d.row0, points2D_offsets, ((size_t)num_images + 1) * 4, st));
  HIPCHK(ctx, dev_upload(d.img_wh, N.img_wh.data(), N.img_wh.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.kp, points2D_xy, F * 16, st));
  HIPCHK(ctx, dev_upload(d.pair_img, N.S.pair_img.data(), N.S.pair_img.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.moff, match_offsets, ((size_t)num_pairs + 1) * 8, st));
  HIPCHK(ctx, dev_upload(d.matches, matches, NM * 8, st));
  HIPCHK(ctx, d.acc.reserve(std::max<uint64_t>(NM, 16)));
  if (num_pairs) {
    hipLaunchKernelGGL(k_rt_dedup, dim3(num_pairs), dim3(NI_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.nfeat.as<uint32_t>(), d.acc.as<uint8_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, hipEventRecord(ev[1], st));

  // ------------------------------------------------------------ the batches: whole problems, cut where the memory budget asks
  std::vector<uint32_t> h_nv(n_slots), h_no(n_slots), h_order(n_slots), h_order_n(num_problems);
  std::vector<uint64_t> h_score(n_slots);
  // what a slot costs on the device: its observations' points, its two bitmaps and its per-slot words
  auto problem_bytes = [&](uint32_t p) {
    const uint32_t s0 = N.slot_off[p], s1 = N.slot_off[p + 1];
    return (N.obs_off[s1] - N.obs_off[s0]) * 4 + (N.word_off[s1] - N.word_off[s0]) * 8 + (uint64_t)(s1 - s0) * 64 +
           (uint64_t)(N.ent_off[p + 1] - N.ent_off[p]) * 12;
  };
  std::vector<uint32_t> b_slot_off, b_ent_off, b_ent_slot, b_slot_prob;
  std::vector<uint64_t> b_obs_off, b_word_off;
  double ms = 0;
  for (uint32_t p0 = 0; p0 < num_problems;) {
    uint32_t p1 = p0;
    uint64_t bytes = 0;
    for (; p1 < num_problems; ++p1) {
      const uint64_t mine = problem_bytes(p1);
      if (ctx->memory_budget && p1 > p0 && bytes + mine > ctx->memory_budget) break;
      bytes += mine;
    }
    ++rep.num_batches;
    const uint32_t nP = p1 - p0, sb = N.slot_off[p0], nS = N.slot_off[p1] - sb, eb = N.ent_off[p0], nE = N.ent_off[p1] - eb;
    const uint64_t ob = N.obs_off[sb], nO = N.obs_off[sb + nS] - ob, wb = N.word_off[sb], nW = N.word_off[sb + nS] - wb;
    b_slot_off.resize((size_t)nP + 1), b_ent_off.resize((size_t)nP + 1), b_slot_prob.resize(nS), b_ent_slot.resize(2 * (size_t)nE);
    b_obs_off.resize((size_t)nS + 1), b_word_off.resize((size_t)nS + 1);
    for (uint32_t p = 0; p <= nP; ++p) b_slot_off[p] = N.slot_off[p0 + p] - sb, b_ent_off[p] = N.ent_off[p0 + p] - eb;
    for (uint32_t p = 0; p < nP; ++p)
      for (uint32_t s = b_slot_off[p]; s < b_slot_off[p + 1]; ++s) b_slot_prob[s] = p;
    for (uint32_t s = 0; s <= nS; ++s) b_obs_off[s] = N.obs_off[sb + s] - ob, b_word_off[s] = N.word_off[sb + s] - wb;
    for (size_t i = 0; i < b_ent_slot.size(); ++i) b_ent_slot[i] = N.ent_slot[2 * (size_t)eb + i] - sb;
    HIPCHK(ctx, hipEventRecord(bev[0], st));
    HIPCHK(ctx, dev_upload(d.slot_off, b_slot_off.data(), b_slot_off.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.ent_off, b_ent_off.data(), b_ent_off.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.slot_prob, b_slot_prob.data(), (size_t)nS * 4, st));
    HIPCHK(ctx, dev_upload(d.slot_img, N.slot_img.data() + sb, (size_t)nS * 4, st));
    HIPCHK(ctx, dev_upload(d.slot_id, N.slot_id.data() + sb, (size_t)nS * 4, st));
    HIPCHK(ctx, dev_upload(d.slot_flags, N.slot_flags.data() + sb, (size_t)nS * 4, st));
    HIPCHK(ctx, dev_upload(d.obs_off, b_obs_off.data(), b_obs_off.size() * 8, st));
    HIPCHK(ctx, dev_upload(d.word_off, b_word_off.data(), b_word_off.size() * 8, st));
    HIPCHK(ctx, dev_upload(d.obs_point, nO ? slot_obs_point3D + ob : nullptr, nO * 4, st));
    HIPCHK(ctx, dev_upload(d.ent_pair, N.ent_pair.data() + eb, (size_t)nE * 4, st));
    HIPCHK(ctx, dev_upload(d.ent_slot, b_ent_slot.data(), b_ent_slot.size() * 4, st));
    HIPCHK(ctx, dev_fill(d.bits, 0, 2 * nW * 4, st));
    HIPCHK(ctx, d.num_visible.reserve(std::max<size_t>((size_t)nS * 4, 16)));
    HIPCHK(ctx, d.num_observations.reserve(std::max<size_t>((size_t)nS * 4, 16)));
    HIPCHK(ctx, d.score.reserve(std::max<size_t>((size_t)nS * 8, 16)));
    HIPCHK(ctx, d.key.reserve(std::max<size_t>((size_t)nS * 8, 16)));
    HIPCHK(ctx, dev_fill(d.order, 0, (size_t)nS * 4, st));
    HIPCHK(ctx, dev_fill(d.order_n, 0, (size_t)nP * 4, st));
    NiView v;
    v.n_problems = nP, v.n_slots = nS, v.n_entries = nE;
    v.slot_off = d.slot_off.as<uint32_t>(), v.slot_img = d.slot_img.as<uint32_t>(), v.slot_id = d.slot_id.as<uint32_t>();
    v.slot_flags = d.slot_flags.as<uint32_t>(), v.obs_off = d.obs_off.as<uint64_t>(), v.obs_point = d.obs_point.as<int32_t>();
    v.word_off = d.word_off.as<uint64_t>(), v.ent_off = d.ent_off.as<uint32_t>(), v.ent_pair = d.ent_pair.as<uint32_t>();
    v.ent_slot = d.ent_slot.as<uint32_t>(), v.moff = d.moff.as<uint64_t>(), v.matches = d.matches.as<uint32_t>(), v.acc = d.acc.as<uint8_t>();
    v.row0 = d.row0.as<uint32_t>(), v.kp = d.kp.as<double>(), v.img_wh = d.img_wh.as<uint64_t>();
    v.vis = d.bits.as<uint32_t>(), v.has = d.bits.as<uint32_t>() + nW;
    v.num_visible = d.num_visible.as<uint32_t>(), v.num_observations = d.num_observations.as<uint32_t>(), v.score = d.score.as<uint64_t>();
    v.key = d.key.as<uint64_t>(), v.order = d.order.as<uint32_t>(), v.order_n = d.order_n.as<uint32_t>();
    v.method = o.image_selection_method, v.min_num_inliers = (uint32_t)o.abs_pose_min_num_inliers;
    if (serial) {
#ifdef DSM_CHECK_BUILD
      hipLaunchKernelGGL(k_ni_serial, dim3(1), dim3(1), 0, st, v);
#endif
      HIPCHK(ctx, hipEventRecord(bev[1], st));
      HIPCHK(ctx, hipEventRecord(bev[2], st));
    } else {
      if (nE) hipLaunchKernelGGL(k_ni_visibility, dim3(nE), dim3(NI_BLOCK), 0, st, v);
      HIPCHK(ctx, hipEventRecord(bev[1], st));
      if (nS) hipLaunchKernelGGL(k_ni_slot, dim3(nS), dim3(64), 0, st, v);
      HIPCHK(ctx, hipEventRecord(bev[2], st));
      if (nS) hipLaunchKernelGGL(k_ni_rank, dim3((nS + NI_BLOCK - 1) / NI_BLOCK), dim3(NI_BLOCK), 0, st, v, d.slot_prob.as<uint32_t>());
    }
    HIPCHK(ctx, hipGetLastError());
    if (nS) {
      HIPCHK(ctx, hipMemcpyAsync(h_nv.data() + sb, d.num_visible.p, (size_t)nS * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(h_no.data() + sb, d.num_observations.p, (size_t)nS * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(h_score.data() + sb, d.score.p, (size_t)nS * 8, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(h_order.data() + sb, d.order.p, (size_t)nS * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(h_order_n.data() + p0, d.order_n.p, (size_t)nP * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipEventRecord(bev[3], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, bev.ms(0, 1, &ms));
    rep.visibility_ms += ms;
    HIPCHK(ctx, bev.ms(1, 2, &ms));
    rep.score_ms += ms;
    HIPCHK(ctx, bev.ms(2, 3, &ms));
    rep.rank_ms += ms;
    p0 = p1;
  }
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, ev.ms(0, 1, &rep.graph_ms));
  HIPCHK(ctx, ev.ms(0, 2, &rep.device_ms));

  // ------------------------------------------------------------ the results
  uint64_t total = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    if (h_order_n[p] > N.slot_off[p + 1] - N.slot_off[p]) return fail(DSM_ERR_HIP, "the ranking overran its list");
    total += h_order_n[p];
  }
  if (total > next_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "next_image_ids is too small");
  uint64_t at = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    next_offsets[p] = at;
    for (uint32_t i = 0; i < h_order_n[p]; ++i) next_image_ids[at++] = h_order[N.slot_off[p] + i];
  }
  if (num_problems) next_offsets[num_problems] = at;
  for (uint32_t s = 0; s < n_slots; ++s) {
    if (slot_num_visible) slot_num_visible[s] = h_nv[s];
    if (slot_num_observations) slot_num_observations[s] = h_no[s];
    if (slot_score) slot_score[s] = h_score[s];
    const bool eligible = ni_eligible(N.slot_flags[s], h_nv[s], (uint32_t)o.abs_pose_min_num_inliers);
    rep.num_eligible += eligible;
    rep.num_first_bucket += eligible && !(N.slot_flags[s] & NI_SLOT_SECOND);
    rep.num_second_bucket += eligible && (N.slot_flags[s] & NI_SLOT_SECOND);
  }
  if (report) *report = rep;
  return DSM_OK;
}

extern "C" void dsm_default_local_bundle_selection_options(dsm_local_bundle_selection_options* o) { lb_default_options(o); }

extern "C" int dsm_find_local_bundles(dsm_ctx* ctx, uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets,
                                                 uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                                                 const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                                                 const double* slot_qvec, const double* slot_tvec, const uint64_t* point_offsets,
                                                 const double* point_xyz, uint32_t num_queries, const uint32_t* query_problem,
                                                 const uint32_t* query_image_id, const dsm_local_bundle_selection_options* options,
                                                 uint64_t* bundle_offsets, uint32_t* bundle_image_ids, uint64_t bundle_capacity,
                                                 uint64_t* overlap_offsets, uint32_t* overlap_image_ids, uint32_t* overlap_shared,
                                                 double* overlap_tri_angle, uint64_t overlap_capacity, dsm_local_bundle_selection_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](int code, const char* msg) { return dsm_fail(ctx, code, "dsm_find_local_bundles", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  dsm_local_bundle_selection_options o;
  if (options)
    o = *options;
  else
    lb_default_options(&o);
  LbSetup L;
  if (const char* bad = L.load(num_images, image_ids, points2D_offsets, num_problems, problem_image_offsets, problem_image_ids, slot_registered,
                               slot_obs_offsets, slot_obs_point3D, slot_qvec, slot_tvec, point_offsets, point_xyz, num_queries, query_problem,
                               query_image_id, o))
    return fail(L.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT, bad);
  const bool want_overlap = overlap_offsets || overlap_image_ids || overlap_shared || overlap_tri_angle;
  if ((num_queries && (!bundle_offsets || !bundle_image_ids)) ||
      (want_overlap && num_queries && (!overlap_offsets || !overlap_image_ids || !overlap_shared || !overlap_tri_angle)))
    return fail(DSM_ERR_INVALID_ARGUMENT, "NULL argument");
  const NiSetup& N = L.N;
  const uint32_t n_slots = (uint32_t)N.slot_img.size();
  const uint64_t n_obs = N.obs_off[n_slots], n_points = point_offsets[num_problems];
  dsm_local_bundle_selection_report rep{};
  rep.min_tri_angle_margin = INFINITY;
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  bool serial = false;
#ifdef DSM_CHECK_BUILD
  if (const char* dv = ctx->dbg("DSM_NEXT_IMAGES_SERIAL")) serial = atoi(dv) != 0;
#endif

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  LbBufs d;
  DevEvents<3> ev, bev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, bev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  auto grid = [](uint64_t n) { return dim3(dsm_grid(n, NI_BLOCK)); };

  // ------------------------------------------------------------ the state, the centres, the tracks
  std::vector<uint32_t> obs_slot(n_obs);
  for (uint32_t s = 0; s < n_slots; ++s)
    for (uint64_t i = N.obs_off[s]; i < N.obs_off[s + 1]; ++i) obs_slot[i] = s;
  HIPCHK(ctx, dev_upload(d.slot_off, N.slot_off.data(), N.slot_off.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.slot_id, N.slot_id.data(), (size_t)n_slots * 4, st));
  HIPCHK(ctx, dev_upload(d.slot_flags, N.slot_flags.data(), (size_t)n_slots * 4, st));
  HIPCHK(ctx, dev_upload(d.slot_prob, L.slot_prob.data(), (size_t)n_slots * 4, st));
  HIPCHK(ctx, dev_upload(d.obs_off, N.obs_off.data(), N.obs_off.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.obs_point, slot_obs_point3D, n_obs * 4, st));
  HIPCHK(ctx, dev_upload(d.obs_slot, obs_slot.data(), n_obs * 4, st));
  HIPCHK(ctx, dev_upload(d.point_off, point_offsets, ((size_t)num_problems + 1) * 8, st));
  HIPCHK(ctx, dev_upload(d.point_xyz, point_xyz, n_points * 24, st));
  HIPCHK(ctx, dev_upload(d.pose, L.pose.data(), L.pose.size() * 8, st));
  HIPCHK(ctx, d.center.reserve(std::max<size_t>((size_t)n_slots * 24, 16)));
  HIPCHK(ctx, dev_fill(d.trk_start, 0, (n_points + 1) * 4, st));
  HIPCHK(ctx, dev_fill(d.trk_fill, 0, n_points * 4, st));
  HIPCHK(ctx, d.trk_slot.reserve(std::max<uint64_t>(n_obs * 4, 16)));
  HIPCHK(ctx, dev_upload(d.q_slot, L.q_slot.data(), (size_t)num_queries * 4, st));
  HIPCHK(ctx, dev_upload(d.row_off, L.row_off.data(), L.row_off.size() * 8, st));
  LbView v;
  v.n_problems = num_problems, v.n_slots = n_slots, v.n_queries = num_queries, v.n_obs = n_obs, v.n_points = n_points;
  v.slot_off = d.slot_off.as<uint32_t>(), v.slot_id = d.slot_id.as<uint32_t>(), v.slot_flags = d.slot_flags.as<uint32_t>();
  v.slot_prob = d.slot_prob.as<uint32_t>(), v.obs_off = d.obs_off.as<uint64_t>(), v.obs_point = d.obs_point.as<int32_t>();
  v.point_off = d.point_off.as<uint64_t>(), v.point_xyz = d.point_xyz.as<double>(), v.pose = d.pose.as<double>(), v.center = d.center.as<double>();
  v.trk_start = d.trk_start.as<uint32_t>(), v.trk_fill = d.trk_fill.as<uint32_t>(), v.trk_slot = d.trk_slot.as<uint32_t>();
  v.q_slot = d.q_slot.as<uint32_t>(), v.row_off = d.row_off.as<uint64_t>();
  v.shared = v.q_points = v.ov_slot = v.ov_n = nullptr;
  if (serial) {
#ifdef DSM_CHECK_BUILD
    hipLaunchKernelGGL(k_lb_serial_tracks, dim3(1), dim3(1), 0, st, v);
#endif
  } else {
    if (n_slots) hipLaunchKernelGGL(k_lb_centers, grid(n_slots), dim3(NI_BLOCK), 0, st, v);
    if (n_obs) hipLaunchKernelGGL(k_lb_track_hist, grid(n_obs), dim3(NI_BLOCK), 0, st, v, d.obs_slot.as<uint32_t>(), 0);
    hipLaunchKernelGGL(k_lb_scan, dim3(1), dim3(NI_BLOCK), 0, st, d.trk_start.as<uint32_t>(), n_points);
    if (n_obs) hipLaunchKernelGGL(k_lb_track_hist, grid(n_obs), dim3(NI_BLOCK), 0, st, v, d.obs_slot.as<uint32_t>(), 1);
  }
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[1], st));

  // ------------------------------------------------------------ the batches: whole queries, cut where the memory budget asks
  struct Answer {
    std::vector<uint32_t> ids, shared, bundle;
    std::vector<double> tri_angle;
  };
  std::vector<Answer> answers(num_queries);
  // what a query costs on the device: its rows, and a list of angle bits per overlapping image
  auto query_bytes = [&](uint32_t q) {
    const uint64_t rows = L.row_off[q + 1] - L.row_off[q], n = N.obs_off[L.q_slot[q] + 1] - N.obs_off[L.q_slot[q]];
    return rows * 32 + rows * n * 8;
  };
  std::vector<uint32_t> row_query, h_shared, h_ov_slot, h_ov_n, h_points, it_slots, it_count, it_query;
  std::vector<uint64_t> it_off;
  std::vector<double> it_angle;
  std::vector<uint8_t> used;
  double ms = 0;
  for (uint32_t q0 = 0; q0 < num_queries;) {
    uint32_t q1 = q0;
    uint64_t bytes = 0;
    for (; q1 < num_queries; ++q1) {
      const uint64_t mine = query_bytes(q1);
      if (ctx->memory_budget && q1 > q0 && bytes + mine > ctx->memory_budget) break;
      bytes += mine;
    }
    ++rep.num_batches;
    const uint32_t nq = q1 - q0;
    const uint64_t r_base = L.row_off[q0], n_rows = L.row_off[q1] - r_base;
    row_query.resize(n_rows);
    for (uint32_t q = q0; q < q1; ++q)
      for (uint64_t r = L.row_off[q]; r < L.row_off[q + 1]; ++r) row_query[r - r_base] = q;
    HIPCHK(ctx, hipEventRecord(bev[0], st));
    HIPCHK(ctx, dev_upload(d.row_query, row_query.data(), n_rows * 4, st));
    HIPCHK(ctx, dev_fill(d.shared, 0, n_rows * 4, st));
    HIPCHK(ctx, dev_fill(d.ov_slot, 0, n_rows * 4, st));
    HIPCHK(ctx, dev_fill(d.q_points, 0, (size_t)nq * 4, st));
    HIPCHK(ctx, dev_fill(d.ov_n, 0, (size_t)nq * 4, st));
    v.shared = d.shared.as<uint32_t>(), v.q_points = d.q_points.as<uint32_t>(), v.ov_slot = d.ov_slot.as<uint32_t>(), v.ov_n = d.ov_n.as<uint32_t>();
    if (serial) {
#ifdef DSM_CHECK_BUILD
      hipLaunchKernelGGL(k_lb_serial_overlap, dim3(1), dim3(1), 0, st, v, q0, nq);
#endif
    } else {
      hipLaunchKernelGGL(k_lb_shared, dim3(nq), dim3(NI_BLOCK), 0, st, v, q0, nq);
      if (n_rows) hipLaunchKernelGGL(k_lb_overlap_rank, grid(n_rows), dim3(NI_BLOCK), 0, st, v, q0, n_rows, d.row_query.as<uint32_t>());
    }
    HIPCHK(ctx, hipGetLastError());
    h_shared.resize(n_rows), h_ov_slot.resize(n_rows), h_ov_n.resize(nq), h_points.resize(nq);
    if (n_rows) {
      HIPCHK(ctx, hipMemcpyAsync(h_shared.data(), d.shared.p, n_rows * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipMemcpyAsync(h_ov_slot.data(), d.ov_slot.p, n_rows * 4, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipMemcpyAsync(h_ov_n.data(), d.ov_n.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(h_points.data(), d.q_points.p, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipEventRecord(bev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    // the overlap lists; the items: every image a threshold of a chained query can reach
    it_slots.clear(), it_count.clear(), it_query.clear(), it_off.assign(1, 0);
    for (uint32_t q = q0; q < q1; ++q) {
      Answer& a = answers[q];
      const uint32_t p = L.slot_prob[L.q_slot[q]], s0 = N.slot_off[p], n = h_ov_n[q - q0];
      const uint64_t r0 = L.row_off[q] - r_base;
      if (n > L.row_off[q + 1] - L.row_off[q]) return fail(DSM_ERR_HIP, "an overlap list overran its rows");
      a.ids.resize(n), a.shared.resize(n), a.tri_angle.assign(n, -1.0);
      for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = h_ov_slot[r0 + i];
        if (s < s0 || s >= N.slot_off[p + 1]) return fail(DSM_ERR_HIP, "an overlap list left its problem");
        a.ids[i] = N.slot_id[s], a.shared[i] = h_shared[r0 + (s - s0)];
        if (n > (uint32_t)(o.local_ba_num_images - 1) && lb_reachable(a.shared[i], h_points[q - q0])) {
          it_slots.push_back(L.q_slot[q]), it_slots.push_back(s), it_count.push_back(h_points[q - q0]), it_query.push_back(q);
          it_query.push_back(i);
          it_off.push_back(it_off.back() + (N.obs_off[L.q_slot[q] + 1] - N.obs_off[L.q_slot[q]]));
        }
      }
    }
    const uint32_t n_items = (uint32_t)it_count.size();
    it_angle.resize(n_items);
    if (n_items) {
      HIPCHK(ctx, dev_upload(d.it_slots, it_slots.data(), it_slots.size() * 4, st));
      HIPCHK(ctx, dev_upload(d.it_off, it_off.data(), it_off.size() * 8, st));
      HIPCHK(ctx, dev_upload(d.it_count, it_count.data(), it_count.size() * 4, st));
      HIPCHK(ctx, d.it_bits.reserve(std::max<uint64_t>(it_off.back() * 8, 16)));
      HIPCHK(ctx, d.it_angle.reserve((size_t)n_items * 8));
      LbItems it{n_items, d.it_slots.as<uint32_t>(), d.it_off.as<uint64_t>(), d.it_count.as<uint32_t>(), d.it_bits.as<uint64_t>(), d.it_angle.as<double>()};
      if (serial) {
#ifdef DSM_CHECK_BUILD
        hipLaunchKernelGGL(k_lb_serial_tri_angle, dim3(1), dim3(1), 0, st, v, it);
#endif
      } else {
        hipLaunchKernelGGL(k_lb_tri_angle, dim3(n_items), dim3(64), 0, st, v, it);
      }
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipMemcpyAsync(it_angle.data(), d.it_angle.p, (size_t)n_items * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(bev[2], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, bev.ms(0, 1, &ms));
    rep.overlap_ms += ms;
    HIPCHK(ctx, bev.ms(1, 2, &ms));
    rep.angles_ms += ms;
    rep.num_angles += n_items;
    for (uint32_t c = 0; c < n_items; ++c) answers[it_query[2 * c]].tri_angle[it_query[2 * c + 1]] = it_angle[c];
    // the selection chain of every query (a dozen compares each)
    for (uint32_t q = q0; q < q1; ++q) {
      Answer& a = answers[q];
      const uint32_t n = (uint32_t)a.ids.size();
      a.bundle.resize(std::min<uint32_t>(n, (uint32_t)(o.local_ba_num_images - 1)));
      used.resize(n + 1);
      const LbChain ch = lb_select(n, a.ids.data(), a.shared.data(), a.tri_angle.data(), h_points[q - q0], o.local_ba_num_images,
                                   o.local_ba_min_tri_angle, used.data(), a.bundle.data());
      if (ch.n_out != a.bundle.size()) return fail(DSM_ERR_HIP, "a selection chain ended short");
      rep.min_tri_angle_margin = std::min(rep.min_tri_angle_margin, ch.margin);
      rep.num_filled += ch.n_filled;
      if (n > (uint32_t)(o.local_ba_num_images - 1))
        ++rep.num_chained;
      else
        ++rep.num_copied;
    }
    q0 = q1;
  }
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  HIPCHK(ctx, ev.ms(0, 1, &rep.tracks_ms));
  HIPCHK(ctx, ev.ms(0, 2, &rep.device_ms));

  // ------------------------------------------------------------ the results
  uint64_t n_bundle = 0, n_overlap = 0;
  for (const Answer& a : answers) n_bundle += a.bundle.size(), n_overlap += a.ids.size();
  if (n_bundle > bundle_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "bundle_image_ids is too small");
  if (want_overlap && n_overlap > overlap_capacity) return fail(DSM_ERR_OUT_OF_RANGE, "the overlap lists are too small");
  uint64_t at_b = 0, at_o = 0;
  for (uint32_t q = 0; q < num_queries; ++q) {
    const Answer& a = answers[q];
    bundle_offsets[q] = at_b;
    for (uint32_t id : a.bundle) bundle_image_ids[at_b++] = id;
    if (!want_overlap) continue;
    overlap_offsets[q] = at_o;
    for (size_t i = 0; i < a.ids.size(); ++i, ++at_o)
      overlap_image_ids[at_o] = a.ids[i], overlap_shared[at_o] = a.shared[i], overlap_tri_angle[at_o] = a.tri_angle[i];
  }
  if (num_queries) bundle_offsets[num_queries] = at_b;
  if (num_queries && want_overlap) overlap_offsets[num_queries] = at_o;
  if (report) *report = rep;
  return DSM_OK;
}
