// retriangulation.hip -- re-triangulation of the separator images ("Re-triangulation"), and of the under-reconstructed pairs (below).
//   DistributedMapperController::Triangulate                       src/controllers/distributed_mapper_controller.cpp:823-834
//   IncrementalTriangulator::TriangulateImage / Find / Create / Continue   src/sfm/incremental_triangulator.cc:61-117, 419-586
//   EstimateTriangulation, TriangulationEstimator                   src/estimators/triangulation.cc
//   LORANSAC + InlierSupportMeasurer + CombinationSampler           src/optim/loransac.h:91-233, combination_sampler.cc
//   TriangulatePoint / TriangulateMultiViewPoint / CalculateTriangulationAngle   src/base/triangulation.cc
//   CorrespondenceGraph::AddCorrespondences / IsTwoViewObservation  src/base/correspondence_graph.cc:77-161, 250-261
// The graph: one workgroup per verified pair applies the duplicate rule in match order (an LDS bitmap of the pair's two
// images) and flags the accepted matches; each becomes two directed entries placed in its source feature's CSR segment
// (integer-atomic counts, a fixed-block scan), and every segment is then sorted by pair index -- a feature has at most one
// correspondence per pair, so this is the reference's (pair, match) append order whatever order the atomics took.
// The problems: one per (separator in ascending id, point2D) with a non-empty filtered correspondence list.  A problem reads
// and writes only its own feature set (the reference feature and its correspondences) and point xyz never changes, so the
// host schedules the problems into rounds before any solve: in sequential order, a problem commits in the current round when
// its feature set meets no set of an earlier problem of the round (committed or deferred), otherwise it is deferred to the
// next round.  That is one pass in problem order (a problem's round is 1 + the largest round of the earlier problems sharing
// a feature with it), and every round is enqueued at once without a host sync.  Each round then solves its committed
// problems at once, one lane per problem (Continue, then the Create chain with its recursion: LORANSAC, trials in sampler
// order), and writes their results into the feature -> point state.
// New points carry slot ids while the rounds run; the host numbers them in (separator, point2D, depth) order at the end.
// No floating-point atomics: every result is the same bytes for any schedule, any order of the points3D and of the matches
// inside a pair (as long as the duplicate rule does not fire).
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <cmath>
#include <limits>
#include <numeric>
#include <string>
#include <vector>

#include "camera_bogus.h"
#include "ctx.h"
#include "tri_angle.h"
#include "rt_graph.h"
#include "rt_loransac.h"
#include "verify_camera.h"
#include "verify_linalg.h"

namespace {

constexpr int RT_BLOCK = 256;
static_assert(RT_BLOCK == RT_GRAPH_BLOCK, "rt_scan launches rt_graph.h's scan kernels with RT_BLOCK lanes");
constexpr uint32_t kRtMaxPoints2D = 262144;   // per image: the pair's two images fit one 64 KiB LDS bitmap

// Find (max_transitivity 1): the correspondences on usable images, counted and then written
__global__ void k_rt_find(uint32_t Q, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ goff, const uint32_t* __restrict__ gval,
                          const uint32_t* __restrict__ feat_img, const uint8_t* __restrict__ img_ok, const uint32_t* __restrict__ moff,
                          uint32_t* __restrict__ cnt, uint32_t* __restrict__ mem) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= Q) return;
  const uint32_t f = ref[q];
  uint32_t c = 0;
  for (uint32_t e = goff[f]; e < goff[f + 1]; ++e) {
    const uint32_t g = gval[e];
    if (!img_ok[feat_img[g]]) continue;
    if (mem) mem[moff[q] + c] = g;
    ++c;
  }
  if (cnt) cnt[q] = c;
}

// Continue (incremental_triangulator.cc:545-586) for the committed problems of a round
__global__ void k_rt_continue(uint32_t R, const uint32_t* __restrict__ run, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ moff,
                              const uint32_t* __restrict__ mem, const int32_t* __restrict__ pid, const double* __restrict__ pxyz,
                              const double* __restrict__ nxyz, const uint32_t* __restrict__ feat_img, const double* __restrict__ img_P,
                              const double* __restrict__ img_C, const double* __restrict__ uv, RtParams prm, int32_t* __restrict__ cont,
                              double* __restrict__ margins) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint32_t q = run[r];
  int32_t target = -1;
  double mg = INFINITY;
  if (pid[ref[q]] < 0) {
    RtView w;
    rt_load(ref[q], feat_img, img_P, img_C, uv, &w);
    double best = DBL_MAX, second = DBL_MAX;
    for (int pass = 0; pass < 2; ++pass)  // the choice (strict <: the first wins ties), then the best error on another point
      for (uint32_t e = moff[q]; e < moff[q + 1]; ++e) {
        const int32_t p = pid[mem[e]];
        if (p < 0 || (pass == 1 && p == target)) continue;
        const double* X = (uint32_t)p < prm.num_points ? &pxyz[3 * (size_t)p] : &nxyz[3 * (size_t)((uint32_t)p - prm.num_points)];
        double cd;
        const double err = sqrt(rt_residual(w, X, &cd));
        if (!(cd <= kRtCosineEdge)) mg = 0.0;
        if (pass == 0 && err < best) {
          best = err;
          target = p;
        } else if (pass == 1 && err < second) {
          second = err;
        }
      }
    if (target >= 0) {
      if (second != DBL_MAX && best > 0.0) mg = fmin(mg, (second - best) / best);
      mg = fmin(mg, fabs(best - prm.continue_max_error) / prm.continue_max_error);
      if (!(best <= prm.continue_max_error)) target = -1;
    }
  }
  cont[q] = target;
  margins[(size_t)q * kRtMargins + 4] = mg;
}

// Create (incremental_triangulator.cc:461-543) with its recursion, for the committed problems of a round.  Per problem slot
// (moff[q] + q, members + 1 entries): clist the create list, assign the depth of the point that takes each entry (-1 none),
// lvl scratch, nxyz the new points by depth.
__global__ void k_rt_create(uint32_t R, const uint32_t* __restrict__ run, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ moff,
                            const uint32_t* __restrict__ mem, const int32_t* __restrict__ pid, const int32_t* __restrict__ cont,
                            const uint32_t* __restrict__ goff, const uint32_t* __restrict__ gval, const uint32_t* __restrict__ feat_img,
                            const double* __restrict__ img_P, const double* __restrict__ img_C, const double* __restrict__ uv,
                            const uint32_t* __restrict__ tab, const uint32_t* __restrict__ tab_off, RtParams prm, int32_t* __restrict__ clist,
                            int32_t* __restrict__ assign, int32_t* __restrict__ lvl, double* __restrict__ nxyz, uint32_t* __restrict__ ncreated,
                            uint32_t* __restrict__ ncl, uint32_t* __restrict__ trials, double* __restrict__ margins) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint32_t q = run[r];
  const size_t slot = (size_t)moff[q] + q;
  int n = 0;
  for (uint32_t e = moff[q]; e < moff[q + 1]; ++e)
    if (pid[mem[e]] < 0) clist[slot + n++] = (int32_t)mem[e];
  if (pid[ref[q]] < 0 && cont[q] < 0) clist[slot + n++] = (int32_t)ref[q];
  ncl[q] = n;
  for (int i = 0; i < n; ++i) assign[slot + i] = -1;
  RtLane L;
  L.feat_img = feat_img, L.img_P = img_P, L.img_C = img_C, L.uv = uv, L.clist = clist + slot, L.idx = lvl + slot, L.prm = prm;
  for (int k = 0; k < 4; ++k) L.mg[k] = INFINITY;
  uint32_t created = 0, tr = 0;
  bool go = n >= 2;
  if (go && prm.ignore_two_view && n == 2) {  // IsTwoViewObservation of the first entry
    const uint32_t f = (uint32_t)clist[slot];
    if (goff[f + 1] - goff[f] == 1) {
      const uint32_t g = gval[goff[f]];
      if (goff[g + 1] - goff[g] == 1) go = false;
    }
  }
  while (go) {
    int m = 0;
    for (int i = 0; i < n; ++i)
      if (assign[slot + i] < 0) lvl[slot + m++] = i;
    L.n = m;
    double X[3];
    if (m < 2 || !rt_loransac(L, tab, tab_off, X, &tr)) break;
    int len = 0;
    for (int i = 0; i < m; ++i) {
      RtView w;
      rt_view(L, i, &w);
      if (rt_residual(w, X) <= prm.max_residual) {
        assign[slot + L.idx[i]] = (int32_t)created;
        ++len;
      }
    }
    nxyz[3 * (slot + created)] = X[0];
    nxyz[3 * (slot + created) + 1] = X[1];
    nxyz[3 * (slot + created) + 2] = X[2];
    ++created;
    go = m - len >= 3;
  }
  ncreated[q] = created;
  trials[q] = tr;
  for (int k = 0; k < 4; ++k) margins[(size_t)q * kRtMargins + k] = L.mg[k];
}

// the committed problems' writes into the feature -> point state (their feature sets are disjoint)
__global__ void k_rt_apply(uint32_t R, const uint32_t* __restrict__ run, const uint32_t* __restrict__ ref, const uint32_t* __restrict__ moff,
                           const int32_t* __restrict__ cont, const int32_t* __restrict__ clist, const int32_t* __restrict__ assign,
                           const uint32_t* __restrict__ ncl, RtParams prm, int32_t* __restrict__ pid) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const uint32_t q = run[r];
  const size_t slot = (size_t)moff[q] + q;
  if (cont[q] >= 0) pid[ref[q]] = cont[q];
  for (uint32_t i = 0; i < ncl[q]; ++i)
    if (assign[slot + i] >= 0) pid[clist[slot + i]] = (int32_t)(prm.num_points + slot + (uint32_t)assign[slot + i]);
}

struct RtBufs {
  DevBuf pair_img, moff, matches, nfeat, foff, acc, epair, val2, goff, scan_s[4], scan_x[4];
  DevBuf cnt, feat_img, img_ok, img_cam, cams, xy, uv, img_P, img_C, pid, pxyz;
  DevBuf ref, pmoff, mem, pcnt, run, cont, clist, assign, lvl, nxyz, ncreated, ncl, trials, margins, tab, tab_off;
};

// goff[0 .. n) = exclusive scan of d.cnt[0 .. n) in fixed blocks: level l scans the block totals of level l - 1
hipError_t rt_scan(RtBufs& d, uint32_t n, hipStream_t st) {
  const uint32_t B = RT_BLOCK * 4;
  hipError_t e = d.goff.reserve((size_t)n * 4 + 16);
  std::vector<uint32_t> lens{n};
  while (lens.back() > B) lens.push_back((lens.back() + B - 1) / B);
  if (lens.size() > 4) return hipErrorInvalidValue;
  for (size_t l = 0; l < lens.size() && e == hipSuccess; ++l) {
    e = d.scan_s[l].reserve(((size_t)(lens[l] + B - 1) / B) * 4 + 16);
    if (e == hipSuccess) e = d.scan_x[l].reserve((size_t)lens[l] * 4 + 16);
  }
  if (e != hipSuccess) return e;
  std::vector<uint32_t*> outs;
  const uint32_t* in = d.cnt.as<uint32_t>();
  for (size_t l = 0; l < lens.size(); ++l) {
    uint32_t* out = l == 0 ? d.goff.as<uint32_t>() : d.scan_x[l].as<uint32_t>();
    hipLaunchKernelGGL(k_rt_scan_block, dim3((lens[l] + B - 1) / B), dim3(RT_BLOCK), 0, st, lens[l], in, out, d.scan_s[l].as<uint32_t>());
    outs.push_back(out);
    in = d.scan_s[l].as<uint32_t>();
  }
  for (size_t l = outs.size(); l-- > 1;)
    hipLaunchKernelGGL(k_rt_scan_add, dim3((lens[l - 1] + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, lens[l - 1], outs[l - 1], outs[l]);
  return hipGetLastError();
}

// the message of the first option out of range, or NULL
const char* rt_options_error(const dsm_triangulation_options& o) {
  if (o.max_transitivity != 1) return "max_transitivity other than 1 is not supported";
  if (!(o.create_max_angle_error > 0) || !(o.continue_max_angle_error >= 0) || !(o.min_angle > 0) || !(o.min_focal_length_ratio > 0) ||
      !(o.max_focal_length_ratio >= o.min_focal_length_ratio) || !(o.max_extra_param >= 0) || !(o.ransac_confidence > 0 && o.ransac_confidence < 1) ||
      !(o.ransac_min_inlier_ratio >= 0 && o.ransac_min_inlier_ratio <= 1) || o.ransac_max_num_trials < 1 || !std::isfinite(o.max_focal_length_ratio) ||
      !std::isfinite(o.create_max_angle_error) || !std::isfinite(o.continue_max_angle_error) || !std::isfinite(o.min_angle) ||
      !std::isfinite(o.max_extra_param))
    return "option out of range";
  return nullptr;
}

// The scene of a re-triangulation call, validated and in the canonical image order (ascending image id): what both entry
// points read.  rt_load_scene returns the message of the first invalid argument, or an empty string.
struct RtScene {
  std::vector<uint32_t> order;  // canonical index -> input index
  std::vector<uint32_t> nfeat, foff, img_cam, feat_img, pair_img;
  std::vector<uint8_t> cam_bogus, img_ok;
  std::vector<double> img_P, img_C, xy;
  std::vector<int32_t> pid0;
  uint64_t F = 0, NM = 0, next_id = 0;
  int64_t find_img(const uint32_t* image_ids, uint32_t id) const {
    auto it = std::lower_bound(order.begin(), order.end(), id, [&](uint32_t a, uint32_t v) { return image_ids[a] < v; });
    return (it != order.end() && image_ids[*it] == id) ? (int64_t)(it - order.begin()) : -1;
  }
};

std::string rt_load_scene(RtScene& S, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                          const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint8_t* image_registered,
                          const double* image_qvec, const double* image_tvec, const uint32_t* points2D_offsets, const double* points2D_xy,
                          const int32_t* points2D_point3D, uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz,
                          uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                          uint64_t next_point3D_id, const dsm_triangulation_options& o, double* bogus_margin) {
  std::vector<uint32_t> cam_order(num_cameras);
  std::iota(cam_order.begin(), cam_order.end(), 0u);
  std::sort(cam_order.begin(), cam_order.end(), [&](uint32_t a, uint32_t b) { return camera_ids[a] < camera_ids[b]; });
  for (uint32_t i = 1; i < num_cameras; ++i)
    if (camera_ids[cam_order[i]] == camera_ids[cam_order[i - 1]]) return "a repeated camera id";
  std::vector<uint8_t> cam_bogus(num_cameras);
  for (uint32_t c = 0; c < num_cameras; ++c) {
    const dsm_camera& k = cameras[c];
    if (!cam_model_exists(k.model_id)) return "an unknown camera model";
    for (int i = 0; i < cam_num_params(k.model_id); ++i)
      if (!std::isfinite(k.params[i])) return "non-finite camera parameters";
    cam_bogus[c] = cam_has_bogus_params(k, o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param, bogus_margin);
  }
  auto find_cam = [&](uint32_t id) -> int64_t {
    auto it = std::lower_bound(cam_order.begin(), cam_order.end(), id, [&](uint32_t a, uint32_t v) { return camera_ids[a] < v; });
    return (it != cam_order.end() && camera_ids[*it] == id) ? (int64_t)*it : -1;
  };
  if (points2D_offsets[0] != 0) return "points2D offsets must start at 0";
  std::vector<uint32_t>& order = S.order;  // canonical index -> input index
  order.resize(num_images);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return image_ids[a] < image_ids[b]; });
  for (uint32_t i = 1; i < num_images; ++i)
    if (image_ids[order[i]] == image_ids[order[i - 1]]) return "a repeated image id";
  std::vector<uint32_t> canon(num_images);  // input index -> canonical index
  for (uint32_t i = 0; i < num_images; ++i) canon[order[i]] = i;
  std::vector<uint32_t> nfeat(num_images), foff(num_images + 1, 0), img_cam(num_images);
  std::vector<uint8_t> img_ok(num_images);
  std::vector<double> img_P(12 * (size_t)num_images), img_C(3 * (size_t)num_images);
  for (uint32_t i = 0; i < num_images; ++i) {
    if (points2D_offsets[i + 1] < points2D_offsets[i]) return "points2D offsets must be non-decreasing";
    if (points2D_offsets[i + 1] - points2D_offsets[i] > kRtMaxPoints2D) return "more than 262144 points2D in one image";
  }
  const uint64_t F = points2D_offsets[num_images];
  if (F >= 0x40000000u) return "too many points2D";
  if (F && (!points2D_xy || !points2D_point3D)) return "NULL argument";
  for (uint32_t c = 0; c < num_images; ++c) {
    const uint32_t i = order[c];
    nfeat[c] = points2D_offsets[i + 1] - points2D_offsets[i];
    foff[c + 1] = foff[c] + nfeat[c];
    const int64_t cam = find_cam(image_camera_ids[i]);
    if (cam < 0) return "an image on an unknown camera id";
    img_cam[c] = (uint32_t)cam;
    img_ok[c] = image_registered[i] && !cam_bogus[cam];
    const double* qv = image_qvec + 4 * (size_t)i;
    const double* tv = image_tvec + 3 * (size_t)i;
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(qv[k])) return "non-finite qvec";
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(tv[k])) return "non-finite tvec";
    // NormalizeQuaternion + Eigen's toRotationMatrix (pose.cc:75-91), ProjectionCenterFromPose as -R^T t
    const double nq = std::sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
    if (nq == 0) return "a zero qvec";
    const double w = qv[0] / nq, x = qv[1] / nq, y = qv[2] / nq, z = qv[3] / nq;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double Rm[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    double* P = &img_P[12 * (size_t)c];
    for (int r = 0; r < 3; ++r) {
      for (int k = 0; k < 3; ++k) P[4 * r + k] = Rm[3 * r + k];
      P[4 * r + 3] = tv[r];
    }
    for (int k = 0; k < 3; ++k) img_C[3 * (size_t)c + k] = -((Rm[k] * tv[0] + Rm[3 + k] * tv[1]) + Rm[6 + k] * tv[2]);
  }
  // points3D: internal index = input index; ids unique
  std::vector<uint64_t> sorted_ids(point3D_ids, point3D_ids + num_points3D);
  std::sort(sorted_ids.begin(), sorted_ids.end());
  for (uint32_t i = 1; i < num_points3D; ++i)
    if (sorted_ids[i] == sorted_ids[i - 1]) return "a repeated point3D id";
  for (size_t i = 0; i < 3 * (size_t)num_points3D; ++i)
    if (!std::isfinite(point3D_xyz[i])) return "non-finite point3D xyz";
  const uint64_t max_id = num_points3D ? sorted_ids.back() : 0;
  uint64_t next_id = next_point3D_id ? next_point3D_id : max_id + 1;
  if (num_points3D && next_id <= max_id) return "next_point3D_id at or below an existing id";
  if (num_points3D >= 0x40000000u) return "too many points3D";
  std::vector<double> xy(2 * F);
  std::vector<int32_t> pid0(F);
  std::vector<uint32_t> feat_img(F);
  for (uint32_t c = 0; c < num_images; ++c) {
    const uint32_t i = order[c];
    for (uint32_t k = 0; k < nfeat[c]; ++k) {
      const size_t s = (size_t)points2D_offsets[i] + k, d = (size_t)foff[c] + k;
      xy[2 * d] = points2D_xy[2 * s];
      xy[2 * d + 1] = points2D_xy[2 * s + 1];
      if (!std::isfinite(xy[2 * d]) || !std::isfinite(xy[2 * d + 1])) return "non-finite points2D xy";
      const int32_t p = points2D_point3D[s];
      if (p < -1 || p >= (int64_t)num_points3D) return "a point3D index out of range";
      pid0[d] = p;
      feat_img[d] = c;
    }
  }
  if (match_offsets[0] != 0) return "match offsets must start at 0";
  std::vector<uint32_t> pair_img(2 * (size_t)num_pairs);
  std::vector<uint64_t> pair_keys(num_pairs);
  for (uint32_t k = 0; k < num_pairs; ++k) {
    if (match_offsets[k + 1] < match_offsets[k]) return "match offsets must be non-decreasing";
    const int64_t a = S.find_img(image_ids, pair_image_ids[2 * k]), b = S.find_img(image_ids, pair_image_ids[2 * k + 1]);
    if (a < 0 || b < 0) return "a pair on an unknown image id";
    if (a == b) return "a self-pair";
    pair_img[2 * k] = (uint32_t)a;
    pair_img[2 * k + 1] = (uint32_t)b;
    pair_keys[k] = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
    for (uint64_t m = match_offsets[k]; m < match_offsets[k + 1]; ++m)
      if (matches[2 * m] >= nfeat[a] || matches[2 * m + 1] >= nfeat[b]) return "a match index out of range";
  }
  std::sort(pair_keys.begin(), pair_keys.end());
  for (uint32_t k = 1; k < num_pairs; ++k)
    if (pair_keys[k] == pair_keys[k - 1]) return "a repeated pair";
  const uint64_t NM = match_offsets[num_pairs];
  if (NM >= 0x20000000u) return "too many matches";
  S.nfeat = std::move(nfeat), S.foff = std::move(foff), S.img_cam = std::move(img_cam), S.feat_img = std::move(feat_img);
  S.pair_img = std::move(pair_img), S.cam_bogus = std::move(cam_bogus), S.img_ok = std::move(img_ok);
  S.img_P = std::move(img_P), S.img_C = std::move(img_C), S.xy = std::move(xy), S.pid0 = std::move(pid0);
  S.F = F, S.NM = NM, S.next_id = next_id;
  return std::string();
}

}  // namespace

extern "C" void dsm_default_triangulation_options(dsm_triangulation_options* o) {
  o->create_max_angle_error = 2.0;    // IncrementalTriangulator::Options (incremental_triangulator.h)
  o->continue_max_angle_error = 2.0;
  o->min_angle = 1.5;
  o->min_focal_length_ratio = 0.1;
  o->max_focal_length_ratio = 10.0;
  o->max_extra_param = 1.0;
  o->ransac_confidence = 0.9999;      // Create(), incremental_triangulator.cc:505-508
  o->ransac_min_inlier_ratio = 0.02;
  o->ransac_max_num_trials = 10000;
  o->ignore_two_view_tracks = 1;
  o->max_transitivity = 1;
  o->reserved = 0;
}

extern "C" int dsm_retriangulate(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                 uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                 const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                                 const uint32_t* points2D_offsets, const double* points2D_xy, const int32_t* points2D_point3D,
                                 uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, uint32_t num_pairs,
                                 const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                 uint32_t num_separators, const uint32_t* separator_ids, uint64_t next_point3D_id,
                                 const dsm_triangulation_options* options, uint64_t* new_point_ids, double* new_point_xyz,
                                 uint64_t* new_track_offsets, uint32_t* new_track_obs, uint64_t* n_new_points,
                                 uint32_t* continued_obs, uint64_t* continued_point_ids, uint64_t* n_continued, uint32_t* touched_obs,
                                 uint64_t* touched_point_ids, uint64_t* n_touched, uint32_t* num_tris_per_separator,
                                 uint64_t* num_tris_out, dsm_triangulation_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_retriangulate", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  if ((num_cameras && (!camera_ids || !cameras)) || (num_images && (!image_ids || !image_camera_ids || !image_registered || !image_qvec ||
                                                                     !image_tvec)) ||
      !points2D_offsets || (num_points3D && (!point3D_ids || !point3D_xyz)) || (num_pairs && (!pair_image_ids || !matches)) ||
      !match_offsets || (num_separators && (!separator_ids || !num_tris_per_separator)) || !n_new_points || !n_continued || !n_touched ||
      !num_tris_out)
    return fail("NULL argument");
  dsm_triangulation_options o;
  if (options)
    o = *options;
  else
    dsm_default_triangulation_options(&o);
  if (const char* msg = rt_options_error(o)) return fail(msg);
  dsm_triangulation_report rep{};
  rep.min_residual_margin = rep.min_support_margin = rep.min_angle_margin = rep.min_depth_margin = rep.min_continue_margin =
      rep.min_bogus_margin = INFINITY;

  // ------------------------------------------------------------ validation and the canonical image order (host)
  RtScene scn;
  {
    const std::string msg = rt_load_scene(scn, num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, image_registered,
                                          image_qvec, image_tvec, points2D_offsets, points2D_xy, points2D_point3D, num_points3D, point3D_ids,
                                          point3D_xyz, num_pairs, pair_image_ids, match_offsets, matches, next_point3D_id, o,
                                          &rep.min_bogus_margin);
    if (!msg.empty()) return fail(msg.c_str());
  }
  const std::vector<uint32_t>&order = scn.order, &nfeat = scn.nfeat, &foff = scn.foff, &img_cam = scn.img_cam, &feat_img = scn.feat_img,
                             &pair_img = scn.pair_img;
  const std::vector<uint8_t>& img_ok = scn.img_ok;
  const std::vector<double>&img_P = scn.img_P, &img_C = scn.img_C, &xy = scn.xy;
  const std::vector<int32_t>& pid0 = scn.pid0;
  const uint64_t F = scn.F, NM = scn.NM, next_id = scn.next_id;
  auto find_img = [&](uint32_t id) { return scn.find_img(image_ids, id); };
  std::vector<uint32_t> sep(num_separators);
  for (uint32_t s = 0; s < num_separators; ++s) {
    const int64_t c = find_img(separator_ids[s]);
    if (c < 0) return fail("a separator on an unknown image id");
    sep[s] = (uint32_t)c;
  }
  std::vector<uint32_t> sep_order(num_separators);  // ascending image id = ascending canonical index
  std::iota(sep_order.begin(), sep_order.end(), 0u);
  std::sort(sep_order.begin(), sep_order.end(), [&](uint32_t a, uint32_t b) { return sep[a] < sep[b]; });
  for (uint32_t s = 1; s < num_separators; ++s)
    if (sep[sep_order[s]] == sep[sep_order[s - 1]]) return fail("a repeated separator id");

  // candidates: (separator ascending, point2D) of the usable separators
  std::vector<uint32_t> cand, cand_sep;
  for (uint32_t s : sep_order) {
    const uint32_t c = sep[s];
    if (!img_ok[c]) continue;
    ++rep.num_separators;
    for (uint32_t k = 0; k < nfeat[c]; ++k) {
      cand.push_back(foff[c] + k);
      cand_sep.push_back(s);
    }
  }
  const double setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  RtBufs d;
  DevEvents<5> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  const size_t F1 = std::max<uint64_t>(F, 1);

  // ------------------------------------------------------------ the correspondence graph (device)
  HIPCHK(ctx, dev_upload(d.nfeat, nfeat.data(), nfeat.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.foff, foff.data(), foff.size() * 4, st));
  HIPCHK(ctx, d.goff.reserve((F1 + 1) * 4));
  uint32_t E = 0;
  HIPCHK(ctx, d.cnt.reserve((F1 + 1) * 4));
  HIPCHK(ctx, hipMemsetAsync(d.cnt.p, 0, (F1 + 1) * 4, st));
  if (NM) {
    HIPCHK(ctx, dev_upload(d.pair_img, pair_img.data(), pair_img.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.moff, match_offsets, ((size_t)num_pairs + 1) * 8, st));
    HIPCHK(ctx, dev_upload(d.matches, matches, NM * 8, st));
    HIPCHK(ctx, d.acc.reserve(NM));
    hipLaunchKernelGGL(k_rt_dedup, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.nfeat.as<uint32_t>(), d.acc.as<uint8_t>());
    hipLaunchKernelGGL(k_rt_count, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.acc.as<uint8_t>(), d.foff.as<uint32_t>(), d.cnt.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, rt_scan(d, (uint32_t)F + 1, st));  // goff = exclusive scan of the counts (F + 1 entries: the last is E)
  HIPCHK(ctx, hipMemcpyAsync(&E, d.goff.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (DevBuf* b : {&d.epair, &d.val2}) HIPCHK(ctx, b->reserve(std::max<size_t>((size_t)E * 4, 16)));
  if (E) {
    HIPCHK(ctx, hipMemsetAsync(d.cnt.p, 0, F1 * 4, st));  // reused as the fill counters
    hipLaunchKernelGGL(k_rt_emit, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.acc.as<uint8_t>(), d.foff.as<uint32_t>(), d.goff.as<uint32_t>(), d.cnt.as<uint32_t>(),
                       d.epair.as<uint32_t>(), d.val2.as<uint32_t>());
    hipLaunchKernelGGL(k_rt_segsort, dim3((uint32_t)((F + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, st, (uint32_t)F, d.goff.as<uint32_t>(),
                       d.epair.as<uint32_t>(), d.val2.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  rep.num_correspondences = E;
  HIPCHK(ctx, hipEventRecord(ev[1], st));

  // ------------------------------------------------------------ the problems: Find on the device, non-empty ones kept
  std::vector<dsm_camera> cams(cameras, cameras + num_cameras);
  HIPCHK(ctx, dev_upload(d.feat_img, feat_img.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(d.img_ok, img_ok.data(), num_images, st));
  HIPCHK(ctx, dev_upload(d.img_cam, img_cam.data(), num_images * 4, st));
  HIPCHK(ctx, dev_upload(d.cams, cams.data(), cams.size() * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.xy, xy.data(), F * 16, st));
  HIPCHK(ctx, d.uv.reserve(F1 * 16));
  HIPCHK(ctx, dev_upload(d.img_P, img_P.data(), img_P.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.img_C, img_C.data(), img_C.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.pid, pid0.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(d.pxyz, point3D_xyz, (size_t)num_points3D * 24, st));
  if (F)
    hipLaunchKernelGGL(k_rt_normalize, dim3((uint32_t)((F + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, st, (uint32_t)F, d.feat_img.as<uint32_t>(),
                       d.img_ok.as<uint8_t>(), d.img_cam.as<uint32_t>(), d.cams.as<dsm_camera>(), d.xy.as<double>(), d.uv.as<double>());
  const uint32_t Q0 = (uint32_t)cand.size();
  std::vector<uint32_t> cnt(Q0);
  if (Q0) {
    HIPCHK(ctx, dev_upload(d.ref, cand.data(), (size_t)Q0 * 4, st));
    HIPCHK(ctx, d.pcnt.reserve((size_t)Q0 * 4));
    hipLaunchKernelGGL(k_rt_find, dim3((Q0 + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, Q0, d.ref.as<uint32_t>(), d.goff.as<uint32_t>(),
                       d.val2.as<uint32_t>(), d.feat_img.as<uint32_t>(), d.img_ok.as<uint8_t>(), (const uint32_t*)nullptr, d.pcnt.as<uint32_t>(),
                       (uint32_t*)nullptr);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(cnt.data(), d.pcnt.p, (size_t)Q0 * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  std::vector<uint32_t> pref, psep, pmoff(1, 0);
  for (uint32_t q = 0; q < Q0; ++q)
    if (cnt[q]) {
      pref.push_back(cand[q]);
      psep.push_back(cand_sep[q]);
      pmoff.push_back(pmoff.back() + cnt[q]);
    }
  const uint32_t Q = (uint32_t)pref.size();
  const uint64_t M = pmoff.back();
  const uint64_t S = M + Q;  // problem slots: members + 1 each
  if (S >= 0x40000000u) return fail("too many correspondences in the separator images");
  rep.num_problems = Q;
  std::vector<uint32_t> mem(M);
  uint32_t maxn = 2;
  for (uint32_t q = 0; q < Q; ++q) maxn = std::max(maxn, pmoff[q + 1] - pmoff[q] + 1);
  if (Q) {
    HIPCHK(ctx, dev_upload(d.ref, pref.data(), (size_t)Q * 4, st));
    HIPCHK(ctx, dev_upload(d.pmoff, pmoff.data(), ((size_t)Q + 1) * 4, st));
    HIPCHK(ctx, d.mem.reserve(std::max<size_t>(M * 4, 16)));
    hipLaunchKernelGGL(k_rt_find, dim3((Q + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, Q, d.ref.as<uint32_t>(), d.goff.as<uint32_t>(),
                       d.val2.as<uint32_t>(), d.feat_img.as<uint32_t>(), d.img_ok.as<uint8_t>(), d.pmoff.as<uint32_t>(), (uint32_t*)nullptr,
                       d.mem.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(mem.data(), d.mem.p, M * 4, hipMemcpyDeviceToHost, st));
  }
  // ComputeNumTrials for n <= maxn (the host's libm)
  std::vector<uint32_t> tab_off(maxn + 1, 0), tab;
  for (uint32_t n = 2; n <= maxn; ++n) {
    tab_off[n] = (uint32_t)tab.size();
    for (uint32_t k = 0; k <= n; ++k) tab.push_back(rt_num_trials(k, n, o.ransac_confidence));
  }
  HIPCHK(ctx, dev_upload(d.tab, tab.data(), tab.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.tab_off, tab_off.data(), tab_off.size() * 4, st));
  const size_t Q1 = std::max<uint32_t>(Q, 1), S1 = std::max<uint64_t>(S, 1);
  for (DevBuf* b : {&d.cont, &d.ncreated, &d.ncl, &d.trials, &d.run}) HIPCHK(ctx, b->reserve(Q1 * 4));
  HIPCHK(ctx, d.margins.reserve(Q1 * kRtMargins * 8));
  for (DevBuf* b : {&d.clist, &d.assign, &d.lvl}) HIPCHK(ctx, b->reserve(S1 * 4));
  HIPCHK(ctx, d.nxyz.reserve(S1 * 24));
  HIPCHK(ctx, hipStreamSynchronize(st));

  // ------------------------------------------------------------ the rounds (schedule on the host, solves on the device)
  // A problem is pending in round r while an earlier problem that shares a feature with it is pending in round r, so its
  // round is 1 + the largest round of those problems: one pass in problem order with the largest round seen per feature.
  const auto t_rep0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> last(F1, 0), qround(Q);
  uint32_t nrounds = 0;
  for (uint32_t q = 0; q < Q; ++q) {
    uint32_t r = last[pref[q]];
    for (uint32_t e = pmoff[q]; e < pmoff[q + 1]; ++e) r = std::max(r, last[mem[e]]);
    ++r;
    qround[q] = r;
    last[pref[q]] = r;
    for (uint32_t e = pmoff[q]; e < pmoff[q + 1]; ++e) last[mem[e]] = r;
    nrounds = std::max(nrounds, r);
    rep.num_deferred += r - 1;
  }
  std::vector<uint32_t> roff(nrounds + 2, 0), run(Q);  // problems by (round, problem order): a counting sort
  for (uint32_t q = 0; q < Q; ++q) ++roff[qround[q] + 1];
  for (uint32_t r = 1; r <= nrounds + 1; ++r) roff[r] += roff[r - 1];
  {
    std::vector<uint32_t> fillp(roff.begin(), roff.end() - 1);
    for (uint32_t q = 0; q < Q; ++q) run[fillp[qround[q]]++] = q;
  }
  rep.num_rounds = nrounds;
  rep.schedule_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_rep0).count();
  RtParams prm;
  prm.max_residual = (o.create_max_angle_error * kRtDegToRad) * (o.create_max_angle_error * kRtDegToRad);
  prm.min_tri_angle = o.min_angle * kRtDegToRad;
  prm.continue_max_error = o.continue_max_angle_error * kRtDegToRad;
  prm.ignore_two_view = o.ignore_two_view_tracks ? 1 : 0;
  prm.max_trials = o.ransac_max_num_trials;
  prm.tab_n = maxn;
  prm.num_points = num_points3D;
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  if (Q) HIPCHK(ctx, hipMemcpyAsync(d.run.p, run.data(), (size_t)Q * 4, hipMemcpyHostToDevice, st));
  DevEventList rev(4 * (size_t)nrounds);  // per round: before Continue, Create, apply, after apply
  HIPCHK(ctx, rev.create());
  const double* nx = d.nxyz.as<double>();
  for (uint32_t r = 1; r <= nrounds; ++r) {  // every round enqueued back to back: the schedule needs no result
    const uint32_t R = roff[r + 1] - roff[r];
    const uint32_t* rl = d.run.as<uint32_t>() + roff[r];
    const dim3 g((R + RT_BLOCK - 1) / RT_BLOCK);
    DevEvent* re = &rev[4 * (size_t)(r - 1)];
    HIPCHK(ctx, hipEventRecord(re[0], st));
    hipLaunchKernelGGL(k_rt_continue, g, dim3(RT_BLOCK), 0, st, R, rl, d.ref.as<uint32_t>(), d.pmoff.as<uint32_t>(),
                       d.mem.as<uint32_t>(), d.pid.as<int32_t>(), d.pxyz.as<double>(), nx, d.feat_img.as<uint32_t>(), d.img_P.as<double>(),
                       d.img_C.as<double>(), d.uv.as<double>(), prm, d.cont.as<int32_t>(), d.margins.as<double>());
    HIPCHK(ctx, hipEventRecord(re[1], st));
    hipLaunchKernelGGL(k_rt_create, g, dim3(RT_BLOCK), 0, st, R, rl, d.ref.as<uint32_t>(), d.pmoff.as<uint32_t>(),
                       d.mem.as<uint32_t>(), d.pid.as<int32_t>(), d.cont.as<int32_t>(), d.goff.as<uint32_t>(), d.val2.as<uint32_t>(),
                       d.feat_img.as<uint32_t>(), d.img_P.as<double>(), d.img_C.as<double>(), d.uv.as<double>(), d.tab.as<uint32_t>(),
                       d.tab_off.as<uint32_t>(), prm, d.clist.as<int32_t>(), d.assign.as<int32_t>(), d.lvl.as<int32_t>(), d.nxyz.as<double>(),
                       d.ncreated.as<uint32_t>(), d.ncl.as<uint32_t>(), d.trials.as<uint32_t>(), d.margins.as<double>());
    HIPCHK(ctx, hipEventRecord(re[2], st));
    hipLaunchKernelGGL(k_rt_apply, g, dim3(RT_BLOCK), 0, st, R, rl, d.ref.as<uint32_t>(), d.pmoff.as<uint32_t>(),
                       d.cont.as<int32_t>(), d.clist.as<int32_t>(), d.assign.as<int32_t>(), d.ncl.as<uint32_t>(), prm, d.pid.as<int32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(re[3], st));
  }
  HIPCHK(ctx, hipEventRecord(ev[3], st));

  // ------------------------------------------------------------ results back, new ids in (separator, point2D, depth) order
  std::vector<int32_t> cont(Q), clist(S), assign(S);
  std::vector<uint32_t> ncreated(Q), ncl(Q), trials(Q);
  std::vector<double> nxyz(3 * S), margins((size_t)Q * kRtMargins);
  if (Q) {
    HIPCHK(ctx, hipMemcpyAsync(cont.data(), d.cont.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ncreated.data(), d.ncreated.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(ncl.data(), d.ncl.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(trials.data(), d.trials.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(margins.data(), d.margins.p, margins.size() * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(clist.data(), d.clist.p, S * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(assign.data(), d.assign.p, S * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(nxyz.data(), d.nxyz.p, S * 24, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(ctx, hipEventRecord(ev[4], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const auto t_out0 = std::chrono::steady_clock::now();
  std::vector<uint64_t> slot_id(S, 0);  // slot -> final id of the point created there
  uint64_t nnew = 0, nobs = 0;
  for (uint32_t q = 0; q < Q; ++q) {
    const size_t slot = (size_t)pmoff[q] + q;
    for (uint32_t k = 0; k < ncreated[q]; ++k) slot_id[slot + k] = next_id + nnew++;
  }
  auto final_id = [&](int32_t p) -> uint64_t {
    return (uint32_t)p < num_points3D ? point3D_ids[p] : slot_id[(uint32_t)p - num_points3D];
  };
  std::vector<uint64_t> touched_id(F, UINT64_MAX);
  std::vector<uint64_t> sep_tris(num_separators, 0);
  uint64_t ncont = 0, pnew = 0, tris = 0;
  if (new_track_offsets) new_track_offsets[0] = 0;
  for (uint32_t q = 0; q < Q; ++q) {
    const size_t slot = (size_t)pmoff[q] + q;
    uint64_t t = 0;
    if (cont[q] >= 0) {
      const uint64_t id = final_id(cont[q]);
      const uint32_t f = pref[q], c = feat_img[f];
      if (continued_obs) {
        continued_obs[2 * ncont] = image_ids[order[c]];
        continued_obs[2 * ncont + 1] = f - foff[c];
      }
      if (continued_point_ids) continued_point_ids[ncont] = id;
      ++ncont;
      touched_id[f] = id;
      ++t;
    }
    for (uint32_t k = 0; k < ncreated[q]; ++k) {
      const uint64_t id = slot_id[slot + k];
      if (new_point_ids) new_point_ids[pnew] = id;
      if (new_point_xyz)
        for (int j = 0; j < 3; ++j) new_point_xyz[3 * pnew + j] = nxyz[3 * (slot + k) + j];
      for (uint32_t i = 0; i < ncl[q]; ++i)
        if (assign[slot + i] == (int32_t)k) {
          const uint32_t f = (uint32_t)clist[slot + i], c = feat_img[f];
          if (new_track_obs) {
            new_track_obs[2 * nobs] = image_ids[order[c]];
            new_track_obs[2 * nobs + 1] = f - foff[c];
          }
          ++nobs;
          ++t;
          touched_id[f] = id;
        }
      ++pnew;
      if (new_track_offsets) new_track_offsets[pnew] = nobs;
    }
    sep_tris[psep[q]] += t;
    tris += t;
    rep.ransac_trials += trials[q];
    const double* mg = &margins[(size_t)q * kRtMargins];
    rep.min_residual_margin = std::min(rep.min_residual_margin, mg[0]);
    rep.min_support_margin = std::min(rep.min_support_margin, mg[1]);
    rep.min_angle_margin = std::min(rep.min_angle_margin, mg[2]);
    rep.min_depth_margin = std::min(rep.min_depth_margin, mg[3]);
    rep.min_continue_margin = std::min(rep.min_continue_margin, mg[4]);
  }
  uint64_t nt = 0;
  for (uint64_t f = 0; f < F; ++f)
    if (touched_id[f] != UINT64_MAX) {
      const uint32_t c = feat_img[f];
      if (touched_obs) {
        touched_obs[2 * nt] = image_ids[order[c]];
        touched_obs[2 * nt + 1] = (uint32_t)(f - foff[c]);
      }
      if (touched_point_ids) touched_point_ids[nt] = touched_id[f];
      ++nt;
    }
  for (uint32_t s = 0; s < num_separators; ++s) num_tris_per_separator[s] = (uint32_t)sep_tris[s];
  *n_new_points = pnew;
  *n_continued = ncont;
  *n_touched = nt;
  *num_tris_out = tris;
  rep.num_tris = tris;
  rep.num_new_points = pnew;
  rep.num_new_observations = nobs;
  rep.num_continued = ncont;
  double g_ms = 0, solve_ms = 0, dl_ms = 0, tot_ms = 0;
  HIPCHK(ctx, ev.ms(0, 1, &g_ms));
  HIPCHK(ctx, ev.ms(2, 3, &solve_ms));
  HIPCHK(ctx, ev.ms(3, 4, &dl_ms));
  HIPCHK(ctx, ev.ms(0, 4, &tot_ms));
  double cont_ms = 0, create_ms = 0, apply_ms = 0;
  for (uint32_t r = 0; r < nrounds; ++r) {
    double a = 0, b = 0, c = 0;
    HIPCHK(ctx, rev.ms(4 * r, 4 * r + 1, &a));
    HIPCHK(ctx, rev.ms(4 * r + 1, 4 * r + 2, &b));
    HIPCHK(ctx, rev.ms(4 * r + 2, 4 * r + 3, &c));
    cont_ms += a;
    create_ms += b;
    apply_ms += c;
  }
  rep.setup_ms = setup_ms;
  rep.graph_ms = g_ms;
  rep.continue_ms = cont_ms;
  rep.ransac_ms = create_ms;
  rep.apply_ms = apply_ms;
  rep.round_gap_ms = std::max(0.0, (double)solve_ms - cont_ms - create_ms - apply_ms);
  rep.download_ms = dl_ms;
  rep.assemble_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_out0).count();
  rep.replay_ms = rep.schedule_ms + rep.apply_ms + rep.round_gap_ms + rep.assemble_ms;
  rep.device_ms = tot_ms;
  if (report) *report = rep;
  return DSM_OK;
}

// ================================================================== re-triangulation of under-reconstructed pairs
//   IncrementalTriangulator::Retriangulate                          src/sfm/incremental_triangulator.cc:289-390
//   CorrespondenceGraph::FindCorrespondencesBetweenImages           src/base/correspondence_graph.cc:223-248
//   Reconstruction::SetObservationAsTriangulated (num_tri_corrs)    src/base/reconstruction.cc:2018-2050
// The unit of work is a (pair, kept correspondence).  The duplicate rule and the per-feature correspondence counts are the
// kernels above; a pair's kept matches are then ranked by the point2D index of image1 (an LDS bitmap of image1's features and
// its prefix popcounts) and placed into one correspondence list in sequential (pair, correspondence) order.  A pair is open
// while tri / total < re_min_ratio; the ratio never falls during the call, so the pairs open on the input state (and
// registered, with trials left) are a candidate set known before any solve.  Inside a candidate pair no two correspondences
// share a feature, and its gate reads exactly the features its correspondences read and write, so the host schedules whole
// pairs: round(P) = 1 + the largest round of an earlier candidate pair sharing a feature with P.  Per round, back to back:
// k_rp_gate recounts the round's pairs from the current state and takes the ratio test; k_rp_solve runs one lane per
// (pair of the round, kept correspondence), returns for a closed pair, and otherwise writes the feature -> point state and the
// new point's slot directly.  New points carry their correspondence's slot until the host numbers them at the end.
namespace {

constexpr int kRpMargins = 4;  // residual, angle, depth, continue
constexpr uint32_t kRpBitWords = kRtMaxPoints2D / 32;
constexpr uint32_t kRpTimedRounds = 1024;  // a call of more rounds records no events per round
enum : uint8_t { RC_BOTH = 0, RC_CONTINUE_REJECTED, RC_CONTINUED_1, RC_CONTINUED_2, RC_TWO_VIEW, RC_CREATE_FAILED, RC_CREATED, RC_NOT_RUN = 255 };

// the kept matches of a pair counted, and each ranked by its point2D index in image1 (the image with the smaller id)
__global__ void k_rp_rank(uint32_t n_pairs, const uint32_t* __restrict__ pair_img, const uint64_t* __restrict__ moff,
                          const uint32_t* __restrict__ matches, const uint32_t* __restrict__ img_nfeat, const uint8_t* __restrict__ acc,
                          uint32_t* __restrict__ total, uint32_t* __restrict__ rank) {
  __shared__ uint32_t bits[kRpBitWords];
  __shared__ uint32_t chunk[RT_BLOCK];  // prefix popcount of every run of kRpBitWords / RT_BLOCK words
  constexpr uint32_t kRun = kRpBitWords / RT_BLOCK;
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  const uint32_t a = pair_img[2 * k], b = pair_img[2 * k + 1];
  const uint32_t col = a < b ? 0u : 1u;
  const uint32_t words = (img_nfeat[col ? b : a] + 31) / 32;
  for (uint32_t w = threadIdx.x; w < words; w += blockDim.x) bits[w] = 0u;
  __syncthreads();
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x)
    if (acc[m]) {
      const uint32_t i = matches[2 * m + col];
      atomicOr(&bits[i >> 5], 1u << (i & 31));
    }
  __syncthreads();
  uint32_t t = 0;
  for (uint32_t w = threadIdx.x * kRun; w < (threadIdx.x + 1) * kRun && w < words; ++w) t += __popc(bits[w]);
  chunk[threadIdx.x] = t;
  __syncthreads();
  for (int d = 1; d < RT_BLOCK; d *= 2) {
    const uint32_t x = threadIdx.x >= (uint32_t)d ? chunk[threadIdx.x - d] : 0u;
    __syncthreads();
    chunk[threadIdx.x] += x;
    __syncthreads();
  }
  const uint32_t before = chunk[threadIdx.x] - t;
  if (threadIdx.x == RT_BLOCK - 1) total[k] = chunk[threadIdx.x];
  __syncthreads();
  chunk[threadIdx.x] = before;
  __syncthreads();
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x) {
    uint32_t r = UINT32_MAX;
    if (acc[m]) {
      const uint32_t i = matches[2 * m + col], w = i >> 5;
      r = chunk[w / kRun];
      for (uint32_t j = w - w % kRun; j < w; ++j) r += __popc(bits[j]);
      r += __popc(bits[w] & ((1u << (i & 31)) - 1u));
    }
    rank[m] = r;
  }
}

// the kept matches as (feature of image1, feature of image2) at cbeg[pair] + rank
__global__ void k_rp_place(uint32_t n_pairs, const uint32_t* __restrict__ pair_img, const uint64_t* __restrict__ moff,
                           const uint32_t* __restrict__ matches, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ img_foff,
                           const uint32_t* __restrict__ cbeg, uint32_t* __restrict__ corr) {
  const uint32_t k = blockIdx.x;
  if (k >= n_pairs) return;
  const uint32_t a = pair_img[2 * k], b = pair_img[2 * k + 1];
  const uint32_t col = a < b ? 0u : 1u;
  const uint32_t f1 = img_foff[col ? b : a], f2 = img_foff[col ? a : b];
  for (uint64_t m = moff[k] + threadIdx.x; m < moff[k + 1]; m += blockDim.x)
    if (rank[m] != UINT32_MAX) {
      const size_t c = (size_t)cbeg[k] + rank[m];
      corr[2 * c] = f1 + matches[2 * m + col];
      corr[2 * c + 1] = f2 + matches[2 * m + 1 - col];
    }
}

// num_tri_corrs of the listed pairs (list NULL: every pair) from the current state, one workgroup per pair; with `decide` the
// ratio test of Retriangulate (:301-306) in double, and the status of the pair at its turn: closed, or open_status (what the
// checks after the ratio make of an open pair)
__global__ void k_rp_gate(uint32_t n, const uint32_t* __restrict__ list, const uint32_t* __restrict__ cbeg, const uint32_t* __restrict__ ctotal,
                          const uint32_t* __restrict__ corr, const int32_t* __restrict__ pid, int decide, double re_min_ratio,
                          const uint8_t* __restrict__ open_status, uint8_t* __restrict__ status, uint32_t* __restrict__ tri) {
  __shared__ uint32_t sh[RT_BLOCK];
  if (blockIdx.x >= n) return;
  const uint32_t k = list ? list[blockIdx.x] : blockIdx.x;
  const uint32_t lo = cbeg[k], hi = lo + ctotal[k];
  uint32_t c = 0;
  for (uint32_t e = lo + threadIdx.x; e < hi; e += blockDim.x) {
    const int32_t p = pid[corr[2 * (size_t)e]];
    if (p >= 0 && p == pid[corr[2 * (size_t)e + 1]]) ++c;
  }
  sh[threadIdx.x] = c;
  __syncthreads();
  for (int d = RT_BLOCK / 2; d > 0; d /= 2) {
    if (threadIdx.x < (uint32_t)d) sh[threadIdx.x] += sh[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  tri[k] = sh[0];
  if (decide) {
    const double tri_ratio = static_cast<double>(sh[0]) / static_cast<double>(hi - lo);
    status[k] = tri_ratio >= re_min_ratio ? DSM_PAIR_CLOSED_BY_ITS_TURN : open_status[k];
  }
}

// One lane per (pair of the round, kept correspondence): work items w0 .. w0 + W of the round-ordered list, whose entry j
// (j0 <= j < j1) is pair wl_pair[j] with its correspondences at wl_off[j] .. wl_off[j + 1] (none for a pair that is only gated).
__global__ void k_rp_solve(uint32_t W, uint32_t w0, uint32_t j0, uint32_t j1, const uint32_t* __restrict__ wl_pair,
                           const uint32_t* __restrict__ wl_off, const uint32_t* __restrict__ cbeg, const uint8_t* __restrict__ status,
                           const uint32_t* __restrict__ corr, const uint32_t* __restrict__ deg, const double* __restrict__ pxyz,
                           const uint32_t* __restrict__ feat_img, const double* __restrict__ img_P, const double* __restrict__ img_C,
                           const double* __restrict__ uv, RtParams prm, int32_t* __restrict__ pid, double* __restrict__ nxyz,
                           uint8_t* __restrict__ outcome, double* __restrict__ margins) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W) return;
  const uint32_t w = w0 + i;
  uint32_t lo = j0, hi = j1 - 1;
  while (lo < hi) {  // the entry that holds w: the first with wl_off[j + 1] > w
    const uint32_t mid = (lo + hi) / 2;
    if (wl_off[mid + 1] > w)
      hi = mid;
    else
      lo = mid + 1;
  }
  const uint32_t k = wl_pair[lo];
  if (status[k] != DSM_PAIR_PROCESSED) return;
  const size_t e = (size_t)cbeg[k] + (w - wl_off[lo]);
  const uint32_t f1 = corr[2 * e], f2 = corr[2 * e + 1];
  const int32_t p1 = pid[f1], p2 = pid[f2];
  double mg[kRpMargins] = {INFINITY, INFINITY, INFINITY, INFINITY};
  uint8_t oc;
  if (p1 >= 0 && p2 >= 0) {
    oc = RC_BOTH;
  } else if (p1 >= 0 || p2 >= 0) {  // Continue (:545-586) of the feature without a point onto the other's
    const uint32_t g = p1 >= 0 ? f2 : f1;
    const int32_t p = p1 >= 0 ? p1 : p2;
    const double* X = (uint32_t)p < prm.num_points ? &pxyz[3 * (size_t)p] : &nxyz[3 * (size_t)((uint32_t)p - prm.num_points)];
    RtView v;
    rt_load(g, feat_img, img_P, img_C, uv, &v);
    double cd;
    const double err = sqrt(rt_residual(v, X, &cd));
    if (!(cd <= kRtCosineEdge)) mg[3] = 0.0;
    oc = RC_CONTINUE_REJECTED;
    if (err < DBL_MAX) {
      mg[3] = fmin(mg[3], fabs(err - prm.continue_max_error) / prm.continue_max_error);
      if (err <= prm.continue_max_error) {
        pid[g] = p;
        oc = p1 >= 0 ? RC_CONTINUED_2 : RC_CONTINUED_1;
      }
    }
  } else if (prm.ignore_two_view && deg[f1] == 1 && deg[f2] == 1) {  // IsTwoViewObservation of the feature of image1
    oc = RC_TWO_VIEW;
  } else {  // Create (:461-543) on two views: one trial, no local optimisation
    RtView va, vb;
    rt_load(f1, feat_img, img_P, img_C, uv, &va);
    rt_load(f2, feat_img, img_P, img_C, uv, &vb);
    double X[3];
    triangulate_two_view(va.P, vb.P, va.u, va.v, vb.u, vb.v, X);
    oc = RC_CREATE_FAILED;
    const bool d0 = rt_depth(va, X, &mg[2]);
    if (d0 && rt_depth(vb, X, &mg[2]) && rt_angle_ok(tri_angle_libm(va.C, vb.C, X), prm.min_tri_angle, &mg[1])) {
      uint32_t c = 0;
      for (int s = 0; s < 2; ++s) {
        double cd;
        const double r = rt_residual(s ? vb : va, X, &cd);
        mg[0] = fmin(mg[0], cd <= kRtCosineEdge ? fabs(r - prm.max_residual) / prm.max_residual : 0.0);
        if (r <= prm.max_residual) ++c;
      }
      if (c == 2) {
        nxyz[3 * e] = X[0];
        nxyz[3 * e + 1] = X[1];
        nxyz[3 * e + 2] = X[2];
        pid[f1] = pid[f2] = (int32_t)(prm.num_points + (uint32_t)e);
        oc = RC_CREATED;
      }
    }
  }
  outcome[e] = oc;
  for (int s = 0; s < kRpMargins; ++s) margins[e * kRpMargins + s] = mg[s];
}

struct RpBufs {
  DevBuf pair_img, moff, matches, nfeat, foff, acc, deg, total, rank, cbeg, corr, tri, status, open_status;
  DevBuf feat_img, img_ok, img_cam, cams, xy, uv, img_P, img_C, pid, pxyz, wl_pair, wl_off, nxyz, outcome, margins;
};

}  // namespace

extern "C" void dsm_default_pair_retriangulation_options(dsm_pair_retriangulation_options* o) {
  dsm_default_triangulation_options(&o->tri);
  o->re_max_angle_error = 5.0;  // IncrementalTriangulator::Options (incremental_triangulator.h:65-73)
  o->re_min_ratio = 0.2;
  o->re_max_trials = 1;
  o->reserved = 0;
}

extern "C" int dsm_retriangulate_pairs(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                       uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                       const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                                       const uint32_t* points2D_offsets, const double* points2D_xy, const int32_t* points2D_point3D,
                                       uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, uint32_t num_pairs,
                                       const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                       uint64_t next_point3D_id, const dsm_pair_retriangulation_options* options,
                                       uint32_t* re_num_trials, uint64_t* new_point_ids, double* new_point_xyz, uint32_t* new_track_obs,
                                       uint64_t* n_new_points, uint32_t* continued_obs, uint64_t* continued_point_ids,
                                       uint64_t* n_continued, uint32_t* touched_obs, uint64_t* touched_point_ids, uint64_t* n_touched,
                                       uint32_t* pair_num_total_corrs, uint32_t* pair_num_tri_corrs, uint8_t* pair_status,
                                       uint64_t* num_tris_out, dsm_pair_retriangulation_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_retriangulate_pairs", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  if ((num_cameras && (!camera_ids || !cameras)) || (num_images && (!image_ids || !image_camera_ids || !image_registered || !image_qvec ||
                                                                     !image_tvec)) ||
      !points2D_offsets || (num_points3D && (!point3D_ids || !point3D_xyz)) || (num_pairs && (!pair_image_ids || !matches)) ||
      !match_offsets || !n_new_points || !n_continued || !n_touched || !num_tris_out)
    return fail("NULL argument");
  dsm_pair_retriangulation_options po;
  if (options)
    po = *options;
  else
    dsm_default_pair_retriangulation_options(&po);
  const dsm_triangulation_options& o = po.tri;
  if (const char* msg = rt_options_error(o)) return fail(msg);
  if (!std::isfinite(po.re_max_angle_error) || !(po.re_max_angle_error > 0)) return fail("re_max_angle_error must be finite and positive");
  if (!std::isfinite(po.re_min_ratio) || !(po.re_min_ratio >= 0)) return fail("re_min_ratio must be finite and not negative");
  if (po.re_max_trials < 0) return fail("re_max_trials must not be negative");
  dsm_pair_retriangulation_report rep{};
  rep.min_residual_margin = rep.min_angle_margin = rep.min_depth_margin = rep.min_continue_margin = rep.min_bogus_margin = INFINITY;

  RtScene S;
  {
    const std::string msg = rt_load_scene(S, num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, image_registered,
                                          image_qvec, image_tvec, points2D_offsets, points2D_xy, points2D_point3D, num_points3D, point3D_ids,
                                          point3D_xyz, num_pairs, pair_image_ids, match_offsets, matches, next_point3D_id, o,
                                          &rep.min_bogus_margin);
    if (!msg.empty()) return fail(msg.c_str());
  }
  const uint64_t F = S.F, NM = S.NM;
  const size_t F1 = std::max<uint64_t>(F, 1), K1 = std::max<uint32_t>(num_pairs, 1);
  // the sequential order: ascending (image1, image2) in canonical indices = ascending ImagePairToPairId
  std::vector<uint32_t> porder(num_pairs);
  std::iota(porder.begin(), porder.end(), 0u);
  auto pair_key = [&](uint32_t k) {
    const uint32_t a = S.pair_img[2 * k], b = S.pair_img[2 * k + 1];
    return ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
  };
  std::sort(porder.begin(), porder.end(), [&](uint32_t x, uint32_t y) { return pair_key(x) < pair_key(y); });
  const double setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  RpBufs d;
  DevEvents<5> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));

  // ------------------------------------------------------------ the duplicate rule, the counts per feature, the ranks (device)
  std::vector<uint32_t> ctotal(num_pairs, 0), cbeg(num_pairs, 0), tri0(num_pairs, 0);
  HIPCHK(ctx, dev_upload(d.nfeat, S.nfeat.data(), S.nfeat.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.foff, S.foff.data(), S.foff.size() * 4, st));
  HIPCHK(ctx, d.deg.reserve(F1 * 4));
  HIPCHK(ctx, hipMemsetAsync(d.deg.p, 0, F1 * 4, st));
  HIPCHK(ctx, dev_upload(d.pid, S.pid0.data(), F * 4, st));
  if (NM) {
    HIPCHK(ctx, dev_upload(d.pair_img, S.pair_img.data(), S.pair_img.size() * 4, st));
    HIPCHK(ctx, dev_upload(d.moff, match_offsets, ((size_t)num_pairs + 1) * 8, st));
    HIPCHK(ctx, dev_upload(d.matches, matches, NM * 8, st));
    HIPCHK(ctx, d.acc.reserve(NM));
    HIPCHK(ctx, d.rank.reserve(NM * 4));
    HIPCHK(ctx, d.total.reserve(K1 * 4));
    hipLaunchKernelGGL(k_rt_dedup, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.nfeat.as<uint32_t>(), d.acc.as<uint8_t>());
    hipLaunchKernelGGL(k_rt_count, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.acc.as<uint8_t>(), d.foff.as<uint32_t>(), d.deg.as<uint32_t>());
    hipLaunchKernelGGL(k_rp_rank, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.nfeat.as<uint32_t>(), d.acc.as<uint8_t>(), d.total.as<uint32_t>(), d.rank.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(ctotal.data(), d.total.p, (size_t)num_pairs * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  uint64_t C = 0;  // the correspondence list in sequential (pair, correspondence) order
  for (uint32_t k : porder) {
    cbeg[k] = (uint32_t)C;
    C += ctotal[k];
  }
  const size_t C1 = std::max<uint64_t>(C, 1);
  rep.num_correspondences = C;
  std::vector<uint32_t> corr(2 * C);
  HIPCHK(ctx, d.corr.reserve(C1 * 8));
  HIPCHK(ctx, d.tri.reserve(K1 * 4));
  HIPCHK(ctx, dev_upload(d.total, ctotal.data(), (size_t)num_pairs * 4, st));
  HIPCHK(ctx, dev_upload(d.cbeg, cbeg.data(), (size_t)num_pairs * 4, st));
  if (C) {
    hipLaunchKernelGGL(k_rp_place, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, d.pair_img.as<uint32_t>(), d.moff.as<uint64_t>(),
                       d.matches.as<uint32_t>(), d.rank.as<uint32_t>(), d.foff.as<uint32_t>(), d.cbeg.as<uint32_t>(), d.corr.as<uint32_t>());
    hipLaunchKernelGGL(k_rp_gate, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, (const uint32_t*)nullptr, d.cbeg.as<uint32_t>(),
                       d.total.as<uint32_t>(), d.corr.as<uint32_t>(), d.pid.as<int32_t>(), 0, 0.0, (const uint8_t*)nullptr, (uint8_t*)nullptr,
                       d.tri.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(corr.data(), d.corr.p, C * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(tri0.data(), d.tri.p, (size_t)num_pairs * 4, hipMemcpyDeviceToHost, st));
  }
  // ImageToWorld of every feature of a usable image, and the poses
  HIPCHK(ctx, dev_upload(d.feat_img, S.feat_img.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(d.img_ok, S.img_ok.data(), num_images, st));
  HIPCHK(ctx, dev_upload(d.img_cam, S.img_cam.data(), (size_t)num_images * 4, st));
  HIPCHK(ctx, dev_upload(d.cams, cameras, (size_t)num_cameras * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.xy, S.xy.data(), F * 16, st));
  HIPCHK(ctx, d.uv.reserve(F1 * 16));
  HIPCHK(ctx, dev_upload(d.img_P, S.img_P.data(), S.img_P.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.img_C, S.img_C.data(), S.img_C.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.pxyz, point3D_xyz, (size_t)num_points3D * 24, st));
  if (F) {
    hipLaunchKernelGGL(k_rt_normalize, dim3((uint32_t)((F + RT_BLOCK - 1) / RT_BLOCK)), dim3(RT_BLOCK), 0, st, (uint32_t)F, d.feat_img.as<uint32_t>(),
                       d.img_ok.as<uint8_t>(), d.img_cam.as<uint32_t>(), d.cams.as<dsm_camera>(), d.xy.as<double>(), d.uv.as<double>());
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, d.nxyz.reserve(C1 * 24));
  HIPCHK(ctx, d.outcome.reserve(C1));
  HIPCHK(ctx, hipMemsetAsync(d.outcome.p, RC_NOT_RUN, C1, st));
  HIPCHK(ctx, d.margins.reserve(C1 * kRpMargins * 8));
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  HIPCHK(ctx, hipStreamSynchronize(st));

  // ------------------------------------------------------------ candidates and their rounds (host)
  // The ratio never falls during the call, so a pair that is closed on the input state never does anything.  Every other
  // pair is gated at its turn; what an open pair then does is known now: nothing with an unregistered image or with its
  // trials exhausted, a counted trial and nothing more on a bogus camera, the solve otherwise (a candidate).  A candidate's
  // round is 1 + the largest round of the earlier candidates that share a feature with it: one pass in sequential order
  // with the largest round written per feature.  A pair that is only gated takes 1 + that round too, reads there and writes
  // nothing; a later candidate that shares a feature with it must not write before that read, so its round is at least the
  // largest round an earlier gate-only pair read one of its features in (equal is enough: a round's gate precedes its solve).
  const auto t_sched0 = std::chrono::steady_clock::now();
  std::vector<uint8_t> status(num_pairs, DSM_PAIR_NOT_UNDER_RECONSTRUCTED), open_status(num_pairs, DSM_PAIR_PROCESSED);
  std::vector<uint32_t> last(F1, 0), read(F1, 0), cand, cand_round;  // per feature: last round written, last gate-only read
  uint32_t nrounds = 0;
  for (uint32_t k : porder) {
    if (ctotal[k] == 0) continue;
    const uint32_t a = S.pair_img[2 * k], b = S.pair_img[2 * k + 1];
    if (static_cast<double>(tri0[k]) / static_cast<double>(ctotal[k]) >= po.re_min_ratio) continue;
    if (!image_registered[S.order[a]] || !image_registered[S.order[b]])
      open_status[k] = DSM_PAIR_UNREGISTERED;
    else if ((int64_t)(re_num_trials ? re_num_trials[k] : 0u) >= (int64_t)po.re_max_trials)
      open_status[k] = DSM_PAIR_TRIALS_EXHAUSTED;
    else if (S.cam_bogus[S.img_cam[a]] || S.cam_bogus[S.img_cam[b]])
      open_status[k] = DSM_PAIR_BOGUS_CAMERA;
    else
      ++rep.num_candidates;
    const bool solves = open_status[k] == DSM_PAIR_PROCESSED;
    const size_t e0 = 2 * (size_t)cbeg[k], e1 = 2 * ((size_t)cbeg[k] + ctotal[k]);
    uint32_t r = 0;
    for (size_t e = e0; e < e1; ++e) r = std::max(r, last[corr[e]]);
    ++r;
    if (solves)
      for (size_t e = e0; e < e1; ++e) r = std::max(r, read[corr[e]]);
    for (size_t e = e0; e < e1; ++e) {
      if (solves)
        last[corr[e]] = r;
      else
        read[corr[e]] = std::max(read[corr[e]], r);
    }
    cand.push_back(k);
    cand_round.push_back(r);
    nrounds = std::max(nrounds, r);
  }
  const uint32_t NC = (uint32_t)cand.size();
  std::vector<uint32_t> roff(nrounds + 2, 0), wl_pair(NC), wl_off(NC + 1, 0);  // the gated pairs by (round, sequential order)
  for (uint32_t c = 0; c < NC; ++c) ++roff[cand_round[c] + 1];
  for (uint32_t r = 1; r <= nrounds + 1; ++r) roff[r] += roff[r - 1];
  {
    std::vector<uint32_t> fillp(roff.begin(), roff.end() - 1);
    for (uint32_t c = 0; c < NC; ++c) wl_pair[fillp[cand_round[c]]++] = cand[c];
  }
  for (uint32_t j = 0; j < NC; ++j) wl_off[j + 1] = wl_off[j] + (open_status[wl_pair[j]] == DSM_PAIR_PROCESSED ? ctotal[wl_pair[j]] : 0u);
  rep.num_rounds = nrounds;
  rep.schedule_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_sched0).count();

  RtParams prm;
  prm.max_residual = (o.create_max_angle_error * kRtDegToRad) * (o.create_max_angle_error * kRtDegToRad);
  prm.min_tri_angle = o.min_angle * kRtDegToRad;
  prm.continue_max_error = po.re_max_angle_error * kRtDegToRad;
  prm.ignore_two_view = o.ignore_two_view_tracks ? 1 : 0;
  prm.max_trials = 1;
  prm.tab_n = 0;
  prm.num_points = num_points3D;
  if ((uint64_t)num_points3D + C >= 0x7fffffffu) return fail("too many points3D and correspondences");
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  HIPCHK(ctx, dev_upload(d.status, status.data(), num_pairs, st));
  HIPCHK(ctx, dev_upload(d.open_status, open_status.data(), num_pairs, st));
  HIPCHK(ctx, dev_upload(d.wl_pair, wl_pair.data(), (size_t)NC * 4, st));
  HIPCHK(ctx, dev_upload(d.wl_off, wl_off.data(), ((size_t)NC + 1) * 4, st));
  const bool timed = nrounds <= kRpTimedRounds;
  DevEventList rev(timed ? 3 * (size_t)nrounds : 0);  // per round: before the gate, before the solve, after it
  HIPCHK(ctx, rev.create());
  for (uint32_t r = 1; r <= nrounds; ++r) {  // every round enqueued back to back: the schedule needs no result
    const uint32_t j0 = roff[r], j1 = roff[r + 1], W = wl_off[j1] - wl_off[j0];
    if (j1 == j0) continue;
    DevEvent* re = timed ? &rev[3 * (size_t)(r - 1)] : nullptr;
    if (timed) HIPCHK(ctx, hipEventRecord(re[0], st));
    hipLaunchKernelGGL(k_rp_gate, dim3(j1 - j0), dim3(RT_BLOCK), 0, st, j1 - j0, d.wl_pair.as<uint32_t>() + j0, d.cbeg.as<uint32_t>(),
                       d.total.as<uint32_t>(), d.corr.as<uint32_t>(), d.pid.as<int32_t>(), 1, po.re_min_ratio, d.open_status.as<uint8_t>(),
                       d.status.as<uint8_t>(), d.tri.as<uint32_t>());
    if (timed) HIPCHK(ctx, hipEventRecord(re[1], st));
    if (W)
      hipLaunchKernelGGL(k_rp_solve, dim3((W + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, st, W, wl_off[j0], j0, j1, d.wl_pair.as<uint32_t>(),
                         d.wl_off.as<uint32_t>(), d.cbeg.as<uint32_t>(), d.status.as<uint8_t>(), d.corr.as<uint32_t>(), d.deg.as<uint32_t>(),
                         d.pxyz.as<double>(), d.feat_img.as<uint32_t>(), d.img_P.as<double>(), d.img_C.as<double>(), d.uv.as<double>(), prm,
                         d.pid.as<int32_t>(), d.nxyz.as<double>(), d.outcome.as<uint8_t>(), d.margins.as<double>());
    HIPCHK(ctx, hipGetLastError());
    if (timed) HIPCHK(ctx, hipEventRecord(re[2], st));
  }
  HIPCHK(ctx, hipEventRecord(ev[3], st));

  // ------------------------------------------------------------ the final counts, results back, new ids in sequential order
  std::vector<uint32_t> tri1(num_pairs, 0);
  std::vector<int32_t> pid1(F);
  std::vector<uint8_t> outcome(C);
  std::vector<double> nxyz(3 * C), margins(C * kRpMargins);
  if (C) {
    hipLaunchKernelGGL(k_rp_gate, dim3(num_pairs), dim3(RT_BLOCK), 0, st, num_pairs, (const uint32_t*)nullptr, d.cbeg.as<uint32_t>(),
                       d.total.as<uint32_t>(), d.corr.as<uint32_t>(), d.pid.as<int32_t>(), 0, 0.0, (const uint8_t*)nullptr, (uint8_t*)nullptr,
                       d.tri.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(tri1.data(), d.tri.p, (size_t)num_pairs * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(status.data(), d.status.p, num_pairs, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(pid1.data(), d.pid.p, F * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(outcome.data(), d.outcome.p, C, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(nxyz.data(), d.nxyz.p, C * 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(margins.data(), d.margins.p, margins.size() * 8, hipMemcpyDeviceToHost, st));
  } else {
    pid1 = S.pid0;
  }
  HIPCHK(ctx, hipEventRecord(ev[4], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const auto t_out0 = std::chrono::steady_clock::now();
  auto obs_of = [&](uint32_t f, uint32_t* out) {
    const uint32_t c = S.feat_img[f];
    out[0] = image_ids[S.order[c]];
    out[1] = f - S.foff[c];
  };
  std::vector<uint64_t> slot_id(C, 0);  // correspondence slot -> final id of the point created there
  uint64_t pnew = 0;
  for (uint64_t e = 0; e < C; ++e)
    if (outcome[e] == RC_CREATED) {
      slot_id[e] = S.next_id + pnew;
      if (new_point_ids) new_point_ids[pnew] = slot_id[e];
      if (new_point_xyz)
        for (int j = 0; j < 3; ++j) new_point_xyz[3 * pnew + j] = nxyz[3 * e + j];
      if (new_track_obs) {
        obs_of(corr[2 * e], &new_track_obs[4 * pnew]);
        obs_of(corr[2 * e + 1], &new_track_obs[4 * pnew + 2]);
      }
      ++pnew;
    }
  auto final_id = [&](int32_t p) -> uint64_t {
    return (uint32_t)p < num_points3D ? point3D_ids[p] : slot_id[(uint32_t)p - num_points3D];
  };
  uint64_t ncont = 0;
  for (uint64_t e = 0; e < C; ++e) {
    const uint8_t oc = outcome[e];
    if (oc == RC_NOT_RUN) continue;
    rep.num_both += oc == RC_BOTH;
    rep.num_continue_tried += oc == RC_CONTINUE_REJECTED || oc == RC_CONTINUED_1 || oc == RC_CONTINUED_2;
    rep.num_two_view_skipped += oc == RC_TWO_VIEW;
    rep.num_create_tried += oc == RC_CREATE_FAILED || oc == RC_CREATED;
    if (oc == RC_CONTINUED_1 || oc == RC_CONTINUED_2) {
      const uint32_t f = corr[2 * e + (oc == RC_CONTINUED_2)];
      if (continued_obs) obs_of(f, &continued_obs[2 * ncont]);
      if (continued_point_ids) continued_point_ids[ncont] = final_id(pid1[f]);
      ++ncont;
    }
    const double* mg = &margins[e * kRpMargins];
    rep.min_residual_margin = std::min(rep.min_residual_margin, mg[0]);
    rep.min_angle_margin = std::min(rep.min_angle_margin, mg[1]);
    rep.min_depth_margin = std::min(rep.min_depth_margin, mg[2]);
    rep.min_continue_margin = std::min(rep.min_continue_margin, mg[3]);
  }
  uint64_t nt = 0;
  for (uint64_t f = 0; f < F; ++f)
    if (pid1[f] != S.pid0[f]) {
      if (touched_obs) obs_of((uint32_t)f, &touched_obs[2 * nt]);
      if (touched_point_ids) touched_point_ids[nt] = final_id(pid1[f]);
      ++nt;
    }
  for (uint32_t k = 0; k < num_pairs; ++k) {
    const bool trial = status[k] == DSM_PAIR_PROCESSED || status[k] == DSM_PAIR_BOGUS_CAMERA;
    if (re_num_trials && trial) ++re_num_trials[k];
    if (pair_num_total_corrs) pair_num_total_corrs[k] = ctotal[k];
    if (pair_num_tri_corrs) pair_num_tri_corrs[k] = tri1[k];
    if (pair_status) pair_status[k] = status[k];
    ++rep.num_pairs_by_status[status[k]];
  }
  rep.num_continue_taken = rep.num_continued = ncont;
  rep.num_create_taken = rep.num_new_points = pnew;
  rep.num_tris = ncont + 2 * pnew;
  *n_new_points = pnew;
  *n_continued = ncont;
  *n_touched = nt;
  *num_tris_out = rep.num_tris;
  double g_ms = 0, rounds_ms = 0, dl_ms = 0, tot_ms = 0;
  HIPCHK(ctx, ev.ms(0, 1, &g_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rounds_ms));
  HIPCHK(ctx, ev.ms(3, 4, &dl_ms));
  HIPCHK(ctx, ev.ms(0, 4, &tot_ms));
  for (uint32_t r = 0; timed && r < nrounds; ++r) {
    double a = 0, b = 0;
    HIPCHK(ctx, rev.ms(3 * r, 3 * r + 1, &a));
    HIPCHK(ctx, rev.ms(3 * r + 1, 3 * r + 2, &b));
    rep.gate_ms += a;
    rep.solve_ms += b;
  }
  rep.setup_ms = setup_ms;
  rep.graph_ms = g_ms;
  rep.rounds_ms = rounds_ms;
  rep.round_gap_ms = timed ? std::max(0.0, (double)rounds_ms - rep.gate_ms - rep.solve_ms) : 0.0;
  rep.download_ms = dl_ms;
  rep.assemble_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_out0).count();
  rep.device_ms = tot_ms;
  if (report) *report = rep;
  return DSM_OK;
}
