// track_update_load.h -- the host half that dsm_update_tracks (track_update.hip) and its host build (track_update_host.cpp)
// share: validation of the arguments, the slot order (ascending point3D id), the tracks as linked lists, the
// ids of the merge events and the order of the outputs.  Plain C++, no HIP in it.
#ifndef DAGSFM_AMD_CSRC_TRACK_UPDATE_LOAD_H_
#define DAGSFM_AMD_CSRC_TRACK_UPDATE_LOAD_H_

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "camera_bogus.h"
#include "track_update.h"

constexpr uint32_t kTuMaxPoints2D = 262144;  // per image, as dsm_retriangulate: the duplicate rule's bitmap of a pair

struct TuHost {
  uint32_t C = 0, N = 0, P = 0, S = 1, K = 0;
  uint64_t F = 0, NM = 0, next_id = 0;
  dsm_track_update_options o;
  std::vector<uint32_t> img_cam, nfeat, foff, feat_img, pair_img, head, tail, len, fnext, sel;
  std::vector<uint8_t> img_reg, img_bogus, alive;
  std::vector<double> pose, xyz;
  std::vector<int32_t> f2p;
  std::vector<uint64_t> slot_id;     // [S]
  std::vector<uint32_t> merged;      // the merged slots of the call so far, in id order
  bool sel_all = true;
  double bogus_margin = INFINITY;
};

inline void tu_default_options(dsm_track_update_options* o) {
  memset(o, 0, sizeof(*o));
  o->tri.create_max_angle_error = 2.0;  // dsm_default_triangulation_options; only the three bogus limits are read
  o->tri.continue_max_angle_error = 2.0;
  o->tri.min_angle = 1.5;
  o->tri.min_focal_length_ratio = 0.1;
  o->tri.max_focal_length_ratio = 10.0;
  o->tri.max_extra_param = 1.0;
  o->tri.ransac_confidence = 0.9999;
  o->tri.ransac_min_inlier_ratio = 0.02;
  o->tri.ransac_max_num_trials = 10000;
  o->tri.ignore_two_view_tracks = 1;
  o->tri.max_transitivity = 1;
  o->complete_max_reproj_error = 4.0;  // IncrementalTriangulator::Options (incremental_triangulator.h)
  o->merge_max_reproj_error = 4.0;
  o->complete_max_transitivity = 5;
}

// the message of the first invalid argument, or an empty string
inline std::string tu_load(TuHost& H, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                           const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint8_t* image_registered,
                           const double* image_qvec, const double* image_tvec, const uint32_t* points2D_offsets, const double* points2D_xy,
                           uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                           uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, const uint64_t* track_offsets,
                           const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps, uint64_t num_selected,
                           const uint64_t* selected_ids, uint64_t next_point3D_id, const dsm_track_update_options* options) {
  if ((num_cameras && (!camera_ids || !cameras)) ||
      (num_images && (!image_ids || !image_camera_ids || !image_registered || !image_qvec || !image_tvec)) || !points2D_offsets ||
      (num_points3D && (!point3D_ids || !point3D_xyz)) || !track_offsets || (num_pairs && !pair_image_ids) || !match_offsets ||
      (num_steps && !steps))
    return "NULL argument";
  if (options)
    H.o = *options;
  else
    tu_default_options(&H.o);
  const dsm_track_update_options& o = H.o;
  if (o.complete_max_transitivity < 1) return "complete_max_transitivity < 1";
  for (double t : {o.complete_max_reproj_error, o.merge_max_reproj_error, o.tri.max_extra_param, o.tri.max_focal_length_ratio})
    if (!(t >= 0) || !std::isfinite(t)) return "option out of range";
  if (!(o.tri.min_focal_length_ratio > 0) || !(o.tri.max_focal_length_ratio >= o.tri.min_focal_length_ratio)) return "option out of range";
  for (uint32_t s = 0; s < num_steps; ++s)
    if (steps[s] != DSM_TRACKS_MERGE && steps[s] != DSM_TRACKS_COMPLETE) return "an unknown step";
  H.C = num_cameras, H.N = num_images, H.P = num_points3D, H.K = num_pairs;
  // cameras
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
    cam_bogus[c] = cam_has_bogus_params(k, o.tri.min_focal_length_ratio, o.tri.max_focal_length_ratio, o.tri.max_extra_param, &H.bogus_margin);
  }
  auto find_cam = [&](uint32_t id) -> int64_t {
    auto it = std::lower_bound(cam_order.begin(), cam_order.end(), id, [&](uint32_t a, uint32_t v) { return camera_ids[a] < v; });
    return (it != cam_order.end() && camera_ids[*it] == id) ? (int64_t)*it : -1;
  };
  // images, in input order
  std::vector<uint32_t> img_order(num_images);
  std::iota(img_order.begin(), img_order.end(), 0u);
  std::sort(img_order.begin(), img_order.end(), [&](uint32_t a, uint32_t b) { return image_ids[a] < image_ids[b]; });
  for (uint32_t i = 1; i < num_images; ++i)
    if (image_ids[img_order[i]] == image_ids[img_order[i - 1]]) return "a repeated image id";
  // id -> input index: a direct table where the ids are dense enough (the usual case), a binary search otherwise
  const uint32_t max_img_id = num_images ? image_ids[img_order[num_images - 1]] : 0;
  std::vector<int32_t> img_table;
  if (num_images && (uint64_t)max_img_id < 16 * (uint64_t)num_images + 1024) {
    img_table.assign((size_t)max_img_id + 1, -1);
    for (uint32_t i = 0; i < num_images; ++i) img_table[image_ids[i]] = (int32_t)i;
  }
  auto find_img = [&](uint32_t id) -> int64_t {
    if (!img_table.empty()) return id <= max_img_id ? (int64_t)img_table[id] : -1;
    auto it = std::lower_bound(img_order.begin(), img_order.end(), id, [&](uint32_t a, uint32_t v) { return image_ids[a] < v; });
    return (it != img_order.end() && image_ids[*it] == id) ? (int64_t)*it : -1;
  };
  if (points2D_offsets[0] != 0) return "points2D offsets must start at 0";
  H.nfeat.resize(num_images), H.foff.assign((size_t)num_images + 1, 0), H.img_cam.resize(num_images), H.img_reg.resize(num_images);
  H.img_bogus.resize(num_images), H.pose.resize((size_t)TU_POSE * num_images);
  for (uint32_t i = 0; i < num_images; ++i) {
    if (points2D_offsets[i + 1] < points2D_offsets[i]) return "points2D offsets must be non-decreasing";
    H.nfeat[i] = points2D_offsets[i + 1] - points2D_offsets[i];
    if (H.nfeat[i] > kTuMaxPoints2D) return "more than 262144 points2D in one image";
    H.foff[i + 1] = points2D_offsets[i + 1];
    const int64_t cam = find_cam(image_camera_ids[i]);
    if (cam < 0) return "an image on an unknown camera id";
    H.img_cam[i] = (uint32_t)cam;
    H.img_reg[i] = image_registered[i] != 0;
    H.img_bogus[i] = cam_bogus[cam];
    const double* qv = image_qvec + 4 * (size_t)i;
    const double* tv = image_tvec + 3 * (size_t)i;
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(qv[k])) return "non-finite qvec";
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(tv[k])) return "non-finite tvec";
    // NormalizeQuaternion + Eigen's toRotationMatrix (pose.cc:75-91), as point_filter.hip's k_pf_images
    const double nq = std::sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
    if (nq == 0) return "a zero qvec";
    const double w = qv[0] / nq, x = qv[1] / nq, y = qv[2] / nq, z = qv[3] / nq;
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
                 tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
    double* T = &H.pose[(size_t)TU_POSE * i];
    for (int k = 0; k < 9; ++k) T[k] = R[k];
    for (int k = 0; k < 3; ++k) T[9 + k] = tv[k];
  }
  H.F = points2D_offsets[num_images];
  if (H.F >= 0x40000000u) return "too many points2D";
  if (H.F && !points2D_xy) return "NULL argument";
  for (size_t i = 0; i < 2 * (size_t)H.F; ++i)
    if (!std::isfinite(points2D_xy[i])) return "non-finite points2D xy";
  H.feat_img.resize(H.F);
  for (uint32_t i = 0; i < num_images; ++i)
    for (uint32_t k = H.foff[i]; k < H.foff[i + 1]; ++k) H.feat_img[k] = i;
  // pairs
  if (match_offsets[0] != 0) return "match offsets must start at 0";
  H.pair_img.resize(2 * (size_t)num_pairs);
  std::vector<uint64_t> pair_keys(num_pairs);
  for (uint32_t k = 0; k < num_pairs; ++k) {
    if (match_offsets[k + 1] < match_offsets[k]) return "match offsets must be non-decreasing";
    if (match_offsets[k + 1] > match_offsets[k] && !matches) return "NULL argument";
    const int64_t a = find_img(pair_image_ids[2 * k]), b = find_img(pair_image_ids[2 * k + 1]);
    if (a < 0 || b < 0) return "a pair on an unknown image id";
    if (a == b) return "a self-pair";
    H.pair_img[2 * k] = (uint32_t)a;
    H.pair_img[2 * k + 1] = (uint32_t)b;
    pair_keys[k] = ((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b);
    for (uint64_t m = match_offsets[k]; m < match_offsets[k + 1]; ++m)
      if (matches[2 * m] >= H.nfeat[a] || matches[2 * m + 1] >= H.nfeat[b]) return "a match index out of range";
  }
  std::sort(pair_keys.begin(), pair_keys.end());
  for (uint32_t k = 1; k < num_pairs; ++k)
    if (pair_keys[k] == pair_keys[k - 1]) return "a repeated pair";
  H.NM = match_offsets[num_pairs];
  if (H.NM >= 0x20000000u) return "too many matches";
  // points: slot = rank by id
  const uint32_t P = num_points3D;
  if (P >= 0x40000000u) return "too many points3D";
  std::vector<uint32_t> order(P);  // slot -> input index
  {
    std::vector<std::pair<uint64_t, uint32_t>> keyed(P);  // sorted with the keys next to each other, not through the index
    for (uint32_t i = 0; i < P; ++i) keyed[i] = {point3D_ids[i], i};
    std::sort(keyed.begin(), keyed.end());
    for (uint32_t i = 0; i < P; ++i) order[i] = keyed[i].second;
  }
  for (uint32_t i = 1; i < P; ++i)
    if (point3D_ids[order[i]] == point3D_ids[order[i - 1]]) return "a repeated point3D id";
  for (size_t i = 0; i < 3 * (size_t)P; ++i)
    if (!std::isfinite(point3D_xyz[i])) return "non-finite point3D xyz";
  const uint64_t max_id = P ? point3D_ids[order[P - 1]] : 0;
  H.next_id = next_point3D_id ? next_point3D_id : max_id + 1;
  if (P && H.next_id <= max_id) return "next_point3D_id at or below an existing id";
  if (track_offsets[0] != 0) return "track offsets must start at 0";
  for (uint32_t i = 0; i < P; ++i)
    if (track_offsets[i + 1] < track_offsets[i]) return "track offsets must be non-decreasing";
  if (track_offsets[P] > H.F) return "a feature in two tracks";  // more elements than features
  if (track_offsets[P] && !track_obs) return "NULL argument";
  H.S = std::max<uint32_t>(2 * P, 2) - 1;
  H.xyz.assign(3 * (size_t)H.S, 0.0), H.head.assign(H.S, TU_NIL), H.tail.assign(H.S, TU_NIL), H.len.assign(H.S, 0), H.alive.assign(H.S, 0);
  H.slot_id.assign(H.S, 0), H.f2p.assign(H.F, -1), H.fnext.assign(H.F, TU_NIL);
  for (uint32_t s = 0; s < P; ++s) {
    const uint32_t i = order[s];
    H.slot_id[s] = point3D_ids[i];
    H.alive[s] = 1;
    for (int k = 0; k < 3; ++k) H.xyz[3 * (size_t)s + k] = point3D_xyz[3 * (size_t)i + k];
    for (uint64_t e = track_offsets[i]; e < track_offsets[i + 1]; ++e) {
      const int64_t im = find_img(track_obs[2 * e]);
      if (im < 0) return "a track element on an unknown image id";
      if (track_obs[2 * e + 1] >= H.nfeat[im]) return "a track element's point2D index out of range";
      if (!H.img_reg[im]) return "a track element in an unregistered image";
      const uint32_t f = H.foff[im] + track_obs[2 * e + 1];
      if (H.f2p[f] >= 0) return "a feature in two tracks";
      H.f2p[f] = (int32_t)s;
      if (H.len[s] == 0)
        H.head[s] = f;
      else
        H.fnext[H.tail[s]] = f;
      H.tail[s] = f;
      H.len[s] += 1;
    }
  }
  // the selection: slots in ascending id
  H.sel_all = selected_ids == nullptr;
  if (!H.sel_all) {
    H.sel.resize(num_selected);
    for (uint64_t k = 0; k < num_selected; ++k) {
      auto it = std::lower_bound(order.begin(), order.end(), selected_ids[k], [&](uint32_t a, uint64_t v) { return point3D_ids[a] < v; });
      if (it == order.end() || point3D_ids[*it] != selected_ids[k]) return "a selected id that is no point3D";
      H.sel[k] = (uint32_t)(it - order.begin());
    }
    std::sort(H.sel.begin(), H.sel.end());
    for (uint64_t k = 1; k < num_selected; ++k)
      if (H.sel[k] == H.sel[k - 1]) return "a repeated selected id";
  }
  return std::string();
}

// the list of a step: the selection, or the snapshot of the ids at the step's start (merged-away slots stay in it: the walks
// skip what no longer exists)
inline std::vector<uint32_t> tu_step_list(const TuHost& H) {
  if (!H.sel_all) return H.sel;
  std::vector<uint32_t> l(H.P);
  std::iota(l.begin(), l.end(), 0u);
  l.insert(l.end(), H.merged.begin(), H.merged.end());
  return l;
}

// The ids of one MERGE step's events, from one ordered pass: slots [first, last) were created by the step, each with the
// position of its outer point in the step's list and its recursion depth; the sequential run creates them in (position,
// depth) order, whatever the components' schedule was.
inline void tu_assign_ids(TuHost& H, uint32_t first, uint32_t last, const uint32_t* ev_pos, const uint32_t* ev_depth) {
  std::vector<uint32_t> ev(last - first);
  std::iota(ev.begin(), ev.end(), first);
  std::sort(ev.begin(), ev.end(), [&](uint32_t a, uint32_t b) {
    return ev_pos[a] != ev_pos[b] ? ev_pos[a] < ev_pos[b] : ev_depth[a] < ev_depth[b];
  });
  for (uint32_t s : ev) {
    H.slot_id[s] = H.next_id++;
    H.merged.push_back(s);
  }
}

// the slots of the output, in ascending id
inline std::vector<uint32_t> tu_output_slots(const TuHost& H, const uint8_t* alive) {
  std::vector<uint32_t> out;
  for (uint32_t s = 0; s < H.P; ++s)
    if (alive[s]) out.push_back(s);
  for (uint32_t s : H.merged)
    if (alive[s]) out.push_back(s);
  return out;
}

#endif  // DAGSFM_AMD_CSRC_TRACK_UPDATE_LOAD_H_
