// track_update_host.cpp -- libdsm_track_update_host.so: dsm_update_tracks on one CPU thread from the kernels' text
// (track_update.h, track_update_load.h).  What tests/test_track_update_cpu.py holds to the restatement and the
// baseline of tools/bench_track_update.py.  No HIP in it.
#define __device__
#define __host__
#define __forceinline__ inline
#define __noinline__ __attribute__((noinline))
#include "ba_project.h"

#define TU_HD static inline
#define TU_HD_MEMBER inline
#define TU_FETCH_INC(ptr) ((*(ptr))++)
#include "track_update_load.h"

namespace {

// CorrespondenceGraph::AddCorrespondences per pair in input order (correspondence_graph.cc:77-161): a match is dropped when
// either feature already holds a correspondence in the pair's other image; the lists in (pair, match) append order
void tu_host_graph(const TuHost& H, const uint64_t* moff, const uint32_t* matches, std::vector<uint32_t>& goff, std::vector<uint32_t>& gval) {
  std::vector<uint8_t> acc(H.NM, 0);
  std::vector<uint32_t> cnt(H.F + 1, 0);
  std::vector<uint8_t> used;
  for (uint32_t k = 0; k < H.K; ++k) {
    const uint32_t a = H.pair_img[2 * k], b = H.pair_img[2 * k + 1];
    used.assign((size_t)H.nfeat[a] + H.nfeat[b], 0);
    for (uint64_t m = moff[k]; m < moff[k + 1]; ++m) {
      const uint32_t x = matches[2 * m], y = H.nfeat[a] + matches[2 * m + 1];
      if (used[x] || used[y]) continue;
      used[x] = used[y] = 1;
      acc[m] = 1;
      ++cnt[H.foff[a] + matches[2 * m]];
      ++cnt[H.foff[b] + matches[2 * m + 1]];
    }
  }
  goff.assign(H.F + 1, 0);
  for (uint64_t f = 0; f < H.F; ++f) goff[f + 1] = goff[f] + cnt[f];
  gval.assign(goff[H.F], 0);
  std::vector<uint32_t> fill(goff.begin(), goff.end() - 1);
  for (uint32_t k = 0; k < H.K; ++k) {
    const uint32_t a = H.pair_img[2 * k], b = H.pair_img[2 * k + 1];
    for (uint64_t m = moff[k]; m < moff[k + 1]; ++m) {
      if (!acc[m]) continue;
      const uint32_t x = H.foff[a] + matches[2 * m], y = H.foff[b] + matches[2 * m + 1];
      gval[fill[x]++] = y;
      gval[fill[y]++] = x;
    }
  }
}

}  // namespace

extern "C" void dsm_tu_host_default_options(dsm_track_update_options* o) { tu_default_options(o); }

extern "C" int dsm_tu_host_update_tracks(uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                                         const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint8_t* image_registered,
                                         const double* image_qvec, const double* image_tvec, const uint32_t* points2D_offsets,
                                         const double* points2D_xy, uint32_t num_pairs, const uint32_t* pair_image_ids,
                                         const uint64_t* match_offsets, const uint32_t* matches, uint32_t num_points3D,
                                         const uint64_t* point3D_ids, const double* point3D_xyz, const uint64_t* track_offsets,
                                         const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps, uint64_t num_selected,
                                         const uint64_t* selected_ids, uint64_t next_point3D_id, const dsm_track_update_options* options,
                                         uint64_t* out_num_points, uint64_t* out_point_ids, double* out_xyz, uint64_t* out_track_offsets,
                                         uint32_t* out_track_obs, uint64_t* out_num_modified, uint64_t* out_modified, uint64_t* step_counts,
                                         dsm_track_update_report* report) {
  if (!out_num_points || !out_num_modified || (num_steps && !step_counts)) return DSM_ERR_INVALID_ARGUMENT;
  TuHost H;
  const std::string msg = tu_load(H, num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, image_registered, image_qvec,
                                  image_tvec, points2D_offsets, points2D_xy, num_pairs, pair_image_ids, match_offsets, matches, num_points3D,
                                  point3D_ids, point3D_xyz, track_offsets, track_obs, num_steps, steps, num_selected, selected_ids,
                                  next_point3D_id, options);
  if (!msg.empty()) return DSM_ERR_INVALID_ARGUMENT;
  std::vector<uint32_t> goff, gval;
  tu_host_graph(H, match_offsets, matches, goff, gval);
  std::vector<uint8_t> modified(H.S, 0);
  std::vector<uint32_t> stamp(H.S), born(H.S), done(H.S), ev_pos(H.S, 0), ev_depth(H.S, 0);
  uint32_t num_slots = H.P;
  TuView v{};
  v.N = H.N, v.P = H.P, v.S = H.S, v.F = H.F;
  v.cams = cameras, v.img_cam = H.img_cam.data(), v.img_reg = H.img_reg.data(), v.img_bogus = H.img_bogus.data(), v.pose = H.pose.data();
  v.feat_img = H.feat_img.data(), v.xy = points2D_xy, v.goff = goff.data(), v.gval = gval.data();
  v.thr2_complete = H.o.complete_max_reproj_error * H.o.complete_max_reproj_error;
  v.thr2_merge = H.o.merge_max_reproj_error * H.o.merge_max_reproj_error;
  v.max_transitivity = H.o.complete_max_transitivity;
  v.f2p = H.f2p.data(), v.fnext = H.fnext.data(), v.xyz = H.xyz.data(), v.head = H.head.data(), v.tail = H.tail.data(), v.len = H.len.data();
  v.alive = H.alive.data(), v.modified = modified.data(), v.stamp = stamp.data(), v.born = born.data(), v.done = done.data();
  v.num_slots = &num_slots, v.ev_pos = ev_pos.data(), v.ev_depth = ev_depth.data();
  dsm_track_update_report rep{};
  rep.num_points = H.P, rep.num_steps = num_steps, rep.num_correspondences = gval.size();
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  for (uint32_t s = 0; s < num_steps; ++s) {
    const std::vector<uint32_t> list = tu_step_list(H);
    uint64_t count = 0;
    if (steps[s] == DSM_TRACKS_COMPLETE) {
      for (uint32_t slot : list) count += tu_complete(v, slot, &mg, &rep.complete_trials);
      rep.num_completed += count;
      ++rep.complete_serial_steps;
    } else {
      std::fill(stamp.begin(), stamp.end(), TU_NIL);
      std::fill(born.begin(), born.end(), 0u);
      std::fill(done.begin(), done.end(), 0u);
      const uint32_t first = num_slots;
      uint32_t clock = 1;
      for (uint32_t i = 0; i < list.size(); ++i) count += tu_merge(v, list[i], i, &clock, &mg, &rep.merge_trials, &rep.num_merge_events, TuSerialTest());
      tu_assign_ids(H, first, num_slots, ev_pos.data(), ev_depth.data());
      rep.num_merged += count;
    }
    step_counts[s] = count;
  }
  const std::vector<uint32_t> out = tu_output_slots(H, H.alive.data());
  uint64_t at = 0, nmod = 0;
  for (size_t i = 0; i < out.size(); ++i) {
    const uint32_t s = out[i];
    if (out_point_ids) out_point_ids[i] = H.slot_id[s];
    if (out_xyz)
      for (int k = 0; k < 3; ++k) out_xyz[3 * i + k] = H.xyz[3 * (size_t)s + k];
    if (out_track_offsets) out_track_offsets[i] = at;
    for (uint32_t f = H.head[s]; f != TU_NIL && H.len[s]; f = H.fnext[f]) {
      if (out_track_obs) {
        out_track_obs[2 * at] = image_ids[H.feat_img[f]];
        out_track_obs[2 * at + 1] = f - H.foff[H.feat_img[f]];
      }
      ++at;
    }
    if (modified[s]) {
      if (out_modified) out_modified[nmod] = H.slot_id[s];
      ++nmod;
    }
  }
  if (out_track_offsets) out_track_offsets[out.size()] = at;
  *out_num_points = out.size();
  *out_num_modified = nmod;
  rep.min_complete_error_margin = mg.complete_error, rep.min_merge_error_margin = mg.merge_error, rep.min_depth_margin = mg.depth;
  rep.min_bogus_margin = H.bogus_margin;
  if (report) *report = rep;
  return DSM_OK;
}
