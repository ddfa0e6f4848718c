// next_images_host.cpp -- the host build of next_images.h: FindNextImages and FindLocalBundle over the stateless
// definitions on one CPU thread from the text the kernels are built from.  What the CPU test holds to tests/next_images_ref.py bit for bit, the
// baseline of tools/bench_next_images.py, and what `make next-images-selftest` runs under the sanitizers.  Two forms of the
// ranking: the sequential selection (ni_serial_rank, the text of DSM_NEXT_IMAGES_SERIAL) and the device's schedule, the packed
// keys of the kernels under std::sort.  No HIP.
#include <cstring>

#define DSM_XT static inline
#define DSM_XT_CONST static const
#define IP_HD static inline
#define IP_D static inline
#include "next_images.h"

extern "C" void dsm_ni_host_default_options(dsm_next_images_options* o) { ni_default_options(o); }
extern "C" uint32_t dsm_ni_host_cell(double x, uint64_t extent) { return ni_cell(x, extent); }
// the score of n points on a width x height image
extern "C" uint64_t dsm_ni_host_score(const double* xy, uint64_t n, uint64_t width, uint64_t height) {
  uint64_t rows[NI_DIM] = {0};
  for (uint64_t i = 0; i < n; ++i) rows[ni_cell(xy[2 * i + 1], height)] |= 1ull << ni_cell(xy[2 * i], width);
  return ni_score(rows);
}
extern "C" float dsm_ni_host_rank(int32_t method, uint32_t num_visible, uint32_t num_observations, uint64_t score) {
  return ni_rank(method, num_visible, num_observations, score);
}
extern "C" uint64_t dsm_ni_host_key(uint32_t flags, int eligible, float rank, uint32_t image_id) { return ni_key(flags, eligible != 0, rank, image_id); }

// dsm_find_next_images without a device.  sorted != 0: the device's schedule of the ranking.  0, or DSM_ERR_INVALID_ARGUMENT /
// DSM_ERR_OUT_OF_RANGE with *why; the outputs are untouched then.
extern "C" int dsm_ni_host_find_next_images(uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                                            const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint32_t* points2D_offsets,
                                            const double* points2D_xy, uint32_t num_pairs, const uint32_t* pair_image_ids,
                                            const uint64_t* match_offsets, const uint32_t* matches, uint32_t num_problems,
                                            const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids, const uint8_t* slot_registered,
                                            const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D, const uint32_t* slot_num_reg_trials,
                                            const uint8_t* slot_filtered, const dsm_next_images_options* options, int sorted, uint64_t* next_offsets,
                                            uint32_t* next_image_ids, uint64_t next_capacity, uint32_t* slot_num_visible,
                                            uint32_t* slot_num_observations, uint64_t* slot_score, const char** why) {
  dsm_next_images_options o;
  if (options)
    o = *options;
  else
    ni_default_options(&o);
  NiSetup N;
  const char* bad = N.load(num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, points2D_offsets, points2D_xy, num_pairs,
                           pair_image_ids, match_offsets, matches, num_problems, problem_image_offsets, problem_image_ids, slot_registered,
                           slot_obs_offsets, slot_obs_point3D, slot_num_reg_trials, slot_filtered, o);
  if (!bad && num_problems && (!next_offsets || !next_image_ids)) bad = "NULL argument";
  if (why) *why = bad;
  if (bad) return N.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  const uint32_t n_slots = (uint32_t)N.slot_img.size(), n_entries = (uint32_t)N.ent_pair.size();
  std::vector<uint8_t> acc(match_offsets[num_pairs] + 1);
  for (uint32_t k = 0; k < num_pairs; ++k)
    ip_host_dedup(N.S.nfeat[N.S.pair_img[2 * k]], N.S.nfeat[N.S.pair_img[2 * k + 1]], matches ? matches + 2 * match_offsets[k] : nullptr,
                  match_offsets[k + 1] - match_offsets[k], acc.data() + match_offsets[k]);
  const uint64_t n_words = N.word_off[n_slots];
  std::vector<uint32_t> vis(n_words + 1, 0), has(n_words + 1, 0), nv(n_slots + 1), no(n_slots + 1), order(n_slots + 1), order_n(num_problems + 1);
  std::vector<uint64_t> score(n_slots + 1), key(n_slots + 1);
  NiView v;
  v.n_problems = num_problems, v.n_slots = n_slots, v.n_entries = n_entries;
  v.slot_off = N.slot_off.data(), v.slot_img = N.slot_img.data(), v.slot_id = N.slot_id.data(), v.slot_flags = N.slot_flags.data();
  v.obs_off = N.obs_off.data(), v.obs_point = slot_obs_point3D, v.word_off = N.word_off.data();
  v.ent_off = N.ent_off.data(), v.ent_pair = N.ent_pair.data(), v.ent_slot = N.ent_slot.data();
  v.moff = match_offsets, v.matches = matches, v.acc = acc.data(), v.row0 = points2D_offsets, v.kp = points2D_xy, v.img_wh = N.img_wh.data();
  v.vis = vis.data(), v.has = has.data(), v.num_visible = nv.data(), v.num_observations = no.data(), v.score = score.data(), v.key = key.data();
  v.order = order.data(), v.order_n = order_n.data();
  v.method = o.image_selection_method, v.min_num_inliers = (uint32_t)o.abs_pose_min_num_inliers;
  if (!sorted) {
    ni_serial(v);
  } else {  // k_ni_visibility, k_ni_slot, k_ni_rank
    for (uint32_t p = 0; p < num_problems; ++p) {
      ni_serial_visibility(v, p);
      std::vector<uint64_t> keys;
      for (uint32_t s = N.slot_off[p]; s < N.slot_off[p + 1]; ++s) {
        ni_serial_slot(v, s);
        if (key[s] != NI_KEY_NONE) keys.push_back(key[s]);
      }
      std::sort(keys.begin(), keys.end());
      for (size_t i = 0; i < keys.size(); ++i) order[N.slot_off[p] + i] = (uint32_t)keys[i];
      order_n[p] = (uint32_t)keys.size();
    }
  }
  uint64_t total = 0;
  for (uint32_t p = 0; p < num_problems; ++p) total += order_n[p];
  if (total > next_capacity) {
    if (why) *why = "next_image_ids is too small";
    return DSM_ERR_OUT_OF_RANGE;
  }
  uint64_t at = 0;
  for (uint32_t p = 0; p < num_problems; ++p) {
    next_offsets[p] = at;
    for (uint32_t i = 0; i < order_n[p]; ++i) next_image_ids[at++] = order[N.slot_off[p] + i];
  }
  if (num_problems) next_offsets[num_problems] = at;
  for (uint32_t s = 0; s < n_slots; ++s) {
    if (slot_num_visible) slot_num_visible[s] = nv[s];
    if (slot_num_observations) slot_num_observations[s] = no[s];
    if (slot_score) slot_score[s] = score[s];
  }
  return DSM_OK;
}

extern "C" void dsm_lb_host_default_options(dsm_local_bundle_selection_options* o) { lb_default_options(o); }
extern "C" uint64_t dsm_lb_host_percentile_index(uint64_t n) { return lb_percentile_index(n); }
extern "C" double dsm_lb_host_percentile(const double* a, uint64_t n) { return ip_rank_serial(a, n, lb_percentile_index(n)); }

// dsm_find_local_bundles without a device: the sequential forms, the angles of the images a chain can reach.  margin (or
// NULL) gets the report's min_tri_angle_margin.  0, or DSM_ERR_INVALID_ARGUMENT / DSM_ERR_OUT_OF_RANGE with *why; the outputs
// are untouched then.
extern "C" int dsm_lb_host_find_local_bundles(uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets, uint32_t num_problems,
                                              const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                                              const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                                              const double* slot_qvec, const double* slot_tvec, const uint64_t* point_offsets,
                                              const double* point_xyz, uint32_t num_queries, const uint32_t* query_problem,
                                              const uint32_t* query_image_id, const dsm_local_bundle_selection_options* options,
                                              uint64_t* bundle_offsets, uint32_t* bundle_image_ids, uint64_t bundle_capacity,
                                              uint64_t* overlap_offsets, uint32_t* overlap_image_ids, uint32_t* overlap_shared,
                                              double* overlap_tri_angle, uint64_t overlap_capacity, double* margin, const char** why) {
  dsm_local_bundle_selection_options o;
  if (options)
    o = *options;
  else
    lb_default_options(&o);
  LbSetup L;
  const char* bad = L.load(num_images, image_ids, points2D_offsets, num_problems, problem_image_offsets, problem_image_ids, slot_registered,
                           slot_obs_offsets, slot_obs_point3D, slot_qvec, slot_tvec, point_offsets, point_xyz, num_queries, query_problem,
                           query_image_id, o);
  const bool want_overlap = overlap_offsets || overlap_image_ids || overlap_shared || overlap_tri_angle;
  if (!bad && ((num_queries && (!bundle_offsets || !bundle_image_ids)) ||
               (want_overlap && num_queries && (!overlap_offsets || !overlap_image_ids || !overlap_shared || !overlap_tri_angle))))
    bad = "NULL argument";
  if (why) *why = bad;
  if (bad) return L.out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  const NiSetup& N = L.N;
  const uint32_t n_slots = (uint32_t)N.slot_img.size();
  const uint64_t n_obs = N.obs_off[n_slots], n_points = point_offsets[num_problems], n_rows = L.row_off[num_queries];
  std::vector<double> center(3 * (size_t)n_slots + 1, 0.0);
  for (uint32_t s = 0; s < n_slots; ++s)
    if (N.slot_flags[s] & NI_SLOT_REGISTERED) ip_projection_center(L.pose.data() + 7 * (size_t)s, L.pose.data() + 7 * (size_t)s + 4, center.data() + 3 * (size_t)s);
  std::vector<uint32_t> trk_start(n_points + 1), trk_fill(n_points + 1), trk_slot(n_obs + 1), shared(n_rows + 1, 0), q_points(num_queries + 1, 0),
      ov_slot(n_rows + 1, 0), ov_n(num_queries + 1, 0);
  LbView v;
  v.n_problems = num_problems, v.n_slots = n_slots, v.n_queries = num_queries, v.n_obs = n_obs, v.n_points = n_points;
  v.slot_off = N.slot_off.data(), v.slot_id = N.slot_id.data(), v.slot_flags = N.slot_flags.data(), v.slot_prob = L.slot_prob.data();
  v.obs_off = N.obs_off.data(), v.obs_point = slot_obs_point3D, v.point_off = point_offsets, v.point_xyz = point_xyz, v.pose = L.pose.data();
  v.center = center.data(), v.trk_start = trk_start.data(), v.trk_fill = trk_fill.data(), v.trk_slot = trk_slot.data();
  v.q_slot = L.q_slot.data(), v.row_off = L.row_off.data(), v.shared = shared.data(), v.q_points = q_points.data(), v.ov_slot = ov_slot.data();
  v.ov_n = ov_n.data();
  lb_serial_tracks(v);
  std::vector<std::vector<uint32_t>> ids(num_queries), cnt(num_queries), bundle(num_queries);
  std::vector<std::vector<double>> ang(num_queries);
  std::vector<double> work;
  std::vector<uint8_t> used;
  double min_margin = ip_inf();
  uint64_t n_bundle = 0, n_overlap = 0;
  for (uint32_t q = 0; q < num_queries; ++q) {
    lb_serial_overlap(v, q, 0);
    const uint32_t qs = L.q_slot[q], s0 = N.slot_off[L.slot_prob[qs]], n = ov_n[q];
    ids[q].resize(n), cnt[q].resize(n), ang[q].assign(n, -1.0);
    work.resize(q_points[q] + 1);
    for (uint32_t i = 0; i < n; ++i) {
      const uint32_t s = ov_slot[L.row_off[q] + i];
      ids[q][i] = N.slot_id[s], cnt[q][i] = shared[L.row_off[q] + (s - s0)];
      if (n > (uint32_t)(o.local_ba_num_images - 1) && lb_reachable(cnt[q][i], q_points[q])) ang[q][i] = lb_serial_tri_angle(v, qs, s, work.data());
    }
    bundle[q].resize(std::min<uint32_t>(n, (uint32_t)(o.local_ba_num_images - 1)) + 1);
    used.resize(n + 1);
    const LbChain ch = lb_select(n, ids[q].data(), cnt[q].data(), ang[q].data(), q_points[q], o.local_ba_num_images, o.local_ba_min_tri_angle, used.data(),
                                 bundle[q].data());
    bundle[q].resize(ch.n_out);
    ip_take(&min_margin, ch.margin);
    n_bundle += ch.n_out, n_overlap += n;
  }
  if (n_bundle > bundle_capacity || (want_overlap && n_overlap > overlap_capacity)) {
    if (why) *why = "an output is too small";
    return DSM_ERR_OUT_OF_RANGE;
  }
  uint64_t at_b = 0, at_o = 0;
  for (uint32_t q = 0; q < num_queries; ++q) {
    bundle_offsets[q] = at_b;
    for (uint32_t id : bundle[q]) bundle_image_ids[at_b++] = id;
    if (!want_overlap) continue;
    overlap_offsets[q] = at_o;
    for (size_t i = 0; i < ids[q].size(); ++i, ++at_o) overlap_image_ids[at_o] = ids[q][i], overlap_shared[at_o] = cnt[q][i], overlap_tri_angle[at_o] = ang[q][i];
  }
  if (num_queries) bundle_offsets[num_queries] = at_b;
  if (num_queries && want_overlap) overlap_offsets[num_queries] = at_o;
  if (margin) *margin = min_margin;
  return DSM_OK;
}
