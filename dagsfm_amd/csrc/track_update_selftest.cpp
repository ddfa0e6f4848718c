// track_update_selftest.cpp -- the host build of track_update.h (track_update_host.cpp) as a stand-alone program under the
// address and undefined-behaviour sanitizers (`make tracks-selftest`): a completion chain cut by the transitivity cap, a merge
// with its recursion and the ids it hands out, a merge chain of 65 points, both step orders, empty inputs, and the refusals with
// their untouched outputs.  The geometry is the one of tests/track_update_scenes.py: f = 500, cameras at (0.5 i, 0, -8) looking
// along +z, points at z = 0, a feature the exact projection of its point plus an offset in pixels.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/dagsfm_mi355x.h"

extern "C" {
void dsm_tu_host_default_options(dsm_track_update_options* o);
int dsm_tu_host_update_tracks(uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                              const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint8_t* image_registered,
                              const double* image_qvec, const double* image_tvec, const uint32_t* points2D_offsets, const double* points2D_xy,
                              uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                              uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, const uint64_t* track_offsets,
                              const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps, uint64_t num_selected,
                              const uint64_t* selected_ids, uint64_t next_point3D_id, const dsm_track_update_options* options,
                              uint64_t* out_num_points, uint64_t* out_point_ids, double* out_xyz, uint64_t* out_track_offsets,
                              uint32_t* out_track_obs, uint64_t* out_num_modified, uint64_t* out_modified, uint64_t* step_counts,
                              dsm_track_update_report* report);
}

static int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

typedef std::pair<uint32_t, uint32_t> Feat;  // (image index, point2D index)

struct Scene {
  uint32_t n;
  std::vector<std::vector<double>> feats;  // per image: x, y, x, y, ...
  std::vector<std::pair<uint32_t, uint32_t>> pairs;
  std::map<std::pair<uint32_t, uint32_t>, std::vector<uint32_t>> links;
  std::vector<uint64_t> ids, toff{0};
  std::vector<double> xyz;
  std::vector<uint32_t> tobs;
  explicit Scene(uint32_t n_images) : n(n_images), feats(n_images) {}
  Feat feat(uint32_t img, double X, double dx = 0.0) {
    feats[img].push_back(500.0 * (X - 0.5 * img) / 8.0 + 320.0 + dx);
    feats[img].push_back(240.0);
    return Feat(img, (uint32_t)feats[img].size() / 2 - 1);
  }
  void link(Feat a, Feat b) {
    if (a.first > b.first) std::swap(a, b);
    const auto key = std::make_pair(a.first, b.first);
    if (!links.count(key)) pairs.push_back(key);
    links[key].push_back(a.second);
    links[key].push_back(b.second);
  }
  void point(uint64_t id, double X, const std::vector<Feat>& elems) {
    ids.push_back(id);
    xyz.insert(xyz.end(), {X, 0.0, 0.0});
    for (const Feat& e : elems) {
      tobs.push_back(3 * e.first + 1);
      tobs.push_back(e.second);
    }
    toff.push_back(tobs.size() / 2);
  }
};

struct Result {
  int rc = 0;
  std::vector<uint64_t> ids, toff, modified, counts;
  std::vector<double> xyz;
  std::vector<uint32_t> obs;
  dsm_track_update_report rep;
};

static Result run(const Scene& s, std::vector<int32_t> steps, const std::vector<uint64_t>* selected = nullptr, int32_t max_t = 5,
                  uint64_t next_id = 0) {
  dsm_camera cam;
  std::memset(&cam, 0, sizeof(cam));
  cam.model_id = 0, cam.width = 640, cam.height = 480;
  cam.params[0] = 500.0, cam.params[1] = 320.0, cam.params[2] = 240.0;
  const uint32_t cam_id = 7;
  std::vector<uint32_t> image_ids(s.n), image_cams(s.n, cam_id), poff{0}, pair_ids, matches;
  std::vector<uint8_t> reg(s.n, 1);
  std::vector<double> qvec, tvec, xy;
  for (uint32_t i = 0; i < s.n; ++i) {
    image_ids[i] = 3 * i + 1;
    qvec.insert(qvec.end(), {1.0, 0.0, 0.0, 0.0});
    tvec.insert(tvec.end(), {-0.5 * i, 0.0, 8.0});
    xy.insert(xy.end(), s.feats[i].begin(), s.feats[i].end());
    poff.push_back((uint32_t)xy.size() / 2);
  }
  std::vector<uint64_t> moff{0};
  for (const auto& p : s.pairs) {
    pair_ids.push_back(3 * p.first + 1);
    pair_ids.push_back(3 * p.second + 1);
    const auto& m = s.links.at(p);
    matches.insert(matches.end(), m.begin(), m.end());
    moff.push_back(matches.size() / 2);
  }
  dsm_track_update_options o;
  dsm_tu_host_default_options(&o);
  o.complete_max_transitivity = max_t;
  const size_t P = s.ids.size(), T = xy.size() / 2;
  Result r;
  r.ids.assign(P + 1, 77), r.toff.assign(P + 2, 77), r.modified.assign(P + 1, 77), r.counts.assign(steps.size() + 1, 77);
  r.xyz.assign(3 * P + 3, 77.0), r.obs.assign(2 * T + 2, 77);
  uint64_t n = 77, nm = 77;
  r.rc = dsm_tu_host_update_tracks(1, &cam_id, &cam, s.n, image_ids.data(), image_cams.data(), reg.data(), qvec.data(), tvec.data(), poff.data(),
                                   xy.data(), (uint32_t)s.pairs.size(), pair_ids.data(), moff.data(), matches.data(), (uint32_t)P, s.ids.data(),
                                   s.xyz.data(), s.toff.data(), s.tobs.data(), (uint32_t)steps.size(), steps.data(),
                                   selected ? selected->size() : 0, selected ? selected->data() : nullptr, next_id, &o, &n, r.ids.data(),
                                   r.xyz.data(), r.toff.data(), r.obs.data(), &nm, r.modified.data(), r.counts.data(), &r.rep);
  if (r.rc != DSM_OK) {  // a refusal leaves every output as it was
    EXPECT(n == 77 && nm == 77 && r.ids[0] == 77 && r.toff[0] == 77 && r.obs[0] == 77 && r.xyz[0] == 77.0 && r.counts[0] == 77);
    return r;
  }
  EXPECT(n <= P && nm <= n && r.ids[n] == 77 && r.toff[n + 1] == 77 && r.modified[nm] == 77 && r.counts[steps.size()] == 77);
  EXPECT(r.toff[n] <= T && r.obs[2 * r.toff[n]] == 77);
  r.ids.resize(n), r.toff.resize(n + 1), r.modified.resize(nm), r.counts.resize(steps.size()), r.xyz.resize(3 * n), r.obs.resize(2 * r.toff[n]);
  return r;
}

int main() {
  const int32_t M = DSM_TRACKS_MERGE, C = DSM_TRACKS_COMPLETE;
  {  // a0, a1 in the track, f2 .. f7 each behind the one before: the cap of 5 adds f2 .. f6 and never tests f7
    Scene s(8);
    Feat a0 = s.feat(0, 0.0), a1 = s.feat(1, 0.0), prev = a1;
    s.link(a0, a1);
    for (uint32_t i = 2; i < 8; ++i) {
      Feat f = s.feat(i, 0.0);
      s.link(prev, f);
      prev = f;
    }
    s.point(10, 0.0, {a0, a1});
    Result r = run(s, {C});
    EXPECT(r.rc == DSM_OK && r.ids == std::vector<uint64_t>{10} && r.counts == std::vector<uint64_t>{5} && r.toff[1] == 7);
    EXPECT(r.rep.complete_trials == 5 && r.modified == std::vector<uint64_t>{10});
    EXPECT(r.obs[2 * 6] == 3 * 6 + 1 && r.obs[2 * 6 + 1] == 0);
    r = run(s, {C}, nullptr, 1);
    EXPECT(r.rc == DSM_OK && r.counts == std::vector<uint64_t>{1} && r.toff[1] == 3 && r.rep.complete_trials == 1);
    EXPECT(run(s, {C}, nullptr, 0).rc == DSM_ERR_INVALID_ARGUMENT);
    EXPECT(run(s, {C, 2}).rc == DSM_ERR_INVALID_ARGUMENT);
    EXPECT(run(s, {C}, nullptr, 5, 10).rc == DSM_ERR_INVALID_ARGUMENT);  // next_point3D_id at an existing id
    const std::vector<uint64_t> twice{10, 10}, unknown{11};
    EXPECT(run(s, {C}, &twice).rc == DSM_ERR_INVALID_ARGUMENT && run(s, {C}, &unknown).rc == DSM_ERR_INVALID_ARGUMENT);
  }
  {  // A (3) + B (8) -> 13, the recursion takes C (12) -> 14; the count is the last merge's 6; then nothing is left for COMPLETE
    Scene s(6);
    Feat a0 = s.feat(0, 0.0), a1 = s.feat(1, 0.0), b2 = s.feat(2, 0.02), b3 = s.feat(3, 0.02), c4 = s.feat(4, 0.01), c5 = s.feat(5, 0.01);
    s.point(3, 0.0, {a0, a1});
    s.point(8, 0.02, {b2, b3});
    s.point(12, 0.01, {c4, c5});
    s.link(a1, b2);
    s.link(b3, c4);
    Result r = run(s, {M, C});
    EXPECT(r.rc == DSM_OK && r.ids == std::vector<uint64_t>{14} && r.counts == (std::vector<uint64_t>{6, 0}) && r.toff[1] == 6);
    EXPECT(r.rep.merge_trials == 2 && r.rep.num_merge_events == 2 && r.modified == std::vector<uint64_t>{14});
    const double m1 = (2.0 * 0.0 + 2.0 * 0.02) / 4.0, m2 = (4.0 * m1 + 2.0 * 0.01) / 6.0;
    EXPECT(r.xyz[0] == m2 && r.xyz[1] == 0.0);
    const uint32_t want[12] = {1, 0, 4, 0, 7, 0, 10, 0, 13, 0, 16, 0};
    EXPECT(r.obs.size() == 12 && std::memcmp(r.obs.data(), want, sizeof(want)) == 0);
    const std::vector<uint64_t> only_b{8};  // Merge(8) takes A through b2 first (-> 13: track b2 b3 a0 a1), then C by recursion
    r = run(s, {M}, &only_b, 5, 100);
    EXPECT(r.rc == DSM_OK && r.ids == std::vector<uint64_t>{101} && r.obs[0] == 7 && r.obs[4] == 1);
    // a feature in two tracks
    Scene t = s;
    t.tobs[4] = t.tobs[0], t.tobs[5] = t.tobs[1];
    EXPECT(run(t, {M}).rc == DSM_ERR_INVALID_ARGUMENT);
  }
  {  // 65 points in a chain: one component, 64 events, the ids 178 + 1 .. 178 + 64, one point of 130 elements left
    Scene s(130);
    Feat prev;
    for (uint32_t j = 0; j < 65; ++j) {
      Feat a = s.feat(2 * j, 0.0), b = s.feat(2 * j + 1, 0.0);
      s.point(50 + 2 * j, 0.0, {a, b});
      if (j) s.link(prev, a);
      prev = b;
    }
    for (const std::vector<int32_t>& steps : {std::vector<int32_t>{M}, std::vector<int32_t>{C, M}, std::vector<int32_t>{M, C, M}}) {
      Result r = run(s, steps);
      EXPECT(r.rc == DSM_OK && r.ids == std::vector<uint64_t>{178 + 64} && r.toff[1] == 130 && r.rep.num_merge_events == 64);
    }
  }
  {  // nothing at all
    Scene s(0);
    Result r = run(s, {C, M});
    EXPECT(r.rc == DSM_OK && r.ids.empty() && r.counts == (std::vector<uint64_t>{0, 0}));
  }
  if (failures) {
    std::printf("track_update_selftest: %d FAILED\n", failures);
    return 1;
  }
  std::printf("track_update_selftest: ok\n");
  return 0;
}
