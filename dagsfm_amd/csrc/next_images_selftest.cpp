// next_images_selftest.cpp -- the host build of next_images.h (next_images_host.cpp) as a stand-alone program under the address
// and undefined-behaviour sanitizers (`make next-images-selftest`): the pieces at their edges, a small call in both schedules of
// the ranking with the answers worked out by hand, word-edge image sizes, and the refusals with their untouched outputs.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dagsfm_mi355x.h"

extern "C" {
void dsm_ni_host_default_options(dsm_next_images_options* o);
uint32_t dsm_ni_host_cell(double x, uint64_t extent);
uint64_t dsm_ni_host_score(const double* xy, uint64_t n, uint64_t width, uint64_t height);
float dsm_ni_host_rank(int32_t method, uint32_t num_visible, uint32_t num_observations, uint64_t score);
uint64_t dsm_ni_host_key(uint32_t flags, int eligible, float rank, uint32_t image_id);
int dsm_ni_host_find_next_images(uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images,
                                 const uint32_t* image_ids, const uint32_t* image_camera_ids, const uint32_t* points2D_offsets,
                                 const double* points2D_xy, uint32_t num_pairs, const uint32_t* pair_image_ids, const uint64_t* match_offsets,
                                 const uint32_t* matches, uint32_t num_problems, const uint32_t* problem_image_offsets,
                                 const uint32_t* problem_image_ids, const uint8_t* slot_registered, const uint64_t* slot_obs_offsets,
                                 const int32_t* slot_obs_point3D, const uint32_t* slot_num_reg_trials, const uint8_t* slot_filtered,
                                 const dsm_next_images_options* options, int sorted, uint64_t* next_offsets, uint32_t* next_image_ids,
                                 uint64_t next_capacity, uint32_t* slot_num_visible, uint32_t* slot_num_observations, uint64_t* slot_score,
                                 const char** why);
uint64_t dsm_lb_host_percentile_index(uint64_t n);
double dsm_lb_host_percentile(const double* a, uint64_t n);
int dsm_lb_host_find_local_bundles(uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets, uint32_t num_problems,
                                   const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids, const uint8_t* slot_registered,
                                   const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D, const double* slot_qvec,
                                   const double* slot_tvec, const uint64_t* point_offsets, const double* point_xyz, uint32_t num_queries,
                                   const uint32_t* query_problem, const uint32_t* query_image_id,
                                   const dsm_local_bundle_selection_options* options, uint64_t* bundle_offsets, uint32_t* bundle_image_ids,
                                   uint64_t bundle_capacity, uint64_t* overlap_offsets, uint32_t* overlap_image_ids, uint32_t* overlap_shared,
                                   double* overlap_tri_angle, uint64_t overlap_capacity, double* margin, const char** why);
}

static int failures = 0;
#define EXPECT(cond)                                                       \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
      ++failures;                                                          \
    }                                                                      \
  } while (0)

struct Scene {
  std::vector<uint32_t> cam_ids{1};
  std::vector<dsm_camera> cams;
  std::vector<uint32_t> image_ids, image_cams, poff{0}, pairs, matches, prob_off{0}, prob_ids, trials;
  std::vector<double> xy;
  std::vector<uint64_t> moff{0}, obs_off{0};
  std::vector<uint8_t> registered, filtered;
  std::vector<int32_t> obs;
  dsm_next_images_options o;
  Scene() {
    dsm_camera c;
    std::memset(&c, 0, sizeof(c));
    c.width = 640, c.height = 480;
    cams.push_back(c);
    dsm_ni_host_default_options(&o);
  }
  void image(uint32_t id, uint32_t n) {
    image_ids.push_back(id), image_cams.push_back(1);
    for (uint32_t f = 0; f < n; ++f) xy.push_back(10.0 * (f % 64) + 0.5), xy.push_back(7.0 * (f / 64) + 0.25);
    poff.push_back(poff.back() + n);
  }
  uint32_t count(uint32_t id) const {
    for (size_t i = 0; i < image_ids.size(); ++i)
      if (image_ids[i] == id) return poff[i + 1] - poff[i];
    return 0;
  }
  void pair(uint32_t a, uint32_t b, const std::vector<uint32_t>& m) {
    pairs.push_back(a), pairs.push_back(b);
    matches.insert(matches.end(), m.begin(), m.end());
    moff.push_back(moff.back() + m.size() / 2);
  }
  // a slot of the open problem: the first n_points observations of a registered image have a point
  void slot(uint32_t id, bool reg, uint32_t n_points, uint32_t tr = 0, bool filt = false) {
    prob_ids.push_back(id), registered.push_back(reg), trials.push_back(tr), filtered.push_back(filt);
    const uint32_t n = count(id);
    for (uint32_t f = 0; f < n; ++f) obs.push_back(f < n_points ? (int32_t)f : -1);
    obs_off.push_back(obs_off.back() + n);
  }
  void close_problem() { prob_off.push_back((uint32_t)prob_ids.size()); }
  struct Out {
    int rc;
    const char* why;
    std::vector<uint64_t> off, score;
    std::vector<uint32_t> ids, nv, no;
  };
  Out run(int sorted, uint64_t capacity = ~0ull) const {
    Out r;
    const size_t S = prob_ids.size(), P = prob_off.size() - 1;
    r.off.assign(P + 1, 0), r.ids.assign(S + 1, 0), r.nv.assign(S + 1, 0), r.no.assign(S + 1, 0), r.score.assign(S + 1, 0);
    r.why = nullptr;
    // (every array is passed with its exact size, so that an access one past an end is the sanitizer's to find)
    r.rc = dsm_ni_host_find_next_images(1, cam_ids.data(), cams.data(), (uint32_t)image_ids.size(), image_ids.data(), image_cams.data(), poff.data(),
                                        xy.data(), (uint32_t)moff.size() - 1, pairs.data(), moff.data(), matches.data(), (uint32_t)P, prob_off.data(),
                                        prob_ids.data(), registered.data(), obs_off.data(), obs.data(), trials.data(), filtered.data(), &o, sorted,
                                        r.off.data(), r.ids.data(), capacity == ~0ull ? S : capacity, r.nv.data(), r.no.data(), r.score.data(), &r.why);
    return r;
  }
};

static std::vector<uint32_t> identity(uint32_t n) {
  std::vector<uint32_t> m;
  for (uint32_t k = 0; k < n; ++k) m.push_back(k), m.push_back(k);
  return m;
}

int main() {
  // the pieces
  EXPECT(dsm_ni_host_cell(0.0, 640) == 0 && dsm_ni_host_cell(10.0, 640) == 1 && dsm_ni_host_cell(9.999999, 640) == 0);
  EXPECT(dsm_ni_host_cell(640.0, 640) == 63 && dsm_ni_host_cell(1e300, 640) == 63 && dsm_ni_host_cell(1.7e308, 640) == 63);
  EXPECT(dsm_ni_host_cell(639.999, 640) == 63 && dsm_ni_host_cell(630.0, 640) == 63 && dsm_ni_host_cell(629.9999, 640) == 62);
  {
    std::vector<double> full;
    for (int y = 0; y < 64; ++y)
      for (int x = 0; x < 64; ++x) full.push_back(x + 0.5), full.push_back(y + 0.5);
    EXPECT(dsm_ni_host_score(full.data(), 4096, 64, 64) == 17895696ull);
    EXPECT(dsm_ni_host_score(full.data(), 1, 64, 64) == 5460ull);
    EXPECT(dsm_ni_host_score(full.data(), 0, 64, 64) == 0ull);
    EXPECT(dsm_ni_host_score(full.data(), 2, 64, 64) == 5460ull + 4096ull);  // neighbours share every coarser cell
  }
  EXPECT(dsm_ni_host_rank(1, 1, 3, 0) == 1.0f / 3.0f && dsm_ni_host_rank(0, 262144, 1, 0) == 262144.0f);
  EXPECT(dsm_ni_host_key(0, 1, 5.0f, 9) < dsm_ni_host_key(0, 1, 4.5f, 1) && dsm_ni_host_key(0, 1, 4.5f, 1) < dsm_ni_host_key(0, 1, 4.5f, 2));
  EXPECT(dsm_ni_host_key(0, 1, 0.25f, 0xfffffffeu) < dsm_ni_host_key(2, 1, 1e9f, 0) && dsm_ni_host_key(2, 1, 1e-30f, 5) < dsm_ni_host_key(0, 0, 1.0f, 5));

  // a star: image 100 registered with points on all of its points2D; candidates of the word-edge sizes matched one to one
  const uint32_t sizes[] = {0, 1, 31, 32, 33, 63, 64, 65, 257};
  Scene s;
  s.image(100, 257);
  for (uint32_t k = 0; k < 9; ++k) s.image(k + 1, sizes[k]);
  for (uint32_t k = 1; k < 9; ++k) {
    if (k % 2)
      s.pair(100, k + 1, identity(sizes[k]));
    else
      s.pair(k + 1, 100, identity(sizes[k]));
  }
  for (uint32_t k = 9; k-- > 0;) s.slot(k + 1, false, 0, k == 4 ? 1 : 0, k == 6);
  s.slot(100, true, 257);
  s.close_problem();
  s.slot(100, true, 40);  // a second problem on the same images in another state: 40 points, and image 9 registered without points
  s.slot(9, true, 0);
  s.slot(6, false, 0);
  s.slot(3, false, 0);
  s.close_problem();
  s.close_problem();  // an empty problem
  s.o.abs_pose_min_num_inliers = 31;
  s.o.image_selection_method = DSM_NEXT_IMAGE_MAX_VISIBLE_POINTS_NUM;
  for (int sorted = 0; sorted < 2; ++sorted) {
    const Scene::Out r = s.run(sorted);
    EXPECT(r.rc == DSM_OK);
    // first bucket by count descending: 9 (257), 8 (65), 6 (63), 4 (32), 3 (31); second bucket: 7 (64, filtered), 5 (33, tried)
    const uint32_t want[] = {9, 8, 6, 4, 3, 7, 5};
    EXPECT(r.off[0] == 0 && r.off[1] == 7);
    for (int i = 0; i < 7; ++i) EXPECT(r.ids[i] == want[i]);
    for (uint32_t k = 0; k < 9; ++k) EXPECT(r.nv[8 - k] == sizes[k] && r.no[8 - k] == sizes[k]);
    EXPECT(r.nv[9] == 0 && r.no[9] == 257 && r.score[9] == 0);
    EXPECT(r.off[2] == 9 && r.ids[7] == 6 && r.ids[8] == 3 && r.off[3] == 9);  // 40 of image 6's 63 points2D are visible, all 31 of image 3's: 31 >= 31
    EXPECT(r.nv[12] == 40 && r.no[12] == 63 && r.nv[13] == 31);
  }
  {  // the ratio: every candidate sees all it observes, so the ids decide inside a bucket
    Scene t = s;
    t.o.image_selection_method = DSM_NEXT_IMAGE_MAX_VISIBLE_POINTS_RATIO;
    const Scene::Out a = t.run(0), b = t.run(1);
    const uint32_t want[] = {3, 4, 6, 8, 9, 5, 7};
    EXPECT(a.rc == DSM_OK && b.rc == DSM_OK && a.ids == b.ids && a.off == b.off);
    for (int i = 0; i < 7; ++i) EXPECT(a.ids[i] == want[i]);
  }
  {  // refusals leave the outputs untouched
    auto untouched = [](const Scene::Out& r) {
      for (uint64_t x : r.off)
        if (x) return false;
      for (uint32_t x : r.ids)
        if (x) return false;
      for (uint32_t x : r.nv)
        if (x) return false;
      for (uint64_t x : r.score)
        if (x) return false;
      return true;
    };
    Scene t = s;
    t.xy[2 * t.poff[3]] = -1.0;  // image 3 is a candidate
    Scene::Out r = t.run(0);
    EXPECT(r.rc == DSM_ERR_INVALID_ARGUMENT && r.why && untouched(r));
    t = s;
    t.xy[0] = -1.0;  // image 100 is registered everywhere: accepted
    EXPECT(t.run(0).rc == DSM_OK);
    t = s;
    t.obs[0] = 3;  // a point on a slot that is not registered
    r = t.run(1);
    EXPECT(r.rc == DSM_ERR_INVALID_ARGUMENT && untouched(r));
    t = s;
    t.obs_off[1] += 1;
    r = t.run(0);
    EXPECT(r.rc == DSM_ERR_INVALID_ARGUMENT && untouched(r));
    t = s;
    t.o.max_reg_trials = 0;
    r = t.run(0);
    EXPECT(r.rc == DSM_ERR_INVALID_ARGUMENT && untouched(r));
    r = s.run(0, 7);
    EXPECT(r.rc == DSM_ERR_OUT_OF_RANGE && untouched(r));
    r = s.run(1, 8);
    EXPECT(r.rc == DSM_ERR_OUT_OF_RANGE && untouched(r));
    EXPECT(s.run(1, 9).rc == DSM_OK);
  }
  // ---------------------------------------------------------------- the local bundles
  EXPECT(dsm_lb_host_percentile_index(1) == 0 && dsm_lb_host_percentile_index(2) == 1 && dsm_lb_host_percentile_index(3) == 2);
  EXPECT(dsm_lb_host_percentile_index(4) == 2 && dsm_lb_host_percentile_index(5) == 3 && dsm_lb_host_percentile_index(7) == 5);
  {
    const double a[5] = {0.5, 0.125, 0.75, 0.25, 0.125};
    EXPECT(dsm_lb_host_percentile(a, 5) == 0.5 && dsm_lb_host_percentile(a, 1) == 0.5 && dsm_lb_host_percentile(a, 2) == 0.5);
  }
  {
    // four images at x = 0, 1, 0.2, 0.05 looking down z, eight points at depth 10; the query (id 5) sees all of them, image 6
    // all, image 7 six of them, image 8 one; point 0 twice in the query
    const uint32_t image_ids[4] = {5, 6, 7, 8}, poff[5] = {0, 10, 20, 30, 40}, prob_off[2] = {0, 4}, prob_ids[4] = {8, 7, 6, 5};
    const uint8_t reg[4] = {1, 1, 1, 1};
    const uint64_t obs_off[5] = {0, 10, 20, 30, 40}, pt_off[2] = {0, 8};
    std::vector<int32_t> obs(40, -1);
    obs[3] = 2;                                         // image 8
    for (int k = 0; k < 6; ++k) obs[10 + k] = k;        // image 7
    for (int k = 0; k < 8; ++k) obs[20 + k + 1] = k;    // image 6
    for (int k = 0; k < 8; ++k) obs[30 + k] = k;        // image 5, the query
    obs[39] = 0;
    std::vector<double> qv(16, 0.0), tv(12, 0.0), xyz(24);
    const double cx[4] = {0.05, 0.2, 1.0, 0.0};
    for (int k = 0; k < 4; ++k) qv[4 * k] = 1.0 + k, tv[3 * k] = -cx[k];
    for (int k = 0; k < 8; ++k) xyz[3 * k] = 0.1 * k - 0.4, xyz[3 * k + 1] = 0.05 * k, xyz[3 * k + 2] = 10.0;
    const uint32_t q_prob[1] = {0}, q_img[1] = {5};
    dsm_local_bundle_selection_options o = {3, 6.0};
    uint64_t boff[2] = {0, 0}, ooff[2] = {0, 0};
    uint32_t bids[2] = {0, 0}, oids[3] = {0, 0, 0}, oshared[3] = {0, 0, 0};
    double oangle[3] = {0, 0, 0}, margin = 0;
    const char* why = nullptr;
    int rc = dsm_lb_host_find_local_bundles(4, image_ids, poff, 1, prob_off, prob_ids, reg, obs_off, obs.data(), qv.data(), tv.data(), pt_off, xyz.data(), 1,
                                            q_prob, q_img, &o, boff, bids, 2, ooff, oids, oshared, oangle, 3, &margin, &why);
    EXPECT(rc == DSM_OK);
    // shared: image 6 sees the eight points, point 0 counted twice = 9; image 7: 6 + 1 = 7; image 8: 1
    EXPECT(ooff[1] == 3 && oids[0] == 6 && oids[1] == 7 && oids[2] == 8 && oshared[0] == 9 && oshared[1] == 7 && oshared[2] == 1);
    // NumPoints3D = 9; image 6 (about 5.7 degrees) fails the first threshold, passes the second; image 7 (about 1.1) the eighth
    EXPECT(boff[1] == 2 && bids[0] == 6 && bids[1] == 7 && oangle[0] > 0.09 && oangle[0] < 0.1047 && oangle[1] > 0.0175 && oangle[1] < 0.0209);
    EXPECT(oangle[2] > 0.004 && oangle[2] < 0.006 && margin > 1e-9);  // 1 >= 0.1 * 9: image 8 is reachable, its angle is reported
    uint32_t small[1] = {0};
    boff[1] = 0;
    rc = dsm_lb_host_find_local_bundles(4, image_ids, poff, 1, prob_off, prob_ids, reg, obs_off, obs.data(), qv.data(), tv.data(), pt_off, xyz.data(), 1,
                                        q_prob, q_img, &o, boff, small, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &why);
    EXPECT(rc == DSM_ERR_OUT_OF_RANGE && boff[1] == 0 && small[0] == 0);
    obs[5] = 8;  // a point index outside the problem's points
    rc = dsm_lb_host_find_local_bundles(4, image_ids, poff, 1, prob_off, prob_ids, reg, obs_off, obs.data(), qv.data(), tv.data(), pt_off, xyz.data(), 1,
                                        q_prob, q_img, &o, boff, small, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &why);
    EXPECT(rc == DSM_ERR_INVALID_ARGUMENT && why && boff[1] == 0);
  }
  if (failures) {
    std::printf("next_images_selftest: %d check(s) failed\n", failures);
    return 1;
  }
  std::printf("next_images_selftest ok\n");
  return 0;
}
