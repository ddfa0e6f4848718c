// source_selection_selftest.cpp -- `make selection-selftest`: the host build of source_selection.h as a stand-alone program
// under the address and undefined-behaviour sanitizers.  A handful of tiny models through both host drivers (the sorted schedule
// and the reference's loops), which must agree byte for byte, and the small exact pieces at their edges.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dagsfm_mi355x.h"

extern "C" {
double dsm_ss_host_acos(double q);
void dsm_ss_host_default_options(dsm_source_selection_options* o);
void dsm_ss_host_decode_item(uint64_t t, uint64_t* i, uint64_t* j);
uint64_t dsm_ss_host_encode_item(uint64_t i, uint64_t j);
uint64_t dsm_ss_host_depth_index(uint64_t size, float factor);
uint64_t dsm_ss_host_percentile_index(float percentile, uint64_t n);
int dsm_ss_host_run(const dsm_source_selection_options*, uint32_t, const float*, const float*, uint64_t, const float*, const uint64_t*, const uint32_t*,
                    const uint8_t*, float*, uint64_t*, uint64_t*, uint64_t*, const char**);
int dsm_ss_host_run_serial(const dsm_source_selection_options*, uint32_t, const float*, const float*, uint64_t, const float*, const uint64_t*,
                           const uint32_t*, const uint8_t*, float*, uint64_t*, uint64_t*, uint64_t*, const char**);
void dsm_ss_host_get(uint64_t* list_off, uint32_t* list_img, dsm_image_overlap* pairs);
}

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

struct Model {
  std::vector<float> R, T, xyz;
  std::vector<uint64_t> off{0};
  std::vector<uint32_t> img;
  uint32_t n_images() const { return (uint32_t)(T.size() / 3); }
  void image(float cx, float cy, float cz) {  // identity rotation: T = -C
    const float r[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    R.insert(R.end(), r, r + 9);
    T.push_back(-cx), T.push_back(-cy), T.push_back(-cz);
  }
  void point(float x, float y, float z, std::vector<uint32_t> track) {
    xyz.push_back(x), xyz.push_back(y), xyz.push_back(z);
    img.insert(img.end(), track.begin(), track.end());
    off.push_back(img.size());
  }
};

struct Result {
  std::vector<float> ranges;
  std::vector<uint64_t> list_off, counters;
  std::vector<uint32_t> list_img;
  std::vector<dsm_image_overlap> pairs;
};

static Result run(const Model& m, const dsm_source_selection_options& o, const uint8_t* mask, bool serial) {
  Result r;
  const uint32_t n = m.n_images();
  const uint64_t n_points = m.off.size() - 1;
  r.ranges.assign(2 * (size_t)n + 1, 7.0f);
  r.counters.assign(3, 0);
  uint64_t n_list = 0, n_pairs = 0;
  const char* why = nullptr;
  const int rc = (serial ? dsm_ss_host_run_serial : dsm_ss_host_run)(&o, n, m.R.data(), m.T.data(), n_points, m.xyz.data(), m.off.data(), m.img.data(), mask,
                                                                    r.ranges.data(), &n_list, &n_pairs, r.counters.data(), &why);
  if (rc != DSM_OK) fprintf(stderr, "run failed (%d): %s\n", rc, why ? why : "");
  CHECK(rc == DSM_OK);
  r.ranges.resize(2 * (size_t)n);
  r.list_off.assign((size_t)n + 1, 0);
  r.list_img.assign(n_list + 1, 0);
  r.pairs.assign(n_pairs + 1, dsm_image_overlap());
  dsm_ss_host_get(r.list_off.data(), r.list_img.data(), r.pairs.data());
  r.list_img.resize(n_list);
  r.pairs.resize(n_pairs);
  return r;
}

static Result both(const Model& m, const dsm_source_selection_options& o, const uint8_t* mask = nullptr) {
  const Result a = run(m, o, mask, false), b = run(m, o, mask, true);
  CHECK(a.ranges.size() == b.ranges.size() && (a.ranges.empty() || !memcmp(a.ranges.data(), b.ranges.data(), a.ranges.size() * 4)));
  CHECK(a.list_off == b.list_off && a.list_img == b.list_img && a.counters == b.counters);
  CHECK(a.pairs.size() == b.pairs.size() && (a.pairs.empty() || !memcmp(a.pairs.data(), b.pairs.data(), a.pairs.size() * sizeof(dsm_image_overlap))));
  return a;
}

int main() {
  dsm_source_selection_options o;
  dsm_ss_host_default_options(&o);
  CHECK(o.max_num_src_images == 20 && o.triangulation_angle_percentile == 75.0f && o.min_triangulation_angle == 1.0);

  {  // the empty model
    Model m;
    const Result r = both(m, o);
    CHECK(r.list_off.size() == 1 && r.list_off[0] == 0 && r.pairs.empty() && r.counters[0] == 0);
  }
  {  // images, no points
    Model m;
    m.image(0, 0, 0), m.image(1, 0, 0);
    const Result r = both(m, o);
    CHECK(r.ranges[0] == -1.0f && r.ranges[3] == -1.0f && r.list_off[2] == 0 && r.pairs.empty());
  }
  {  // an image without points, a track of length 1, an empty track, an image repeated in a track
    Model m;
    m.image(0, 0, 0), m.image(1, 0, 0), m.image(0, 1, 0), m.image(5, 5, 5);
    m.point(0.5f, 0.5f, 4.0f, {0});
    m.point(0.5f, 0.5f, 3.0f, {});
    m.point(0.2f, 0.1f, 5.0f, {0, 1, 0});
    m.point(0.1f, 0.3f, 6.0f, {1, 2, 0});
    m.point(0.0f, 0.0f, -2.0f, {2, 2});
    const Result r = both(m, o);
    CHECK(r.counters[0] == 2 + 3 && r.counters[1] == 3 && r.counters[2] == 0);
    CHECK(r.pairs[0].a == 0 && r.pairs[0].b == 1 && r.pairs[0].count == 3);
    CHECK(r.ranges[6] == -1.0f && r.ranges[7] == -1.0f);  // image 3 is in no track
    CHECK(r.ranges[0] == 4.0f * 0.75f && r.ranges[1] == 6.0f * 1.25f);  // depths 4 5 5 6: indices 0 and 3
    CHECK(r.list_off[1] == 2 && r.list_img[0] == 1 && r.list_img[1] == 2);  // 3 shared points before 1
    CHECK(r.list_off[4] - r.list_off[3] == 0);
    const uint8_t mask[4] = {1, 0, 1, 1};
    const Result k = both(m, o, mask);
    CHECK(k.list_off[1] == 1 && k.list_img[0] == 2);
    o.max_num_src_images = 0;
    CHECK(both(m, o).list_off[4] == 0);
    o.max_num_src_images = 1;
    CHECK(both(m, o).list_off[4] == 3);
    o.max_num_src_images = 20;
    o.min_triangulation_angle = 60.0;
    CHECK(both(m, o).list_off[4] == 0);
    o.min_triangulation_angle = 1.0;
  }
  {  // a point on the line through two centres beyond both, one at a centre, two images with one centre; ties to the lower index
    Model m;
    m.image(0, 0, 0), m.image(1, 0, 0), m.image(1, 0, 0), m.image(0, 2, 0);
    m.point(3.0f, 0.0f, 0.0f, {0, 1});
    m.point(0.0f, 0.0f, 0.0f, {0, 1, 2, 3});
    m.point(0.3f, 0.7f, 2.0f, {3, 2, 1, 0});
    o.min_triangulation_angle = 0.0;
    for (float p : {0.0f, 33.0f, 50.0f, 75.0f, 100.0f}) {
      o.triangulation_angle_percentile = p;
      const Result r = both(m, o);
      CHECK(r.list_off[4] - r.list_off[3] == 3 && r.list_img[r.list_off[3]] == 0 && r.list_img[r.list_off[3] + 1] == 1 && r.list_img[r.list_off[3] + 2] == 2);
    }
    o.triangulation_angle_percentile = 75.0f;
    o.min_triangulation_angle = 1.0;
  }

  // the small pieces
  for (uint64_t L : {2ull, 3ull, 64ull, 363ull}) {
    uint64_t t = 0;
    for (uint64_t i = 1; i < L; ++i)
      for (uint64_t j = 0; j < i; ++j, ++t) {
        uint64_t di, dj;
        dsm_ss_host_decode_item(t, &di, &dj);
        CHECK(di == i && dj == j && dsm_ss_host_encode_item(i, j) == t);
      }
  }
  {
    const uint64_t i = 4294967295ull, top = dsm_ss_host_encode_item(i, i - 1);  // the last item of the longest track
    uint64_t di, dj;
    dsm_ss_host_decode_item(top, &di, &dj);
    CHECK(di == i && dj == i - 1);
    dsm_ss_host_decode_item(0, &di, &dj);
    CHECK(di == 1 && dj == 0);
  }
  CHECK(dsm_ss_host_depth_index(100, 0.01f) == 1 && dsm_ss_host_depth_index(1, 0.99f) == 0 && dsm_ss_host_depth_index(100, 0.99f) == 99);
  CHECK(dsm_ss_host_percentile_index(75.0f, 1) == 0 && dsm_ss_host_percentile_index(75.0f, 3) == 2 && dsm_ss_host_percentile_index(50.0f, 4) == 2);
  CHECK(dsm_ss_host_acos(1.0) == 0.0 && dsm_ss_host_acos(-1.0) == M_PI && dsm_ss_host_acos(0.0) == M_PI / 2 && std::isnan(dsm_ss_host_acos(1.0000000000000002)));
  for (int k = -1000; k <= 1000; ++k) {
    const double q = k / 1000.0, a = dsm_ss_host_acos(q), b = std::acos(q);
    CHECK(std::fabs(a - b) <= std::fabs(b) * 2.3e-16);
  }
  printf("source_selection_selftest ok\n");
  return 0;
}
