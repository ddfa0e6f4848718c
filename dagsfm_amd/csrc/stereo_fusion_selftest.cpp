// stereo_fusion_selftest.cpp -- a stand-alone program over stereo_fusion_host.cpp (`make fusion-selftest` builds and runs it
// under -fsanitize=address,undefined): a fronto-parallel plane seen by shifted cameras of different sizes, with holes, at the
// defaults, with both limits firing, with an unused image and with the refused arguments.  Exit status 0 when every run gives
// points, a repeated run gives the same bytes and every refused call is refused; the sanitizers abort on anything else.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/dagsfm_mi355x.h"

extern "C" void dsm_fusion_host_default_options(dsm_stereo_fusion_options* o);
extern "C" int dsm_fusion_host_run(const dsm_stereo_fusion_options* options, uint32_t n_images, const dsm_fusion_image* images,
                                   const uint64_t* overlap_offsets, const uint32_t* overlap_images, uint64_t* n_points, uint64_t* n_traversals,
                                   const char** why);
extern "C" void dsm_fusion_host_get(dsm_fused_point* points, uint32_t* vis_bits, uint8_t* masks);

struct Maps {
  std::vector<float> depth, normal;
  std::vector<uint8_t> rgb;
};

int main() {
  const uint32_t n = 4;
  const uint32_t sizes[n][2] = {{37, 23}, {23, 37}, {65, 9}, {30, 26}};
  const float plane = 4.0f, focal = 40.0f;
  std::vector<Maps> maps(n);
  std::vector<dsm_fusion_image> images(n);
  uint32_t state = 12345;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t w = sizes[i][0], h = sizes[i][1], bw = i == 1 ? 2 * w : w, bh = i == 1 ? 2 * h : h;
    maps[i].depth.assign((size_t)w * h, plane);
    maps[i].normal.assign((size_t)3 * w * h, 0.0f);
    maps[i].rgb.resize((size_t)3 * bw * bh);
    for (size_t k = 0; k < (size_t)w * h; ++k) {
      maps[i].normal[2 * (size_t)w * h + k] = -1.0f;
      state = state * 1664525u + 1013904223u;
      if ((state >> 24) < 20) maps[i].depth[k] = 0.0f;  // a hole
    }
    for (auto& c : maps[i].rgb) {
      state = state * 1664525u + 1013904223u;
      c = (uint8_t)(state >> 24);
    }
    dsm_fusion_image& im = images[i];
    memset(&im, 0, sizeof(im));
    im.used = 1;
    im.width = w;
    im.height = h;
    im.bitmap_width = bw;
    im.bitmap_height = bh;
    im.row_stride = 3ull * bw;
    im.depth_map = maps[i].depth.data();
    im.normal_map = maps[i].normal.data();
    im.rgb = maps[i].rgb.data();
    // K [R | T] with R = I, T = (0.1 i, -0.05 i, 0): x_cam = x_world + T
    const float cx = 0.5f * (w - 1), cy = 0.5f * (h - 1), tx = 0.1f * i, ty = -0.05f * i;
    const float P[12] = {focal, 0, cx, focal * tx, 0, focal, cy, focal * ty, 0, 0, 1, 0};
    const float iP[12] = {1 / focal, 0, -cx / focal, -tx, 0, 1 / focal, -cy / focal, -ty, 0, 0, 1, 0};
    const float iR[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    memcpy(im.P, P, sizeof(P));
    memcpy(im.inv_P, iP, sizeof(iP));
    memcpy(im.inv_R, iR, sizeof(iR));
    im.bitmap_scale[0] = (float)w / bw;
    im.bitmap_scale[1] = (float)h / bh;
  }
  const uint64_t off[n + 1] = {0, 3, 6, 8, 9};
  const uint32_t ov[9] = {1, 2, 3, 0, 2, 3, 0, 1, 0};
  int bad = 0;
  for (int variant = 0; variant < 4; ++variant) {
    dsm_stereo_fusion_options o;
    dsm_fusion_host_default_options(&o);
    if (variant == 1) {
      o.max_num_pixels = 3;
      o.min_num_pixels = 2;
    }
    if (variant == 2) {
      o.max_traversal_depth = 2;
      o.min_num_pixels = 2;
    }
    images[2].used = variant == 3 ? 0 : 1;
    uint64_t np[2] = {0, 0}, nt = 0;
    std::vector<dsm_fused_point> pts[2];
    for (int rep = 0; rep < 2; ++rep) {
      const char* why = nullptr;
      if (dsm_fusion_host_run(&o, n, images.data(), off, ov, &np[rep], &nt, &why) != 0) {
        printf("variant %d refused: %s\n", variant, why ? why : "?");
        return 2;
      }
      pts[rep].resize(np[rep] + 1);
      std::vector<uint32_t> vis(np[rep] + 1);
      dsm_fusion_host_get(pts[rep].data(), vis.data(), nullptr);
      for (uint64_t k = 0; k < np[rep]; ++k)
        if (!vis[k] || vis[k] >> n) ++bad;
    }
    if (!np[0] || np[0] != np[1] || memcmp(pts[0].data(), pts[1].data(), np[0] * sizeof(dsm_fused_point))) ++bad;
    for (uint64_t k = 0; k < np[0]; ++k)
      if (fabsf(pts[0][k].z - plane) > 1e-3f || fabsf(pts[0][k].nz + 1.0f) > 1e-6f) ++bad;
    printf("stereo_fusion selftest: variant %d: %llu points, %llu traversals\n", variant, (unsigned long long)np[0], (unsigned long long)nt);
  }
  images[2].used = 1;
  // refused calls
  dsm_stereo_fusion_options o;
  dsm_fusion_host_default_options(&o);
  uint64_t np = 0;
  o.min_num_pixels = 0;
  if (dsm_fusion_host_run(&o, n, images.data(), off, ov, &np, nullptr, nullptr) != DSM_ERR_INVALID_ARGUMENT) ++bad;
  dsm_fusion_host_default_options(&o);
  o.max_depth_error = NAN;
  if (dsm_fusion_host_run(&o, n, images.data(), off, ov, &np, nullptr, nullptr) != DSM_ERR_INVALID_ARGUMENT) ++bad;
  const uint32_t ov_self[9] = {1, 2, 3, 1, 2, 3, 0, 1, 0};
  if (dsm_fusion_host_run(nullptr, n, images.data(), off, ov_self, &np, nullptr, nullptr) != DSM_ERR_INVALID_ARGUMENT) ++bad;
  maps[0].depth[5] = INFINITY;
  if (dsm_fusion_host_run(nullptr, n, images.data(), off, ov, &np, nullptr, nullptr) != DSM_ERR_INVALID_ARGUMENT) ++bad;
  maps[0].depth[5] = plane;
  if (dsm_fusion_host_run(nullptr, 0, nullptr, nullptr, nullptr, &np, nullptr, nullptr) != 0 || np != 0) ++bad;
  printf("stereo_fusion selftest: %d wrong\n", bad);
  return bad ? 1 : 0;
}
