// stereo_fusion_host.cpp -- the host build of stereo_fusion.h: StereoFusion::Run seed after seed on one CPU
// thread, from the text the kernels are built from.  What the CPU test holds to tests/stereo_fusion_ref.py bit for bit, the
// single-threaded baseline of tools/bench_stereo_fusion.py, and what `make fusion-selftest` runs under the sanitizers.  No HIP.
#include "stereo_fusion.h"

static std::vector<dsm_fused_point> g_points;
static std::vector<uint32_t> g_vis;  // [point][vis_words]
static std::vector<uint8_t> g_mask;
static uint32_t g_vis_words = 0;

extern "C" void dsm_fusion_host_default_options(dsm_stereo_fusion_options* o) { fusion_default_options(o); }

// 0, or DSM_ERR_INVALID_ARGUMENT / DSM_ERR_OUT_OF_RANGE with *why; the results stay for dsm_fusion_host_get
extern "C" int dsm_fusion_host_run(const dsm_stereo_fusion_options* options, uint32_t n_images, const dsm_fusion_image* images,
                                   const uint64_t* overlap_offsets, const uint32_t* overlap_images, uint64_t* n_points, uint64_t* n_traversals,
                                   const char** why) {
  dsm_stereo_fusion_options o;
  if (options)
    o = *options;
  else
    fusion_default_options(&o);
  FusionHostScene hs;
  bool out_of_range = false;
  const char* bad = fusion_prepare(o, n_images, images, overlap_offsets, overlap_images, &hs, &out_of_range);
  if (why) *why = bad;
  if (bad) return out_of_range ? DSM_ERR_OUT_OF_RANGE : DSM_ERR_INVALID_ARGUMENT;
  g_points.clear();
  g_vis.clear();
  g_mask.assign(hs.total_pixels, 0);
  g_vis_words = (n_images + 31) / 32;
  FusionScene& sc = hs.scene;
  sc.views = hs.views.data();
  sc.pix0 = hs.pix0.data();
  sc.overlap_off = hs.overlap_off.data();
  sc.overlap = hs.overlap.data();
  sc.depth = hs.depth.data();
  sc.normal = hs.normal.data();
  sc.rgb = hs.rgb.data();
  sc.mask = g_mask.data();
  const uint64_t list_cap = (uint64_t)o.max_num_pixels < hs.total_pixels ? (uint64_t)o.max_num_pixels : hs.total_pixels;
  const uint64_t stack_cap = list_cap * hs.max_list + 1;
  std::vector<uint32_t> list(list_cap + 1), stack_pix(stack_cap > list_cap ? stack_cap : list_cap + 1), stack_depth(stack_cap);
  FusionStore st = {list.data(), stack_pix.data(), stack_depth.data(), 1, (uint32_t)list_cap, (uint32_t)stack_cap};
  uint64_t traversals = 0;
  std::vector<dsm_fused_point> pts;
  std::vector<uint32_t> vis;
  for (uint32_t image : hs.order) {
    const FusionView& v = hs.views[image];
    const uint64_t n_pix = (uint64_t)v.w * v.h;
    if (!n_pix) continue;
    pts.resize(n_pix);
    vis.resize(n_pix * g_vis_words);
    uint64_t n = 0;
    static_assert(sizeof(FusionPoint) == sizeof(dsm_fused_point), "FusionPoint is dsm_fused_point");
    fusion_serial_image(sc, image, st, reinterpret_cast<FusionPoint*>(pts.data()), vis.data(), g_vis_words, &n, &traversals);
    g_points.insert(g_points.end(), pts.begin(), pts.begin() + n);
    g_vis.insert(g_vis.end(), vis.begin(), vis.begin() + n * g_vis_words);
  }
  if (n_points) *n_points = g_points.size();
  if (n_traversals) *n_traversals = traversals;
  return DSM_OK;
}

// the points, their visibility bits ([point][(n_images + 31) / 32] words) and the final masks ([total pixels], the used images'
// maps back to back in index order) of the last dsm_fusion_host_run; any pointer may be NULL
extern "C" void dsm_fusion_host_get(dsm_fused_point* points, uint32_t* vis_bits, uint8_t* masks) {
  if (points && !g_points.empty()) memcpy(points, g_points.data(), g_points.size() * sizeof(dsm_fused_point));
  if (vis_bits && !g_vis.empty()) memcpy(vis_bits, g_vis.data(), g_vis.size() * sizeof(uint32_t));
  if (masks && !g_mask.empty()) memcpy(masks, g_mask.data(), g_mask.size());
}
