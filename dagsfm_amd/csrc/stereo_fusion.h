// stereo_fusion.h -- StereoFusion::Fuse (src/mvs/fusion.cc:295-473) for ONE seed, written once as host + device code
// (DESIGN.md 26).  The device schedules of stereo_fusion.hip (speculate / claim / commit, and the check build's serial lane) and
// the host build stereo_fusion_host.cpp are all built from this text, so what the host build computes is what the kernels
// compute.  tests/stereo_fusion_ref.py is the normative restatement; no contraction (-ffp-contract=off in every build).
//
// A pixel is named by its GLOBAL index g = pix0[image] + row * width + col over the maps of all images, back to back.
#ifndef DAGSFM_AMD_CSRC_STEREO_FUSION_H_
#define DAGSFM_AMD_CSRC_STEREO_FUSION_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DSM_FUSION_HD __host__ __device__ inline
#else
#define DSM_FUSION_HD inline
#endif

#define DSM_FUSION_LIMIT 1u     // the max_num_pixels break or the max_traversal_depth continue fired: the traversal order mattered
#define DSM_FUSION_OVERFLOW 2u  // the storage was too small: the recorded list is not the traversal's

struct FusionView {  // one image; an unused image has w = h = 0
  float P[12], inv_P[12], inv_R[9], scale[2];
  uint64_t rgb0, rgb_stride;  // first byte of the bitmap in FusionScene::rgb, bytes per row
  uint32_t pix0;              // global index of pixel (0, 0)
  int32_t w, h, bw, bh;       // the maps' size, the bitmap's size
  int32_t used;
  uint32_t order_pos;         // place in the FindNextImage order (:58-79); fused_images_[i] <=> order_pos < the current place
  uint32_t reserved;
};

struct FusionScene {
  const FusionView* views;
  const uint32_t* pix0;          // [n_images + 1]
  const uint64_t* overlap_off;   // [n_images + 1]
  const uint32_t* overlap;       // overlapping_images_, lists back to back
  const float* depth;            // [total pixels]
  const float* normal;           // [total pixels][3], the image's frame
  const uint8_t* rgb;            // the bitmaps, back to back
  uint8_t* mask;                 // [total pixels] fused_pixel_masks_
  uint32_t n_images;
  int32_t min_num_pixels, max_num_pixels, max_traversal_depth;
  double max_depth_error;                   // compared in double with the float error, as written (:343)
  float max_squared_reproj_error, min_cos_normal_error;  // rounded to float on the host (fusion.h:142-143)
};

// the storage of one traversal: the accepted pixels and the LIFO queue, element k at base[k * stride]
struct FusionStore {
  uint32_t* list;
  uint32_t* stack_pix;
  uint32_t* stack_depth;
  uint64_t stride;
  uint32_t list_cap, stack_cap;
  uint64_t* seen;  // speculation only, or nullptr: a word per image, element i at seen[i * stride] (fusion_window_bit)
};

struct FusionPoint {  // PlyPoint (src/util/ply.h:45-55)
  float x, y, z, nx, ny, nz;
  uint8_t r, g, b, pad;
};

DSM_FUSION_HD uint32_t fusion_image_of(const FusionScene& sc, uint32_t g) {
  uint32_t lo = 0, hi = sc.n_images;  // the image with pix0[i] <= g < pix0[i + 1]; empty images share a pix0 and never match
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (sc.pix0[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// a row of P * (v0, v1, v2, v3), summed left to right (Eigen fixes no order: DESIGN.md 26)
DSM_FUSION_HD float fusion_row4(const float* m, float v0, float v1, float v2, float v3) { return ((m[0] * v0 + m[1] * v1) + m[2] * v2) + m[3] * v3; }
DSM_FUSION_HD float fusion_row3(const float* m, float v0, float v1, float v2) { return (m[0] * v0 + m[1] * v1) + m[2] * v2; }

// std::round of a projected coordinate as an index below `size`; NaN, negative or not below 2^31 in magnitude: outside (-1)
DSM_FUSION_HD int32_t fusion_round_index(double x, int32_t size) {
  const double r = round(x);  // half away from zero
  if (!(r >= 0.0) || !(r < 2147483648.0)) return -1;
  const int32_t i = (int32_t)r;
  return i < size ? i : -1;
}

// xyz (:373-375) and the global normal (:359-362) of pixel (row, col) of view v with its depth
DSM_FUSION_HD void fusion_xyz_normal(const FusionScene& sc, const FusionView& v, uint32_t g, int32_t row, int32_t col, float depth, float* xyz, float* normal) {
  const float* n = sc.normal + 3 * (uint64_t)g;
  for (int r = 0; r < 3; ++r) normal[r] = fusion_row3(v.inv_R + 3 * r, n[0], n[1], n[2]);
  const float a = (float)col * depth, b = (float)row * depth;
  for (int r = 0; r < 3; ++r) xyz[r] = fusion_row4(v.inv_P + 4 * r, a, b, depth, 1.0f);
}

// InterpolateNearestNeighbor(col / scale_x, row / scale_y) (:378-381): a float division, a double round; outside: (0, 0, 0)
DSM_FUSION_HD void fusion_colour(const FusionScene& sc, const FusionView& v, int32_t row, int32_t col, uint8_t* rgb) {
  const int32_t xx = fusion_round_index((double)((float)col / v.scale[0]), v.bw);
  const int32_t yy = fusion_round_index((double)((float)row / v.scale[1]), v.bh);
  rgb[0] = rgb[1] = rgb[2] = 0;
  if (xx < 0 || yy < 0) return;
  const uint8_t* p = sc.rgb + v.rgb0 + (uint64_t)yy * v.rgb_stride + 3 * (uint64_t)xx;
  rgb[0] = p[0];
  rgb[1] = p[1];
  rgb[2] = p[2];
}

// A pixel can pass the reprojection test (:348-354) only within max_reproj_error of the reference point's projection, so for
// max_reproj_error <= 2.4 every pixel a seed accepts in one image lies in the 7 x 7 window around the rounded projection: its
// place there, 0 .. 48, or -1 outside the window (which the test then rejects: |col - p| <= 2.4 (1 + eps) and |p - round(p)| <=
// 0.5 leave |col - round(p)| <= 2).  A speculating seed keeps "already mine" as one bit per place and image instead of
// searching its list.
#define DSM_FUSION_WINDOW_MAX_SQUARED_ERROR 5.76f
DSM_FUSION_HD int fusion_window_bit(float px, float py, int32_t col, int32_t row) {
  const float dx = (float)col - roundf(px), dy = (float)row - roundf(py);
  if (!(fabsf(dx) <= 3.0f) || !(fabsf(dy) <= 3.0f)) return -1;
  return ((int)dy + 3) * 7 + ((int)dx + 3);
}

// The while loop of Fuse() (:312-437) for the seed g0.
// SPECULATE = false: the reference's loop -- an accepted pixel is marked in sc.mask at once; the store has room for
//   max_num_pixels pixels and for every push.
// SPECULATE = true: sc.mask is only read (the committed masks); the marks this seed would make are its list so far.  A store
//   that is too small ends the traversal with DSM_FUSION_OVERFLOW.  A child that is masked, that the reprojection test is bound
//   to reject or that is already the seed's is not pushed: its pop would drop it all the same, whenever it came.
// Returns the number of accepted pixels (list[0 .. n)); *flags gets DSM_FUSION_LIMIT / DSM_FUSION_OVERFLOW.
template <bool SPECULATE>
DSM_FUSION_HD uint32_t fusion_traverse(const FusionScene& sc, uint32_t cur_pos, uint32_t g0, const FusionStore& st, uint32_t* flags) {
  uint32_t n = 0, sp = 0, fl = 0;
  const bool window = SPECULATE && st.seen && sc.max_squared_reproj_error <= DSM_FUSION_WINDOW_MAX_SQUARED_ERROR;
  float ref[3] = {0.0f, 0.0f, 0.0f}, ref_n[3] = {0.0f, 0.0f, 0.0f};
  if (window)
    for (uint32_t i = 0; i < sc.n_images; ++i) st.seen[i * st.stride] = 0;
  st.stack_pix[0] = g0;
  st.stack_depth[0] = 0;
  sp = 1;
  while (sp > 0) {
    --sp;
    const uint32_t g = st.stack_pix[sp * st.stride];
    const uint32_t td = st.stack_depth[sp * st.stride];
    if (sc.mask[g]) continue;
    if (SPECULATE && td > 0 && g == g0) continue;  // the seed itself, accepted first
    if (SPECULATE && !window) {
      bool mine = false;
      for (uint32_t k = 0; k < n && !mine; ++k) mine = st.list[k * st.stride] == g;
      if (mine) continue;
    }
    const uint32_t image = fusion_image_of(sc, g);
    const FusionView& v = sc.views[image];
    const uint32_t local = g - v.pix0;
    const int32_t row = (int32_t)(local / (uint32_t)v.w), col = (int32_t)(local % (uint32_t)v.w);
    const float depth = sc.depth[g];
    if (depth <= 0.0f) continue;
    int bit = -1;
    if (td > 0) {
      const float p0 = fusion_row4(v.P + 0, ref[0], ref[1], ref[2], 1.0f);
      const float p1 = fusion_row4(v.P + 4, ref[0], ref[1], ref[2], 1.0f);
      const float p2 = fusion_row4(v.P + 8, ref[0], ref[1], ref[2], 1.0f);
      const float depth_error = fabsf((p2 - depth) / depth);
      if (!((double)depth_error <= sc.max_depth_error)) continue;  // a NaN fails the test
      const float col_diff = p0 / p2 - (float)col;
      const float row_diff = p1 / p2 - (float)row;
      const float squared_reproj_error = col_diff * col_diff + row_diff * row_diff;
      if (!(squared_reproj_error <= sc.max_squared_reproj_error)) continue;
      if (window) bit = fusion_window_bit(p0 / p2, p1 / p2, col, row);
    }
    float xyz[3], normal[3];
    fusion_xyz_normal(sc, v, g, row, col, depth, xyz, normal);
    if (td > 0) {
      const float cos_normal_error = (ref_n[0] * normal[0] + ref_n[1] * normal[1]) + ref_n[2] * normal[2];
      if (!(cos_normal_error >= sc.min_cos_normal_error)) continue;
    }
    if (window && td > 0) {  // "already mine" comes after the tests here; either way the pixel is dropped without a trace
      bool mine = false;
      if (bit >= 0)
        mine = (st.seen[image * st.stride] >> bit) & 1u;
      else
        for (uint32_t k = 0; k < n && !mine; ++k) mine = st.list[k * st.stride] == g;
      if (mine) continue;
    }
    if (n >= st.list_cap) {
      fl |= DSM_FUSION_OVERFLOW | DSM_FUSION_LIMIT;
      break;
    }
    if (window && bit >= 0) st.seen[image * st.stride] |= 1ull << bit;
    if (!SPECULATE) sc.mask[g] = 1;
    st.list[n * st.stride] = g;
    ++n;
    if (td == 0)
      for (int r = 0; r < 3; ++r) {
        ref[r] = xyz[r];
        ref_n[r] = normal[r];
      }
    if (n >= (uint32_t)sc.max_num_pixels) {
      fl |= DSM_FUSION_LIMIT;
      break;
    }
    const uint32_t next_td = td + 1;
    if (next_td >= (uint32_t)sc.max_traversal_depth) {
      fl |= DSM_FUSION_LIMIT;
      continue;
    }
    bool full = false;
    for (uint64_t e = sc.overlap_off[image]; e < sc.overlap_off[image + 1]; ++e) {
      const uint32_t next = sc.overlap[e];
      const FusionView& nv = sc.views[next];
      if (!nv.used || nv.order_pos < cur_pos) continue;
      const float q0 = fusion_row4(nv.P + 0, xyz[0], xyz[1], xyz[2], 1.0f);
      const float q1 = fusion_row4(nv.P + 4, xyz[0], xyz[1], xyz[2], 1.0f);
      const float q2 = fusion_row4(nv.P + 8, xyz[0], xyz[1], xyz[2], 1.0f);
      const int32_t ncol = fusion_round_index((double)(q0 / q2), nv.w);  // std::round(float): the same value as the double round
      const int32_t nrow = fusion_round_index((double)(q1 / q2), nv.h);
      if (ncol < 0 || nrow < 0) continue;
      const uint32_t child = nv.pix0 + (uint32_t)nrow * (uint32_t)nv.w + (uint32_t)ncol;
      if (SPECULATE && (sc.mask[child] || child == g0)) continue;
      if (window) {
        const float r0 = fusion_row4(nv.P + 0, ref[0], ref[1], ref[2], 1.0f);
        const float r1 = fusion_row4(nv.P + 4, ref[0], ref[1], ref[2], 1.0f);
        const float r2 = fusion_row4(nv.P + 8, ref[0], ref[1], ref[2], 1.0f);
        const int child_bit = fusion_window_bit(r0 / r2, r1 / r2, ncol, nrow);
        if (child_bit < 0 || ((st.seen[next * st.stride] >> child_bit) & 1u)) continue;
      }
      if (sp >= st.stack_cap) {
        full = true;
        break;
      }
      st.stack_pix[sp * st.stride] = child;
      st.stack_depth[sp * st.stride] = next_td;
      ++sp;
    }
    if (full) {
      fl |= DSM_FUSION_OVERFLOW | DSM_FUSION_LIMIT;
      break;
    }
  }
  *flags = fl;
  return n;
}

// internal::Median (:40-53) of a[0 .. n) (element k at a[k * stride]): sorts in place (shell sort; the median is a value, any
// selection computes it), then the order statistic at n / 2, for an even n averaged with the largest of the lower half
DSM_FUSION_HD float fusion_median(float* a, uint64_t stride, uint32_t n) {
  uint32_t gap = 1;
  while (gap < n / 3) gap = 3 * gap + 1;
  for (; gap > 0; gap /= 3)
    for (uint32_t i = gap; i < n; ++i) {
      const float x = a[i * stride];
      uint32_t j = i;
      for (; j >= gap && a[(j - gap) * stride] > x; j -= gap) a[j * stride] = a[(j - gap) * stride];
      a[j * stride] = x;
    }
  const uint32_t mid = n / 2;
  if (n % 2 == 0) return (a[mid * stride] + a[(mid - 1) * stride]) / 2.0f;
  return a[mid * stride];
}

// TruncateCast<float, uint8_t>(std::round(x)) (:462-467)
DSM_FUSION_HD uint8_t fusion_colour_cast(float median) {
  const float r = roundf(median);
  return (uint8_t)(r < 0.0f ? 0.0f : (r > 255.0f ? 255.0f : r));
}

// The tail of Fuse() (:441-472) over the accepted pixels list[0 .. n): true and *out, vis (one bit per image, vis_words words,
// element w at vis[w * vis_stride]) when the cluster yields a point.  The nine values of a pixel are recomputed from the maps;
// the store's stack (no longer needed) is the scratch of the medians.
DSM_FUSION_HD bool fusion_finish(const FusionScene& sc, const FusionStore& st, uint32_t n, FusionPoint* out, uint32_t* vis, uint64_t vis_stride,
                                 uint32_t vis_words) {
  if (n < (uint32_t)sc.min_num_pixels) return false;
  float* scratch = reinterpret_cast<float*>(st.stack_pix);
  float med[9];
  for (int pass = 0; pass < 9; ++pass) {
    const int ch = pass < 3 ? 3 + pass : (pass < 6 ? pass - 3 : pass);  // the normal first (:446-448), then x, y, z, then the colour
    for (uint32_t k = 0; k < n; ++k) {
      const uint32_t g = st.list[k * st.stride];
      const FusionView& v = sc.views[fusion_image_of(sc, g)];
      const uint32_t local = g - v.pix0;
      const int32_t row = (int32_t)(local / (uint32_t)v.w), col = (int32_t)(local % (uint32_t)v.w);
      float val;
      if (ch < 6) {
        float xyz[3], normal[3];
        fusion_xyz_normal(sc, v, g, row, col, sc.depth[g], xyz, normal);
        val = ch < 3 ? xyz[ch] : normal[ch - 3];
      } else {
        uint8_t rgb[3];
        fusion_colour(sc, v, row, col, rgb);
        val = (float)rgb[ch - 6];
      }
      scratch[k * st.stride] = val;
    }
    med[ch] = fusion_median(scratch, st.stride, n);
    if (pass == 2) {
      const float norm = sqrtf((med[3] * med[3] + med[4] * med[4]) + med[5] * med[5]);
      if (norm < 1.1920928955078125e-7f) return false;  // std::numeric_limits<float>::epsilon() (:450)
    }
  }
  const float norm = sqrtf((med[3] * med[3] + med[4] * med[4]) + med[5] * med[5]);
  out->x = med[0];
  out->y = med[1];
  out->z = med[2];
  out->nx = med[3] / norm;
  out->ny = med[4] / norm;
  out->nz = med[5] / norm;
  out->r = fusion_colour_cast(med[6]);
  out->g = fusion_colour_cast(med[7]);
  out->b = fusion_colour_cast(med[8]);
  out->pad = 0;
  for (uint32_t w = 0; w < vis_words; ++w) vis[w * vis_stride] = 0;
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t image = fusion_image_of(sc, st.list[k * st.stride]);
    vis[(image / 32) * vis_stride] |= 1u << (image % 32);
  }
  return true;
}

// The raster loop of Run() (:261-271) over one image in the reference's way: seed after seed, marks made at once.  The store
// has room for max_num_pixels pixels and every push.  points / vis ([point][vis_words]) are appended at *n_points.
DSM_FUSION_HD void fusion_serial_image(const FusionScene& sc, uint32_t image, const FusionStore& st, FusionPoint* points, uint32_t* vis, uint32_t vis_words,
                                       uint64_t* n_points, uint64_t* n_traversals) {
  const FusionView& v = sc.views[image];
  const uint32_t n_pix = (uint32_t)v.w * (uint32_t)v.h;
  for (uint32_t s = 0; s < n_pix; ++s) {
    const uint32_t g = v.pix0 + s;
    if (sc.mask[g]) continue;
    uint32_t flags;
    const uint32_t n = fusion_traverse<false>(sc, v.order_pos, g, st, &flags);
    ++*n_traversals;
    if (fusion_finish(sc, st, n, points + *n_points, vis + *n_points * vis_words, 1, vis_words)) ++*n_points;
  }
}

// ---- host only: the checks of dsm_fuse_stereo and the scene as flat arrays (what the device gets uploaded, what the host
// build runs on) ----
#include <string.h>

#include <vector>

#include "../../include/dagsfm_mi355x.h"

static inline void fusion_default_options(dsm_stereo_fusion_options* o) {
  o->min_num_pixels = 5;
  o->max_num_pixels = 10000;
  o->max_traversal_depth = 100;
  o->lane_capacity = 0;
  o->max_reproj_error = 2.0f;
  o->max_depth_error = 0.01f;
  o->max_normal_error = 10.0f;
}

struct FusionHostScene {
  std::vector<FusionView> views;
  std::vector<uint32_t> pix0, overlap, order;  // order: the images in the FindNextImage order
  std::vector<uint64_t> overlap_off;
  std::vector<float> depth, normal;
  std::vector<uint8_t> rgb;
  uint64_t total_pixels = 0;
  uint32_t max_list = 0, max_image_pixels = 0;
  FusionScene scene;  // the pointers are the caller's to fill
};

// nullptr, or what is wrong with the call (DSM_ERR_INVALID_ARGUMENT; *out_of_range: DSM_ERR_OUT_OF_RANGE)
static inline const char* fusion_prepare(const dsm_stereo_fusion_options& o, uint32_t n_images, const dsm_fusion_image* images, const uint64_t* overlap_offsets,
                                         const uint32_t* overlap_images, FusionHostScene* hs, bool* out_of_range) {
  *out_of_range = false;
  if (!(o.min_num_pixels >= 1) || !(o.min_num_pixels <= o.max_num_pixels)) return "min_num_pixels outside 1 .. max_num_pixels";
  if (!(o.max_traversal_depth > 0)) return "max_traversal_depth <= 0";
  if (!(o.lane_capacity >= 0)) return "lane_capacity < 0";
  if (!(o.max_reproj_error >= 0) || !(o.max_depth_error >= 0) || !(o.max_normal_error >= 0)) return "an error bound below 0 or NaN";
  if (n_images && (!images || !overlap_offsets)) return "NULL images or overlap_offsets";
  if (n_images && overlap_offsets[0] != 0) return "overlap_offsets[0] != 0";
  for (uint32_t i = 0; i < n_images; ++i) {
    if (overlap_offsets[i + 1] < overlap_offsets[i]) return "overlap_offsets decrease";
    if (overlap_offsets[i + 1] > overlap_offsets[i] && !overlap_images) return "NULL overlap_images";
    for (uint64_t e = overlap_offsets[i]; e < overlap_offsets[i + 1]; ++e)
      if (overlap_images[e] >= n_images || overlap_images[e] == i) return "an overlap index out of range or equal to its own image";
    const dsm_fusion_image& im = images[i];
    if (!im.used) continue;
    if (!im.width || !im.height || !im.bitmap_width || !im.bitmap_height) return "a used image without pixels";
    if (im.width > 32768 || im.height > 32768 || im.bitmap_width > 32768 || im.bitmap_height > 32768) return "an image side above 32768";
    if (im.row_stride < 3ull * im.bitmap_width) return "a row stride below 3 x bitmap_width";
    if (!im.depth_map || !im.normal_map || !im.rgb) return "NULL depth_map, normal_map or rgb of a used image";
  }
  hs->views.assign(n_images, FusionView());
  hs->pix0.assign(n_images + 1, 0);
  hs->overlap_off.assign(overlap_offsets, overlap_offsets + (n_images ? n_images + 1 : 0));
  if (!n_images) hs->overlap_off.assign(1, 0);
  hs->overlap.assign(overlap_images, overlap_images + (n_images ? overlap_offsets[n_images] : 0));
  uint64_t total = 0, rgb_bytes = 0;
  for (uint32_t i = 0; i < n_images; ++i) {
    const dsm_fusion_image& im = images[i];
    FusionView& v = hs->views[i];
    memset(&v, 0, sizeof(v));
    hs->pix0[i] = (uint32_t)total;
    v.pix0 = (uint32_t)total;
    v.order_pos = 0xffffffffu;
    if (!im.used) continue;
    v.used = 1;
    v.w = (int32_t)im.width;
    v.h = (int32_t)im.height;
    v.bw = (int32_t)im.bitmap_width;
    v.bh = (int32_t)im.bitmap_height;
    memcpy(v.P, im.P, sizeof(v.P));
    memcpy(v.inv_P, im.inv_P, sizeof(v.inv_P));
    memcpy(v.inv_R, im.inv_R, sizeof(v.inv_R));
    memcpy(v.scale, im.bitmap_scale, sizeof(v.scale));
    v.rgb0 = rgb_bytes;
    v.rgb_stride = 3ull * im.bitmap_width;
    rgb_bytes += v.rgb_stride * im.bitmap_height;
    total += (uint64_t)im.width * im.height;
    if (total >= (1ull << 31)) {
      *out_of_range = true;
      return "2^31 pixels or more";
    }
    if ((uint64_t)im.width * im.height > hs->max_image_pixels) hs->max_image_pixels = im.width * im.height;
    if (overlap_offsets[i + 1] - overlap_offsets[i] > hs->max_list) hs->max_list = (uint32_t)(overlap_offsets[i + 1] - overlap_offsets[i]);
  }
  hs->pix0[n_images] = (uint32_t)total;
  hs->total_pixels = total;
  hs->depth.resize(total);
  hs->normal.resize(3 * total);
  hs->rgb.resize(rgb_bytes);
  for (uint32_t i = 0; i < n_images; ++i) {
    const dsm_fusion_image& im = images[i];
    const FusionView& v = hs->views[i];
    if (!v.used) continue;
    const uint64_t n = (uint64_t)im.width * im.height;
    for (uint64_t k = 0; k < n; ++k) {
      const float d = im.depth_map[k], n0 = im.normal_map[k], n1 = im.normal_map[n + k], n2 = im.normal_map[2 * n + k];
      if (!isfinite(d) || !isfinite(n0) || !isfinite(n1) || !isfinite(n2)) return "a depth or normal that is not finite";
      hs->depth[v.pix0 + k] = d;
      float* q = &hs->normal[3 * (v.pix0 + k)];
      q[0] = n0;
      q[1] = n1;
      q[2] = n2;
    }
    for (uint32_t y = 0; y < im.bitmap_height; ++y) memcpy(&hs->rgb[v.rgb0 + y * v.rgb_stride], im.rgb + y * im.row_stride, v.rgb_stride);
  }
  // the order of Run()'s loop (:239-241, FindNextImage :58-79): it starts at image 0 whether or not that image is used
  hs->order.clear();
  if (n_images) {
    std::vector<char> fused(n_images, 0);
    for (int64_t cur = 0; cur >= 0;) {
      hs->views[cur].order_pos = (uint32_t)hs->order.size();
      hs->order.push_back((uint32_t)cur);
      fused[cur] = 1;
      int64_t next = -1;
      for (uint64_t e = overlap_offsets[cur]; e < overlap_offsets[cur + 1] && next < 0; ++e)
        if (images[overlap_images[e]].used && !fused[overlap_images[e]]) next = overlap_images[e];
      for (uint32_t i = 0; i < n_images && next < 0; ++i)
        if (images[i].used && !fused[i]) next = i;
      cur = next;
    }
  }
  FusionScene& sc = hs->scene;
  memset(&sc, 0, sizeof(sc));
  sc.n_images = n_images;
  sc.min_num_pixels = o.min_num_pixels;
  sc.max_num_pixels = o.max_num_pixels;
  sc.max_traversal_depth = o.max_traversal_depth;
  sc.max_depth_error = o.max_depth_error;
  sc.max_squared_reproj_error = (float)(o.max_reproj_error * o.max_reproj_error);               // fusion.cc:120-121
  sc.min_cos_normal_error = (float)cos(o.max_normal_error * 0.0174532925199432954743716805978692718781530857086181640625);  // :122, DegToRad
  return nullptr;
}
#endif  // DAGSFM_AMD_CSRC_STEREO_FUSION_H_
