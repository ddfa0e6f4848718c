// undistortion.hip -- image and reconstruction undistortion: UndistortCamera, the point loop of
// UndistortReconstruction (src/base/undistortion.cc:659-842, 869-879) and the warps of src/base/warp.cc:51-172 up to, but not
// including, their final Bitmap::Rescale (FreeImage_Rescale stays with the host application; dsm_warp_images reports that it
// is owed).
//
//   k_ud_border   a thread per border pixel of every camera of the batch, one launch: image_to_world of the distorted camera,
//                 then the pinhole projection f * u + c of the undistorted one (undistortion.cc:738-777)
//   k_ud_minmax   a block per camera: the eight minima / maxima of its four borders with block_reduce.h's std::min / std::max
//                 trees.  A partial starts at DBL_MAX / lowest and a NaN on the right of std::min / std::max is never taken, so no
//                 partial is a NaN and the result does not depend on the order.  The scalar tail (:779-839) runs on the host.
//   k_ud_points   a thread per 2D point: undistorted.WorldToImage(distorted.ImageToWorld(xy)) in place
//   k_ud_warp     a lane per four consecutive target pixels of one row (x fastest across the lanes): the source coordinate of
//                 each once, then Bitmap::InterpolateBilinear + BitmapColor<float>::Cast<uint8_t> of every image and channel of
//                 the chunk with it; full groups store whole dwords.  No LDS, no atomics; every lane reads the same two
//                 cameras, so the switch on the model is wave-uniform.  A non-pinhole target runs IterativeUndistortion per
//                 lane and diverges; the undistorter's own target is always PINHOLE.
//
// The forward model is ba_project.h's, instantiated with UdX: a double whose atan / tan are exact_trig.h's correctly rounded
// ones (what the CPU oracle computes), where ba_world_to_image<double> calls the device library's.  Every operation is a plain
// double operation (-ffp-contract=off), so all eleven models give the oracle's bytes.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ba_project.h"
#include "block_reduce.h"
#include "ctx.h"

namespace {

constexpr int UD_BLOCK = 256;
constexpr int UD_PX = 4;                   // consecutive target pixels of one lane
constexpr int UD_TILE_W = 64 * UD_PX;      // target pixels of one block row: a wave covers 256 pixels of one row
constexpr int UD_TILE_H = UD_BLOCK / 64;   // rows of one block: a wave each
constexpr uint64_t UD_MAX_SIDE = 1u << 30; // Bitmap's sizes are int
constexpr size_t UD_SRC_HEAD = 1024;       // bytes at the head of the source buffer: the two cameras of the warp kernel
constexpr uint64_t UD_DEFAULT_CHUNK_BYTES = 4ull << 30;  // source + target images on the device at a time without a budget

// the scalar of the exact forward model
struct UdX {
  double v;
};
__device__ inline UdX operator+(const UdX& a, const UdX& b) { return UdX{a.v + b.v}; }
__device__ inline UdX operator-(const UdX& a, const UdX& b) { return UdX{a.v - b.v}; }
__device__ inline UdX operator*(const UdX& a, const UdX& b) { return UdX{a.v * b.v}; }
__device__ inline UdX operator/(const UdX& a, const UdX& b) { return UdX{a.v / b.v}; }
__device__ inline UdX operator+(const UdX& a, double b) { return UdX{a.v + b}; }
__device__ inline UdX operator+(double a, const UdX& b) { return UdX{a + b.v}; }
__device__ inline UdX operator-(const UdX& a, double b) { return UdX{a.v - b}; }
__device__ inline UdX operator-(double a, const UdX& b) { return UdX{a - b.v}; }
__device__ inline UdX operator*(const UdX& a, double b) { return UdX{a.v * b}; }
__device__ inline UdX operator*(double a, const UdX& b) { return UdX{a * b.v}; }
__device__ inline UdX operator/(const UdX& a, double b) { return UdX{a.v / b}; }
__device__ inline UdX operator/(double a, const UdX& b) { return UdX{a / b.v}; }
__device__ inline UdX sqrt(const UdX& a) { return UdX{::sqrt(a.v)}; }
__device__ inline UdX atan(const UdX& a) { return UdX{dsm_atan(a.v)}; }
__device__ inline UdX tan(const UdX& a) { return UdX{dsm_tan(a.v)}; }
__device__ inline double ba_val(const UdX& x) { return x.v; }

// Camera::WorldToImage, bit for bit the oracle's: the one instantiation of the forward model this file carries
__device__ __noinline__ void ud_world_to_image(const dsm_camera& cam, double u, double v, double* x, double* y) {
  UdX p[12];
  for (int i = 0; i < 12; ++i) p[i].v = cam.params[i];
  UdX ox, oy;
  ba_world_to_image<UdX>(cam.model_id, p, UdX{u}, UdX{v}, &ox, &oy);
  *x = ox.v;
  *y = oy.v;
}
__device__ __noinline__ void ud_image_to_world(const dsm_camera& cam, double x, double y, double* u, double* v) {
  image_to_world(cam, x, y, u, v);
}

// ---- UndistortCamera: the border scan ----
struct UdBorderCam {
  dsm_camera cam;          // the distorted camera
  double fx, fy, cx, cy;   // the undistorted PINHOLE camera before the scaling
  uint32_t y0, ny, x0, nx; // the ROI: rows y0 .. y0 + ny of the left / right borders, columns x0 .. x0 + nx of the top / bottom ones
  uint32_t off;            // first item: [left ny][right ny][top nx][bottom nx]; ny = nx = 0 for a camera without a scan
  uint32_t pad;
};

__global__ void __launch_bounds__(UD_BLOCK) k_ud_border(uint32_t n_cams, uint32_t n_items, const UdBorderCam* __restrict__ cams,
                                                         double* __restrict__ vals) {
  const uint32_t i = blockIdx.x * UD_BLOCK + threadIdx.x;
  if (i >= n_items) return;
  uint32_t lo = 0, hi = n_cams - 1;  // the last camera with off <= i that has items: the smallest c whose end exceeds i
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (cams[mid].off + 2 * (cams[mid].ny + cams[mid].nx) <= i)
      lo = mid + 1;
    else
      hi = mid;
  }
  const UdBorderCam& c = cams[lo];
  uint32_t j = i - c.off;
  double px, py;
  bool horizontal;  // the x coordinate is what the border contributes
  if (j < 2 * c.ny) {
    const bool right = j >= c.ny;
    if (right) j -= c.ny;
    px = right ? (double)c.cam.width - 0.5 : 0.5;
    py = (double)(c.y0 + j) + 0.5;
    horizontal = true;
  } else {
    j -= 2 * c.ny;
    const bool bottom = j >= c.nx;
    if (bottom) j -= c.nx;
    px = (double)(c.x0 + j) + 0.5;
    py = bottom ? (double)c.cam.height - 0.5 : 0.5;
    horizontal = false;
  }
  double u, v;
  ud_image_to_world(c.cam, px, py, &u, &v);
  vals[i] = horizontal ? c.fx * u + c.cx : c.fy * v + c.cy;  // PinholeCameraModel::WorldToImage
}

// out[8 * camera ..]: left min, left max, right min, right max, top min, top max, bottom min, bottom max
__global__ void __launch_bounds__(UD_BLOCK) k_ud_minmax(const UdBorderCam* __restrict__ cams, const double* __restrict__ vals,
                                                         double* __restrict__ out) {
  __shared__ double sh[4 * UD_BLOCK];
  const UdBorderCam& c = cams[blockIdx.x];
  double mn[4], mx[4];
  uint32_t begin = c.off;
  for (int s = 0; s < 4; ++s) {
    const uint32_t len = s < 2 ? c.ny : c.nx;
    double a = DBL_MAX, b = -DBL_MAX;
    for (uint32_t i = threadIdx.x; i < len; i += UD_BLOCK) {
      const double x = vals[begin + i];
      a = std_min(a, x);
      b = std_max(b, x);
    }
    mn[s] = a;
    mx[s] = b;
    begin += len;
  }
  block_std_min<UD_BLOCK, 4>(mn, sh);
  block_std_max<UD_BLOCK, 4>(mx, sh);
  if (threadIdx.x == 0)
    for (int s = 0; s < 4; ++s) {
      out[8 * (size_t)blockIdx.x + 2 * s] = mn[s];
      out[8 * (size_t)blockIdx.x + 2 * s + 1] = mx[s];
    }
}

// ---- UndistortReconstruction: the 2D points ----
__global__ void __launch_bounds__(UD_BLOCK) k_ud_points(uint64_t n, const dsm_camera* __restrict__ cams, const dsm_camera* __restrict__ und,
                                                         const uint32_t* __restrict__ cam_idx, double* __restrict__ xy) {
  const uint64_t i = (uint64_t)blockIdx.x * UD_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = cam_idx[i];
  double u, v, x, y;
  ud_image_to_world(cams[c], xy[2 * i], xy[2 * i + 1], &u, &v);
  ud_world_to_image(und[c], u, v, &x, &y);
  xy[2 * i] = x;
  xy[2 * i + 1] = y;
}

// ---- the warps ----
enum { UD_MODE_CAMERAS = 0, UD_MODE_H_CAMERAS = 1, UD_MODE_H = 2 };

struct UdWarp {
  // cams[0]: the source (WorldToImage); cams[1]: the target ImageToWorld runs on -- the scaled one without H, the unscaled one
  // with H (warp.cc:154).  In device memory, at the head of the source buffer: a camera in the kernel arguments would be copied
  // to every lane's scratch to be passed to the model functions by reference.
  const dsm_camera* cams;
  double H[9];         // row-major
  int32_t mode;
  uint32_t sw, sh, tw, th;  // source and target sizes in pixels
  uint32_t channels, n_images, tiles_x;
  const uint8_t* src;  // [n_images][sh][src_row], rows top-down
  uint8_t* dst;        // [n_images][th][dst_row]; dst_row is a multiple of 4
  uint64_t src_row, src_img, dst_row, dst_img;
  double* map;         // NULL, or [th][tw][2]: the source point before the - 0.5
};

// the four taps of Bitmap::InterpolateBilinear(x - 0.5, y - 0.5): bitmap.cc:225-243.  A coordinate that is NaN or whose floor
// is outside int is refused (the reference's static_cast<int> is undefined there and lands on INT_MIN on x86: refused too).
struct UdTap {
  double dx, dx_1, dy, dy_1;
  uint32_t x0, row0, row1;  // row0 / row1: the top-down rows of FreeImage's scanlines y0 and y0 + 1
  bool valid;
};
__device__ inline UdTap ud_tap(double sx, double sy, uint32_t w, uint32_t h) {
  UdTap t;
  t.dx = t.dx_1 = t.dy = t.dy_1 = 0.0;
  t.x0 = t.row0 = t.row1 = 0;
  t.valid = false;
  const double x = sx - 0.5, y = sy - 0.5;
  const double inv_y = (double)((int)h - 1) - y;
  const double fx = floor(x), fy = floor(inv_y);
  if (!(fx >= -2147483648.0 && fx <= 2147483647.0 && fy >= -2147483648.0 && fy <= 2147483647.0)) return t;
  const long long x0 = (long long)fx, y0 = (long long)fy;
  if (x0 < 0 || x0 + 1 >= (long long)w || y0 < 0 || y0 + 1 >= (long long)h) return t;
  t.dx = x - (double)x0;
  t.dy = inv_y - (double)y0;
  t.dx_1 = 1 - t.dx;
  t.dy_1 = 1 - t.dy;
  t.x0 = (uint32_t)x0;
  t.row0 = h - 1 - (uint32_t)y0;
  t.row1 = t.row0 - 1;
  t.valid = true;
  return t;
}
// one channel: the interpolation in double, the value through float, std::round of the float clamped to [0, 255] (bitmap.h:217-221)
__device__ inline uint8_t ud_sample(const UdTap& t, uint32_t a0, uint32_t a1, uint32_t b0, uint32_t b1) {
  const double v0 = t.dx_1 * (double)a0 + t.dx * (double)a1;
  const double v1 = t.dx_1 * (double)b0 + t.dx * (double)b1;
  const float value = (float)(t.dy_1 * v0 + t.dy * v1);
  const float r = roundf(value);
  const float lo = 0.0f < r ? r : 0.0f;        // std::max(0, round)
  const float c = lo < 255.0f ? lo : 255.0f;   // std::min(255, .)
  return (uint8_t)c;
}

__device__ inline void ud_source_point(const UdWarp& p, uint32_t x, uint32_t y, double* sx, double* sy) {
  const double ix = (double)x + 0.5, iy = (double)y + 0.5;
  if (p.mode == UD_MODE_CAMERAS) {
    double u, v;
    ud_image_to_world(p.cams[1], ix, iy, &u, &v);
    ud_world_to_image(p.cams[0], u, v, sx, sy);
    return;
  }
  // H * (ix, iy, 1), each row summed in order, then hnormalized
  const double* H = p.H;
  const double w0 = (H[0] * ix + H[1] * iy) + H[2];
  const double w1 = (H[3] * ix + H[4] * iy) + H[5];
  const double w2 = (H[6] * ix + H[7] * iy) + H[8];
  const double hx = w0 / w2, hy = w1 / w2;
  if (p.mode == UD_MODE_H) {
    *sx = hx;
    *sy = hy;
    return;
  }
  double u, v;
  ud_image_to_world(p.cams[1], hx, hy, &u, &v);
  ud_world_to_image(p.cams[0], u, v, sx, sy);
}

template <int C>
__device__ inline void ud_warp_body(const UdWarp& p, uint32_t x, uint32_t y) {
  UdTap tap[UD_PX];
  const uint32_t npx = min((uint32_t)UD_PX, p.tw - x);
#pragma unroll
  for (int k = 0; k < UD_PX; ++k) {
    tap[k] = ud_tap(NAN, NAN, p.sw, p.sh);
    if ((uint32_t)k < npx) {
      double sx, sy;
      ud_source_point(p, x + k, y, &sx, &sy);
      if (p.map) {
        double* m = p.map + 2 * ((size_t)y * p.tw + x + k);
        m[0] = sx;
        m[1] = sy;
      }
      tap[k] = ud_tap(sx, sy, p.sw, p.sh);
    }
  }
  for (uint32_t img = 0; img < p.n_images; ++img) {
    const uint8_t* s = p.src + (size_t)img * p.src_img;
    uint8_t* d = p.dst + (size_t)img * p.dst_img + (size_t)y * p.dst_row + (size_t)x * C;
    uint8_t out[UD_PX * C];
#pragma unroll
    for (int k = 0; k < UD_PX; ++k) {
      const UdTap& t = tap[k];
      // The pixels x0 and x0 + 1 of a scanline are 2 * C contiguous bytes: one unaligned load of 2 (grey) or 8 (RGB, of which 6
      // are used) bytes a scanline in place of 2 * C byte loads.  The two bytes past an RGB pair are the next pixel's, the next
      // row's, the next image's or the slack behind the last image (the buffer ends 16 bytes after it).
      uint64_t w0 = 0, w1 = 0;
      if (t.valid) {
        __builtin_memcpy(&w0, s + (size_t)t.row0 * p.src_row + (size_t)t.x0 * C, C == 1 ? 2 : 8);
        __builtin_memcpy(&w1, s + (size_t)t.row1 * p.src_row + (size_t)t.x0 * C, C == 1 ? 2 : 8);
      }
#pragma unroll
      for (int ch = 0; ch < C; ++ch)
        out[k * C + ch] = t.valid ? ud_sample(t, (uint32_t)(w0 >> (8 * ch)) & 255u, (uint32_t)(w0 >> (8 * (C + ch))) & 255u,
                                              (uint32_t)(w1 >> (8 * ch)) & 255u, (uint32_t)(w1 >> (8 * (C + ch))) & 255u)
                                  : (uint8_t)0;
    }
    if (npx == UD_PX) {  // dst_row and x * C are multiples of 4: whole dwords
#pragma unroll
      for (int j = 0; j < C; ++j)
        reinterpret_cast<uint32_t*>(d)[j] = (uint32_t)out[4 * j] | ((uint32_t)out[4 * j + 1] << 8) | ((uint32_t)out[4 * j + 2] << 16) |
                                            ((uint32_t)out[4 * j + 3] << 24);
    } else {
#pragma unroll
      for (int k = 0; k < UD_PX * C; ++k)
        if ((uint32_t)k < npx * C) d[k] = out[k];
    }
  }
}

__global__ void __launch_bounds__(UD_BLOCK) k_ud_warp(UdWarp p) {
  const uint32_t tile_x = blockIdx.x % p.tiles_x, tile_y = blockIdx.x / p.tiles_x;
  const uint32_t x = tile_x * UD_TILE_W + (threadIdx.x & 63) * UD_PX;
  const uint32_t y = tile_y * UD_TILE_H + (threadIdx.x >> 6);
  if (x >= p.tw || y >= p.th) return;
  if (p.channels == 1)
    ud_warp_body<1>(p, x, y);
  else
    ud_warp_body<3>(p, x, y);
}

// std::min / std::max / Clip as the reference's scalar tail evaluates them (a NaN takes the branch the comparison leaves)
inline double ref_min(double a, double b) { return (b < a) ? b : a; }
inline double ref_max(double a, double b) { return (a < b) ? b : a; }
inline double ref_clip(double value, double low, double high) { return ref_max(low, ref_min(value, high)); }

inline int focal_count(int model_id) { return cam_two_focal(model_id) ? 2 : 1; }
inline double& principal_x(dsm_camera& c) { return c.params[cam_two_focal(c.model_id) ? 2 : 1]; }
inline double& principal_y(dsm_camera& c) { return c.params[cam_two_focal(c.model_id) ? 3 : 2]; }

// Camera::Rescale(scale), camera.cc:228-247
void camera_rescale(dsm_camera& c, double scale) {
  const double scale_x = std::round(scale * c.width) / static_cast<double>(c.width);
  const double scale_y = std::round(scale * c.height) / static_cast<double>(c.height);
  c.width = static_cast<uint64_t>(std::round(scale * c.width));
  c.height = static_cast<uint64_t>(std::round(scale * c.height));
  principal_x(c) = scale_x * principal_x(c);
  principal_y(c) = scale_y * principal_y(c);
  if (focal_count(c.model_id) == 1) {
    c.params[0] = (scale_x + scale_y) / 2.0 * c.params[0];
  } else {
    c.params[0] = scale_x * c.params[0];
    c.params[1] = scale_y * c.params[1];
  }
}
// Camera::Rescale(width, height), camera.cc:249-267
void camera_rescale(dsm_camera& c, uint64_t width, uint64_t height) {
  const double scale_x = static_cast<double>(width) / static_cast<double>(c.width);
  const double scale_y = static_cast<double>(height) / static_cast<double>(c.height);
  c.width = width;
  c.height = height;
  principal_x(c) = scale_x * principal_x(c);
  principal_y(c) = scale_y * principal_y(c);
  if (focal_count(c.model_id) == 1) {
    c.params[0] = (scale_x + scale_y) / 2.0 * c.params[0];
  } else {
    c.params[0] = scale_x * c.params[0];
    c.params[1] = scale_y * c.params[1];
  }
}

void mark_ready(dsm_ctx* ctx) {
  if (!ctx->undistortion_ready) {
    ctx->undistortion_ready = true;
    for (double& t : ctx->undistortion_ms) t = 0.0;
  }
}

}  // namespace

extern "C" void dsm_default_undistort_options(dsm_undistort_options* o) {  // UndistortCameraOptions, undistortion.h:41-62
  o->blank_pixels = 0.0;
  o->min_scale = 0.2;
  o->max_scale = 2.0;
  o->max_image_size = -1;
  o->reserved = 0;
  o->roi_min_x = 0.0;
  o->roi_min_y = 0.0;
  o->roi_max_x = 1.0;
  o->roi_max_y = 1.0;
}

extern "C" int dsm_undistort_cameras(dsm_ctx* ctx, const dsm_undistort_options* options, uint32_t n, const dsm_camera* cameras,
                                     dsm_camera* out_cameras) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_undistort_cameras", msg); };
  if (n && (!cameras || !out_cameras)) return fail("NULL argument");
  dsm_undistort_options o;
  if (options)
    o = *options;
  else
    dsm_default_undistort_options(&o);
  // the CHECKs of undistortion.cc:661-671 (written so that a NaN fails them, as it fails the reference's)
  if (!(o.blank_pixels >= 0)) return fail("blank_pixels < 0");
  if (!(o.blank_pixels <= 1)) return fail("blank_pixels > 1");
  if (!(o.min_scale > 0.0)) return fail("min_scale <= 0");
  if (!(o.min_scale <= o.max_scale)) return fail("min_scale > max_scale");
  if (!(o.max_image_size != 0)) return fail("max_image_size == 0");
  if (!(o.roi_min_x >= 0.0)) return fail("roi_min_x < 0");
  if (!(o.roi_min_y >= 0.0)) return fail("roi_min_y < 0");
  if (!(o.roi_max_x <= 1.0)) return fail("roi_max_x > 1");
  if (!(o.roi_max_y <= 1.0)) return fail("roi_max_y > 1");
  if (!(o.roi_min_x < o.roi_max_x)) return fail("roi_min_x >= roi_max_x");
  if (!(o.roi_min_y < o.roi_max_y)) return fail("roi_min_y >= roi_max_y");
  for (uint32_t i = 0; i < n; ++i) {
    if (!cam_model_exists(cameras[i].model_id)) return fail("an unknown camera model");
    if (cameras[i].width == 0 || cameras[i].height == 0 || cameras[i].width > UD_MAX_SIDE || cameras[i].height > UD_MAX_SIDE)
      return fail("a camera without pixels, or with a side above 2^30");
  }
  if (!n) return DSM_OK;

  // :673-726: the PINHOLE camera and the ROI
  const bool roi_enabled = o.roi_min_x > 0.0 || o.roi_min_y > 0.0 || o.roi_max_x < 1.0 || o.roi_max_y < 1.0;
  std::vector<dsm_camera> und(n);
  std::vector<UdBorderCam> bc(n);
  uint64_t n_items = 0;
  for (uint32_t i = 0; i < n; ++i) {
    const dsm_camera& cam = cameras[i];
    dsm_camera& u = und[i];
    memset(&u, 0, sizeof(u));
    u.model_id = 1;
    u.width = cam.width;
    u.height = cam.height;
    const bool two = cam_two_focal(cam.model_id);
    u.params[0] = cam.params[0];
    u.params[1] = two ? cam.params[1] : cam.params[0];
    u.params[2] = cam.params[two ? 2 : 1];
    u.params[3] = cam.params[two ? 3 : 2];
    uint64_t roi_min_x = 0, roi_min_y = 0, roi_max_x = cam.width, roi_max_y = cam.height;
    if (roi_enabled) {
      roi_min_x = static_cast<uint64_t>(std::round(o.roi_min_x * static_cast<double>(cam.width)));
      roi_min_y = static_cast<uint64_t>(std::round(o.roi_min_y * static_cast<double>(cam.height)));
      roi_max_x = static_cast<uint64_t>(std::round(o.roi_max_x * static_cast<double>(cam.width)));
      roi_max_y = static_cast<uint64_t>(std::round(o.roi_max_y * static_cast<double>(cam.height)));
      roi_min_x = std::min<uint64_t>(roi_min_x, cam.width - 1);
      roi_min_y = std::min<uint64_t>(roi_min_y, cam.height - 1);
      roi_max_x = std::max<uint64_t>(roi_max_x, roi_min_x + 1);
      roi_max_y = std::max<uint64_t>(roi_max_y, roi_min_y + 1);
      u.width = roi_max_x - roi_min_x;
      u.height = roi_max_y - roi_min_y;
      u.params[2] = u.params[2] - static_cast<double>(roi_min_x);
      u.params[3] = u.params[3] - static_cast<double>(roi_min_y);
    }
    UdBorderCam& b = bc[i];
    memset(&b, 0, sizeof(b));
    b.cam = cam;
    b.fx = u.params[0];
    b.fy = u.params[1];
    b.cx = u.params[2];
    b.cy = u.params[3];
    b.off = (uint32_t)n_items;
    if (roi_enabled || (cam.model_id != 0 && cam.model_id != 1)) {
      b.y0 = (uint32_t)roi_min_y;
      b.ny = (uint32_t)(roi_max_y - roi_min_y);
      b.x0 = (uint32_t)roi_min_x;
      b.nx = (uint32_t)(roi_max_x - roi_min_x);
    }
    n_items += 2 * ((uint64_t)b.ny + b.nx);
    if (n_items >= 0x7fffffffu) return fail("too many border pixels in one batch");
  }

  std::vector<double> mm((size_t)8 * n, 0.0);
  double scan_ms = 0;
  if (n_items) {
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
    hipStream_t st = ctx->stream;
    DevEvents<2> ev;
    HIPCHK(ctx, ev.create());
    // the cameras, the per-pixel values and the minima / maxima share one scratch buffer
    const size_t cams_bytes = ((size_t)n * sizeof(UdBorderCam) + 255) & ~(size_t)255;
    const size_t vals_bytes = ((size_t)n_items * 8 + 255) & ~(size_t)255;
    HIPCHK(ctx, ctx->d_ud_border.reserve(cams_bytes + vals_bytes + (size_t)n * 64));
    uint8_t* base = ctx->d_ud_border.as<uint8_t>();
    UdBorderCam* d_cams = reinterpret_cast<UdBorderCam*>(base);
    double* d_vals = reinterpret_cast<double*>(base + cams_bytes);
    double* d_mm = reinterpret_cast<double*>(base + cams_bytes + vals_bytes);
    HIPCHK(ctx, hipMemcpyAsync(d_cams, bc.data(), (size_t)n * sizeof(UdBorderCam), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_ud_border, dim3((uint32_t)((n_items + UD_BLOCK - 1) / UD_BLOCK)), dim3(UD_BLOCK), 0, st, n, (uint32_t)n_items, d_cams,
                       d_vals);
    hipLaunchKernelGGL(k_ud_minmax, dim3(n), dim3(UD_BLOCK), 0, st, d_cams, d_vals, d_mm);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(mm.data(), d_mm, (size_t)n * 64, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, ev.ms(0, 1, &scan_ms));
  }

  // :779-839, the scalar tail in the reference's order
  for (uint32_t i = 0; i < n; ++i) {
    dsm_camera& u = und[i];
    if (bc[i].ny) {
      const double* m = &mm[(size_t)8 * i];
      const double left_min_x = m[0], left_max_x = m[1], right_min_x = m[2], right_max_x = m[3];
      const double top_min_y = m[4], top_max_y = m[5], bottom_min_y = m[6], bottom_max_y = m[7];
      const double cx = u.params[2];
      const double cy = u.params[3];
      const double min_scale_x = ref_min(cx / (cx - left_min_x), (u.width - 0.5 - cx) / (right_max_x - cx));
      const double min_scale_y = ref_min(cy / (cy - top_min_y), (u.height - 0.5 - cy) / (bottom_max_y - cy));
      const double max_scale_x = ref_max(cx / (cx - left_max_x), (u.width - 0.5 - cx) / (right_min_x - cx));
      const double max_scale_y = ref_max(cy / (cy - top_max_y), (u.height - 0.5 - cy) / (bottom_min_y - cy));
      double scale_x = 1.0 / (min_scale_x * o.blank_pixels + max_scale_x * (1.0 - o.blank_pixels));
      double scale_y = 1.0 / (min_scale_y * o.blank_pixels + max_scale_y * (1.0 - o.blank_pixels));
      scale_x = ref_clip(scale_x, o.min_scale, o.max_scale);
      scale_y = ref_clip(scale_y, o.min_scale, o.max_scale);
      const uint64_t orig_width = u.width;
      const uint64_t orig_height = u.height;
      u.width = static_cast<uint64_t>(ref_max(1.0, scale_x * u.width));
      u.height = static_cast<uint64_t>(ref_max(1.0, scale_y * u.height));
      u.params[2] = u.params[2] * static_cast<double>(u.width) / static_cast<double>(orig_width);
      u.params[3] = u.params[3] * static_cast<double>(u.height) / static_cast<double>(orig_height);
    }
    if (o.max_image_size > 0) {
      const double max_image_scale_x = o.max_image_size / static_cast<double>(u.width);
      const double max_image_scale_y = o.max_image_size / static_cast<double>(u.height);
      const double max_image_scale = ref_min(max_image_scale_x, max_image_scale_y);
      if (max_image_scale < 1.0) camera_rescale(u, max_image_scale);
    }
  }
  memcpy(out_cameras, und.data(), (size_t)n * sizeof(dsm_camera));
  mark_ready(ctx);
  ctx->undistortion_ms[0] = scan_ms;
  return DSM_OK;
}

extern "C" int dsm_undistort_points2D(dsm_ctx* ctx, uint32_t n_cameras, const dsm_camera* cameras, const dsm_camera* undistorted_cameras,
                                      uint64_t n_points, const uint32_t* camera_index, double* xy) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_undistort_points2D", msg); };
  if ((n_cameras && (!cameras || !undistorted_cameras)) || (n_points && (!camera_index || !xy))) return fail("NULL argument");
  if (n_points >= ((uint64_t)1 << 31) * UD_BLOCK) return fail("too many points");
  for (uint32_t i = 0; i < n_cameras; ++i)
    if (!cam_model_exists(cameras[i].model_id) || !cam_model_exists(undistorted_cameras[i].model_id)) return fail("an unknown camera model");
  for (uint64_t i = 0; i < n_points; ++i)
    if (camera_index[i] >= n_cameras) return fail("a point on a camera index out of range");
  double ms = 0;
  if (n_points) {
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
    hipStream_t st = ctx->stream;
    DevEvents<2> ev;
    HIPCHK(ctx, ev.create());
    const size_t cams_bytes = ((size_t)n_cameras * sizeof(dsm_camera) + 255) & ~(size_t)255;
    const size_t idx_bytes = ((size_t)n_points * 4 + 255) & ~(size_t)255;
    HIPCHK(ctx, ctx->d_ud_points.reserve(2 * cams_bytes + idx_bytes + (size_t)n_points * 16));
    uint8_t* base = ctx->d_ud_points.as<uint8_t>();
    dsm_camera* d_cams = reinterpret_cast<dsm_camera*>(base);
    dsm_camera* d_und = reinterpret_cast<dsm_camera*>(base + cams_bytes);
    uint32_t* d_idx = reinterpret_cast<uint32_t*>(base + 2 * cams_bytes);
    double* d_xy = reinterpret_cast<double*>(base + 2 * cams_bytes + idx_bytes);
    HIPCHK(ctx, hipMemcpyAsync(d_cams, cameras, (size_t)n_cameras * sizeof(dsm_camera), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_und, undistorted_cameras, (size_t)n_cameras * sizeof(dsm_camera), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_idx, camera_index, (size_t)n_points * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(d_xy, xy, (size_t)n_points * 16, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(k_ud_points, dim3((uint32_t)((n_points + UD_BLOCK - 1) / UD_BLOCK)), dim3(UD_BLOCK), 0, st, n_points, d_cams, d_und, d_idx,
                       d_xy);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipEventRecord(ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(xy, d_xy, (size_t)n_points * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, ev.ms(0, 1, &ms));
  }
  mark_ready(ctx);
  ctx->undistortion_ms[1] = ms;
  return DSM_OK;
}

extern "C" int dsm_warp_images(dsm_ctx* ctx, const dsm_camera* source_camera, const dsm_camera* target_camera, const double* H,
                               uint32_t n_images, uint32_t channels, const uint8_t* src, uint64_t src_row_stride, uint64_t src_image_stride,
                               uint8_t* dst, uint64_t dst_row_stride, uint64_t dst_image_stride, dsm_camera* out_scaled_target_camera,
                               int32_t* out_needs_rescale, double* out_source_xy) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_warp_images", msg); };
  if (!source_camera) return fail("source_camera is NULL (a size-only camera, model_id DSM_CAMERA_SIZE_ONLY, gives the size of a warp without cameras)");
  if (channels != 1 && channels != 3) return fail("channels must be 1 or 3");
  const bool size_only = source_camera->model_id == DSM_CAMERA_SIZE_ONLY;
  int mode;
  if (size_only) {
    if (!H) return fail("a warp without cameras needs H");
    if (target_camera && target_camera->model_id != DSM_CAMERA_SIZE_ONLY) return fail("a size-only source camera with a real target camera");
    mode = UD_MODE_H;
  } else {
    if (!target_camera) return fail("target_camera is NULL");
    if (!cam_model_exists(source_camera->model_id) || !cam_model_exists(target_camera->model_id)) return fail("an unknown camera model");
    mode = H ? UD_MODE_H_CAMERAS : UD_MODE_CAMERAS;
  }
  for (const dsm_camera* c : {source_camera, target_camera})
    if (c && (c->width == 0 || c->height == 0 || c->width > UD_MAX_SIDE || c->height > UD_MAX_SIDE))
      return fail("a camera without pixels, or with a side above 2^30");
  const uint64_t sw = source_camera->width, sh = source_camera->height;
  // with cameras the warp runs at the source resolution (warp.cc:58-68); without, the target image has its own size (:98-122)
  const uint64_t tw = mode == UD_MODE_H && target_camera ? target_camera->width : sw;
  const uint64_t th = mode == UD_MODE_H && target_camera ? target_camera->height : sh;
  if (n_images && (!src || !dst)) return fail("NULL image pointer");
  if (src_row_stride < sw * channels) return fail("src_row_stride below width * channels");
  if (dst_row_stride < tw * channels) return fail("dst_row_stride below width * channels");
  if (n_images > 1 && (src_image_stride < src_row_stride * sh || dst_image_stride < dst_row_stride * th))
    return fail("an image stride below row stride * height");

  dsm_camera scaled;
  memset(&scaled, 0, sizeof(scaled));
  int32_t needs_rescale = 0;
  if (mode != UD_MODE_H) {
    scaled = *target_camera;
    if (target_camera->width != sw || target_camera->height != sh) {
      camera_rescale(scaled, sw, sh);
      needs_rescale = 1;
    }
  } else if (target_camera) {
    scaled = *target_camera;
  } else {
    scaled = *source_camera;
  }

  UdWarp p;
  memset(&p, 0, sizeof(p));
  p.mode = mode;
  dsm_camera kernel_cams[2];
  memset(kernel_cams, 0, sizeof(kernel_cams));
  if (mode != UD_MODE_H) {
    kernel_cams[0] = *source_camera;
    kernel_cams[1] = mode == UD_MODE_CAMERAS ? scaled : *target_camera;
  }
  if (H) memcpy(p.H, H, sizeof(p.H));
  p.sw = (uint32_t)sw;
  p.sh = (uint32_t)sh;
  p.tw = (uint32_t)tw;
  p.th = (uint32_t)th;
  p.channels = channels;
  p.tiles_x = (uint32_t)((tw + UD_TILE_W - 1) / UD_TILE_W);
  const uint64_t tiles = (uint64_t)p.tiles_x * ((th + UD_TILE_H - 1) / UD_TILE_H);
  if (tiles >= 0x7fffffffu) return fail("an image of too many tiles");
  p.src_row = sw * channels;
  p.src_img = p.src_row * sh;
  p.dst_row = (tw * channels + 3) & ~(uint64_t)3;
  p.dst_img = p.dst_row * th;

  double ms[3] = {0.0, 0.0, 0.0};
  if (n_images || out_source_xy) {
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
    hipStream_t st = ctx->stream;
    // chunks of images under dsm_ctx_set_memory_budget: the map (when asked for) and one image always fit by definition
    const uint64_t map_bytes = out_source_xy ? tw * th * 16 : 0;
    const uint64_t per_image = p.src_img + p.dst_img;
    const uint64_t budget = ctx->memory_budget ? ctx->memory_budget : UD_DEFAULT_CHUNK_BYTES;
    uint64_t chunk = budget > map_bytes ? (budget - map_bytes) / (per_image + per_image / 8 + 1024) : 0;  // DevBuf rounds up by an eighth
    chunk = std::max<uint64_t>(1, std::min<uint64_t>(chunk, std::max<uint32_t>(n_images, 1)));
    HIPCHK(ctx, ctx->d_ud_src.reserve(UD_SRC_HEAD + chunk * p.src_img + 16));
    HIPCHK(ctx, ctx->d_ud_dst.reserve(chunk * p.dst_img + 16));
    if (out_source_xy) HIPCHK(ctx, ctx->d_ud_map.reserve(map_bytes));
    p.cams = ctx->d_ud_src.as<dsm_camera>();
    p.src = ctx->d_ud_src.as<uint8_t>() + UD_SRC_HEAD;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_ud_src.p, kernel_cams, sizeof(kernel_cams), hipMemcpyHostToDevice, st));
    p.dst = ctx->d_ud_dst.as<uint8_t>();
    DevEvents<4> ev;
    HIPCHK(ctx, ev.create());
    for (uint64_t first = 0; first < std::max<uint32_t>(n_images, 1); first += chunk) {
      const uint32_t cnt = (uint32_t)std::min<uint64_t>(chunk, n_images - std::min<uint64_t>(first, n_images));
      p.n_images = cnt;
      p.map = out_source_xy && first == 0 ? ctx->d_ud_map.as<double>() : nullptr;
      HIPCHK(ctx, hipEventRecord(ev[0], st));
      for (uint32_t i = 0; i < cnt; ++i)
        HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_ud_src.as<uint8_t>() + UD_SRC_HEAD + (size_t)i * p.src_img, p.src_row, src + (size_t)(first + i) * src_image_stride,
                                     src_row_stride, p.src_row, sh, hipMemcpyHostToDevice, st));
      HIPCHK(ctx, hipEventRecord(ev[1], st));
      hipLaunchKernelGGL(k_ud_warp, dim3((uint32_t)tiles), dim3(UD_BLOCK), 0, st, p);
      HIPCHK(ctx, hipGetLastError());
      HIPCHK(ctx, hipEventRecord(ev[2], st));
      for (uint32_t i = 0; i < cnt; ++i)
        HIPCHK(ctx, hipMemcpy2DAsync(dst + (size_t)(first + i) * dst_image_stride, dst_row_stride, ctx->d_ud_dst.as<uint8_t>() + (size_t)i * p.dst_img,
                                     p.dst_row, tw * channels, th, hipMemcpyDeviceToHost, st));
      if (p.map) HIPCHK(ctx, hipMemcpyAsync(out_source_xy, p.map, map_bytes, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipEventRecord(ev[3], st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      for (int k = 0; k < 3; ++k) {
        double t = 0;
        HIPCHK(ctx, ev.ms(k, k + 1, &t));
        ms[k] += t;
      }
    }
  }
  if (out_scaled_target_camera) *out_scaled_target_camera = scaled;
  if (out_needs_rescale) *out_needs_rescale = needs_rescale;
  mark_ready(ctx);
  for (int k = 0; k < 3; ++k) ctx->undistortion_ms[2 + k] = ms[k];
  return DSM_OK;
}

extern "C" int dsm_get_undistortion_time(dsm_ctx* ctx, double* stage_ms) {
  if (!ctx || !stage_ms) return DSM_ERR_INVALID_ARGUMENT;
  if (!ctx->undistortion_ready) return dsm_fail(ctx, DSM_ERR_NOT_READY, "dsm_get_undistortion_time: no undistortion call yet");
  memcpy(stage_ms, ctx->undistortion_ms, sizeof(ctx->undistortion_ms));
  return DSM_OK;
}
