// point_filter.hip -- the reconstruction's point and observation filters: FilterObservationsWithNegativeDepth,
// FilterPoints3DWithLargeReprojectionError, FilterPoints3DWithSmallTriangulationAngle, ComputeMeanReprojectionError(track_ids)
// and the verdict of FilterImages (src/base/reconstruction.cc:728-770, 814-858, 1352-1465), on the arrays of dsm_bundle_adjust.
//
//   k_pf_images     a thread per image: the normalised quaternion's rotation and the projection centre
//   k_pf_residuals  a thread per observation: depth (row 2 of the projection matrix . (X, 1)) and the squared reprojection error
//   k_pf_tracks     passes 1 and 2 per point, k_pf_angles pass 3, k_pf_means pass 8 -- each in two paths chosen on the host by the
//                   INPUT track length: a lane per point up to PF_LANE_CUT observations, a one-wave workgroup per point above it.
//                   Both paths run the same body (counts are lane-strided and wave-reduced, the in-order error sum is one lane's,
//                   the pairs of the angle test are spread over the lanes in the reference's order), so they give the same bytes.
//   k_pf_flags, k_pf_scan_block / k_pf_scan_add, k_pf_emit   the surviving tracks compacted: a fixed-block exclusive scan over
//                   the observations' keep flags (the pattern of retriangulation.hip's scan; its kernels are tied to its buffers
//                   and live in its translation unit, so these are new ones)
//   k_pf_verdict    FilterImages per image;  k_pf_reduce / k_pf_final   the report's counts (integer atomics) and the two means
//                   (block_reduce.h's fixed-order sums: a block per contiguous range of points, thread t of it adding points
//                   t, t + 256, ... of the range, a halving tree, then one block over the partials -- a fixed order for a given
//                   number of points, not the in-order sum)
// No floating-point atomics; a point's results depend on the point, its images and the options alone.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ba_project.h"
#include "block_reduce.h"
#include "camera_bogus.h"
#include "ctx.h"
#include "tri_angle.h"
#include "wave_reduce.h"

namespace {

// Tracks up to this many observations take the lane path.  Not measured: at 16 observations a lane walks at most 120 pairs,
// about two rounds of the wave path's 64, while the typical track (2 .. 10 views) stays far below it; a longer track in a lane
// would hold its 63 neighbours for the length of its pair loop.
constexpr uint32_t PF_LANE_CUT = 16;
constexpr int PF_BLOCK = 256;
constexpr uint32_t PF_SCAN = PF_BLOCK * 4;  // items of one scan block
constexpr int PF_REDUCE_BLOCKS = 256;       // at most: the partials of the two means
constexpr double kPfDegToRad = 0.0174532925199432954743716805978692718781530857086181640625;  // DegToRad, util/math.h
constexpr int PF_POSE = 15;                 // doubles per image: R (row-major), tvec, the projection centre
enum { PF_C_NF = 0, PF_C_PD = 3, PF_C_OD = 6, PF_C_LEN4 = 9, PF_C_NERR = 10, PF_C_PAIRS = 11, PF_C_KEPT = 12, PF_C_SEL = 13, PF_COUNTERS = 14 };

struct PfPoint {
  double err, sum4, mg_depth, mg_e2, mg_angle;
  uint64_t pairs;
  uint32_t nf[3], od[3], len4;
  uint8_t keep, sel, has_err, delpass;
};

struct PfParams {
  uint32_t N, P, n, passes;
  double thr2, min_angle;
  const dsm_camera* cams;
  const uint32_t* img_cam;
  const double* img_q;
  const double* img_t;
  double* pose;  // [N][PF_POSE]
  const double* xyz;
  const uint32_t* toff;
  const uint32_t* oimg;
  const double* oxy;
  const uint8_t* psel;  // NULL = all
  const uint8_t* isel;  // NULL = none
  double* depth;
  double* e2;
  uint32_t* opoint;
  uint8_t* alive;
  uint32_t* alist;  // [n]: the wave path's surviving image indices of a track, at the track's offset
  PfPoint* pts;
};

__device__ inline double pf_margin(double a, double thr) {
  if (!isfinite(a)) return INFINITY;
  const double den = fmax(fabs(a), fabs(thr));
  return den > 0.0 ? fabs(a - thr) / den : 0.0;
}

// the one instantiation of the projection this file carries (ba_project.h's double path)
__device__ __noinline__ void pf_project(int model, const double* prm, double u, double v, double* x, double* y) {
  ba_world_to_image<double>(model, prm, u, v, x, y);
}

// NormalizeQuaternion + Eigen's toRotationMatrix (pose.cc:75-91); ProjectionCenterFromPose as -R^T t
__global__ void __launch_bounds__(PF_BLOCK) k_pf_images(PfParams p) {
  const uint32_t i = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i >= p.N) return;
  const double* qv = p.img_q + 4 * (size_t)i;
  const double* tv = p.img_t + 3 * (size_t)i;
  const double nq = sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
  const double w = qv[0] / nq, x = qv[1] / nq, y = qv[2] / nq, z = qv[3] / nq;
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
               tyy = ty * y, tyz = tz * y, tzz = tz * z;
  const double R[9] = {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
  double* o = p.pose + (size_t)PF_POSE * i;
  for (int k = 0; k < 9; ++k) o[k] = R[k];
  for (int k = 0; k < 3; ++k) o[9 + k] = tv[k];
  for (int k = 0; k < 3; ++k) o[12 + k] = -((R[k] * tv[0] + R[3 + k] * tv[1]) + R[6 + k] * tv[2]);
}

// CalculateSquaredReprojectionError (projection.cc:119-136) per observation; its z is HasPointPositiveDepth's row-2 product
__global__ void __launch_bounds__(PF_BLOCK) k_pf_residuals(PfParams p) {
  const uint32_t o = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (o >= p.n) return;
  uint32_t lo = 0, hi = p.P - 1;  // the point of observation o: the smallest pid with toff[pid + 1] > o
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (p.toff[mid + 1] <= o)
      lo = mid + 1;
    else
      hi = mid;
  }
  p.opoint[o] = lo;
  const uint32_t img = p.oimg[o];
  const double* T = p.pose + (size_t)PF_POSE * img;
  const double* X = p.xyz + 3 * (size_t)lo;
  const double px = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[9];
  const double py = ((T[3] * X[0] + T[4] * X[1]) + T[5] * X[2]) + T[10];
  const double pz = ((T[6] * X[0] + T[7] * X[1]) + T[8] * X[2]) + T[11];
  p.depth[o] = pz;
  double e2 = DBL_MAX;
  if (!(pz < DBL_EPSILON)) {
    const dsm_camera* cam = p.cams + p.img_cam[img];
    double x, y;
    pf_project(cam->model_id, cam->params, px / pz, py / pz, &x, &y);
    const double dx = x - p.oxy[2 * (size_t)o], dy = y - p.oxy[2 * (size_t)o + 1];
    e2 = dx * dx + dy * dy;
  }
  p.e2[o] = e2;
}

// passes 1 and 2 of one point; W lanes share the point (lane 0 .. W - 1)
template <int W>
__device__ inline void pf_track(const PfParams& p, uint32_t pid, int lane) {
  const uint32_t b = p.toff[pid], L = p.toff[pid + 1] - b;
  uint32_t sel = p.psel ? (p.psel[pid] != 0) : 1u;
  if (p.isel && !sel) {
    uint32_t any = 0;
    for (uint32_t i = lane; i < L; i += W) any += p.isel[p.oimg[b + i]] != 0;
    sel = (W == 64 ? wave_sum(any) : any) != 0;
  }
  uint32_t n_neg = 0;
  double mgd = INFINITY;
  for (uint32_t i = lane; i < L; i += W) {
    const double d = p.depth[b + i];
    mgd = fmin(mgd, pf_margin(d, DBL_EPSILON));
    n_neg += d < DBL_EPSILON;
  }
  if (W == 64) n_neg = wave_sum(n_neg);
  if (W == 64) mgd = wave_fmin(mgd);
  if (!((p.passes & 1u) || (sel && (p.passes & 10u)))) mgd = INFINITY;
  bool keep = true, drop_neg = false, drop_err = false;
  uint32_t len = L, nf1 = 0, od1 = 0, nf2 = 0, od2 = 0, delpass = 0;
  // pass 1, the closed form of the walk with DeleteObservation: the k-th negative meets a track of L - (k - 1) elements and
  // deletes the point once that is <= 2; a point without a negative is never visited
  if ((p.passes & 1u) && n_neg > 0) {
    if (L >= n_neg + 2) {
      drop_neg = true;
      nf1 = od1 = n_neg;
      len = L - n_neg;
    } else {
      keep = false;
      delpass = 1;
      nf1 = min(n_neg, max(L - 1, 1u));
      od1 = L;
    }
  }
  double err = -1.0, mge = INFINITY;
  if (keep && sel && (p.passes & 2u)) {
    if (len < 2) {
      keep = false;
      delpass = 2;
      nf2 = od2 = len;
    } else {
      uint32_t marked = 0;
      for (uint32_t i = lane; i < L; i += W) {
        if (drop_neg && p.depth[b + i] < DBL_EPSILON) continue;
        const double e = p.e2[b + i];
        if (e != DBL_MAX) mge = fmin(mge, pf_margin(e, p.thr2));
        marked += e > p.thr2;
      }
      if (W == 64) marked = wave_sum(marked);
      if (W == 64) mge = wave_fmin(mge);
      if (marked >= len - 1) {
        keep = false;
        delpass = 2;
        nf2 = od2 = len;
      } else {
        drop_err = true;
        nf2 = od2 = marked;
        len -= marked;
        if (lane == 0) {  // the in-order sum over the kept elements, in input track order
          double s = 0.0;
          for (uint32_t i = 0; i < L; ++i) {
            if (drop_neg && p.depth[b + i] < DBL_EPSILON) continue;
            const double e = p.e2[b + i];
            if (e > p.thr2) continue;
            s += sqrt(e);
          }
          err = s / (double)len;  // SetError after the deletions: the remaining length
        }
      }
    }
  }
  for (uint32_t i = lane; i < L; i += W)
    p.alive[b + i] = keep && !(drop_neg && p.depth[b + i] < DBL_EPSILON) && !(drop_err && p.e2[b + i] > p.thr2);
  if (lane == 0) {
    PfPoint* q = p.pts + pid;
    q->err = err;
    q->sum4 = 0.0;
    q->mg_depth = mgd;
    q->mg_e2 = mge;
    q->mg_angle = INFINITY;
    q->pairs = 0;
    q->nf[0] = nf1;
    q->nf[1] = nf2;
    q->nf[2] = 0;
    q->od[0] = od1;
    q->od[1] = od2;
    q->od[2] = 0;
    q->len4 = 0;
    q->keep = keep;
    q->sel = (uint8_t)sel;
    q->has_err = drop_err;
    q->delpass = (uint8_t)delpass;
  }
}

// pass 3 of one point
template <int W>
__device__ inline void pf_angles(const PfParams& p, uint32_t pid, int lane) {
  PfPoint* q = p.pts + pid;
  if (!q->keep || !q->sel) return;
  const uint32_t b = p.toff[pid], L = p.toff[pid + 1] - b;
  const double X[3] = {p.xyz[3 * (size_t)pid], p.xyz[3 * (size_t)pid + 1], p.xyz[3 * (size_t)pid + 2]};
  bool found = false;
  double mg = INFINITY;
  uint64_t pairs = 0;
  uint32_t M = 0;
  if constexpr (W == 1) {  // the reference's loops over the surviving elements
    for (uint32_t i1 = 0; i1 < L && !found; ++i1) {
      if (!p.alive[b + i1]) continue;
      ++M;
      const double* c1 = p.pose + (size_t)PF_POSE * p.oimg[b + i1] + 12;
      for (uint32_t i2 = 0; i2 < i1; ++i2) {
        if (!p.alive[b + i2]) continue;
        const double a = tri_angle_libm(c1, p.pose + (size_t)PF_POSE * p.oimg[b + i2] + 12, X);
        ++pairs;
        const double m = pf_margin(a, p.min_angle);
        if (a >= p.min_angle) {
          found = true;
          mg = m;
          break;
        }
        mg = fmin(mg, m);
      }
    }
    if (!found) {
      M = 0;
      for (uint32_t i = 0; i < L; ++i) M += p.alive[b + i] != 0;
    }
  } else {
    // the surviving elements' images, compacted in track order; then pair k = i1 (i1 - 1) / 2 + i2 (the reference's order) on
    // lane k % 64, a round of 64 at a time, out at the first round with a passing pair
    for (uint32_t c = 0; c < L; c += 64) {
      const uint32_t i = c + lane;
      const bool al = i < L && p.alive[b + i];
      const unsigned long long mask = __ballot(al);
      if (al) p.alist[b + M + __popcll(mask & ((1ull << lane) - 1ull))] = p.oimg[b + i];
      M += __popcll(mask);
    }
    __syncthreads();
    const uint64_t total = (uint64_t)M * (M - (M > 0)) / 2;
    for (uint64_t base = 0; base < total && !found; base += 64) {
      const uint64_t k = base + lane;
      bool pass = false;
      double m = INFINITY;
      if (k < total) {
        uint64_t i1 = (uint64_t)((1.0 + sqrt(1.0 + 8.0 * (double)k)) * 0.5);
        while (i1 * (i1 - 1) / 2 > k) --i1;
        while ((i1 + 1) * i1 / 2 <= k) ++i1;
        const uint64_t i2 = k - i1 * (i1 - 1) / 2;
        const double a = tri_angle_libm(p.pose + (size_t)PF_POSE * p.alist[b + i1] + 12, p.pose + (size_t)PF_POSE * p.alist[b + i2] + 12, X);
        m = pf_margin(a, p.min_angle);
        pass = a >= p.min_angle;
      }
      const unsigned long long won = __ballot(pass);
      if (won) {
        const int first = __ffsll((long long)won) - 1;
        mg = __shfl(m, first);
        pairs += (uint64_t)first + 1;
        found = true;
      } else {
        mg = fmin(mg, wave_fmin(m));
        pairs += min((uint64_t)64, total - base);
      }
    }
  }
  if (lane == 0) {
    q->mg_angle = mg;
    q->pairs = pairs;
    if (!found) {
      q->keep = 0;
      q->delpass = 3;
      q->nf[2] = 1;
      q->od[2] = M;
      q->err = -1.0;
      q->has_err = 0;
    }
  }
}

// pass 8 of one point: ComputeMeanReprojectionError(track_ids)'s per-point half
template <int W>
__device__ inline void pf_mean(const PfParams& p, uint32_t pid, int lane) {
  PfPoint* q = p.pts + pid;
  if (!q->keep || !q->sel) return;
  const uint32_t b = p.toff[pid], L = p.toff[pid + 1] - b;
  uint32_t len = 0;
  for (uint32_t i = lane; i < L; i += W) len += p.alive[b + i] != 0;
  if (W == 64) len = wave_sum(len);
  if (lane != 0) return;
  double s = 0.0;
  for (uint32_t i = 0; i < L; ++i) {
    if (!p.alive[b + i]) continue;
    const double e = p.e2[b + i];
    if (e == DBL_MAX) continue;
    s += sqrt(e);
  }
  q->err = s / (double)len;
  q->has_err = 1;
  q->sum4 = s;
  q->len4 = len;
}

template <int STAGE>
__global__ void __launch_bounds__(PF_BLOCK) k_pf_lane(PfParams p, const uint32_t* __restrict__ list, uint32_t count) {
  const uint32_t i = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i >= count) return;
  if (STAGE == 0) pf_track<1>(p, list[i], 0);
  if (STAGE == 1) pf_angles<1>(p, list[i], 0);
  if (STAGE == 2) pf_mean<1>(p, list[i], 0);
}
template <int STAGE>
__global__ void __launch_bounds__(64) k_pf_wave(PfParams p, const uint32_t* __restrict__ list, uint32_t count) {
  if (blockIdx.x >= count) return;
  if (STAGE == 0) pf_track<64>(p, list[blockIdx.x], threadIdx.x);
  if (STAGE == 1) pf_angles<64>(p, list[blockIdx.x], threadIdx.x);
  if (STAGE == 2) pf_mean<64>(p, list[blockIdx.x], threadIdx.x);
}

// flag[o] = observation o survives (o = n: 0, so that the scan's last entry is the total)
__global__ void __launch_bounds__(PF_BLOCK) k_pf_flags(PfParams p, uint32_t* __restrict__ flag, uint8_t* __restrict__ okeep) {
  const uint32_t o = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (o > p.n) return;
  uint32_t f = 0;
  if (o < p.n) {
    f = p.pts[p.opoint[o]].keep && p.alive[o];
    okeep[o] = (uint8_t)f;
  }
  flag[o] = f;
}

// exclusive scan of n counts in blocks of PF_SCAN; block totals to sums (scanned by the next level)
__global__ void __launch_bounds__(PF_BLOCK) k_pf_scan_block(uint32_t n, const uint32_t* __restrict__ in, uint32_t* __restrict__ out,
                                                            uint32_t* __restrict__ sums) {
  __shared__ uint32_t sh[PF_BLOCK];
  const uint32_t base = blockIdx.x * PF_SCAN + threadIdx.x * 4;
  uint32_t v[4], t = 0;
  for (int i = 0; i < 4; ++i) {
    v[i] = base + i < n ? in[base + i] : 0u;
    t += v[i];
  }
  sh[threadIdx.x] = t;
  __syncthreads();
  for (int d = 1; d < PF_BLOCK; d *= 2) {
    const uint32_t x = threadIdx.x >= (uint32_t)d ? sh[threadIdx.x - d] : 0u;
    __syncthreads();
    sh[threadIdx.x] += x;
    __syncthreads();
  }
  uint32_t run = sh[threadIdx.x] - t;
  for (int i = 0; i < 4; ++i) {
    if (base + i < n) out[base + i] = run;
    run += v[i];
  }
  if (threadIdx.x == PF_BLOCK - 1) sums[blockIdx.x] = sh[threadIdx.x];
}
__global__ void __launch_bounds__(PF_BLOCK) k_pf_scan_add(uint32_t n, uint32_t* __restrict__ out, const uint32_t* __restrict__ sums) {
  const uint32_t i = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i < n) out[i] += sums[i / PF_SCAN];
}

// the compacted tracks: kept_obs at the scanned positions, kept_track_offsets = the scan at the tracks' starts; the images that
// still observe a point (every writer stores the same 1)
__global__ void __launch_bounds__(PF_BLOCK) k_pf_emit(PfParams p, const uint32_t* __restrict__ flag, const uint32_t* __restrict__ pos,
                                                      uint32_t* __restrict__ kobs, uint32_t* __restrict__ koff, uint8_t* __restrict__ img_has) {
  const uint32_t i = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i < p.n && flag[i]) {
    kobs[pos[i]] = i;
    img_has[p.oimg[i]] = 1;
  }
  if (i <= p.P) koff[i] = pos[p.toff[i]];
}

__global__ void __launch_bounds__(PF_BLOCK) k_pf_verdict(uint32_t N, const uint32_t* __restrict__ img_cam, const uint8_t* __restrict__ reg,
                                                         const uint8_t* __restrict__ img_has, const uint8_t* __restrict__ cam_bogus,
                                                         uint8_t* __restrict__ filtered) {
  const uint32_t i = blockIdx.x * PF_BLOCK + threadIdx.x;
  if (i >= N) return;
  filtered[i] = (!reg || reg[i]) && (!img_has[i] || cam_bogus[img_cam[i]]);
}

// Block k takes the points [k * chunk, (k + 1) * chunk): the per-point results out (keep, error), the counts to ctr (integer
// atomics), the margins' minima to mg (atomicMin on the bit patterns: non-negative doubles order like their bits), and the
// block's partials of the two sums to part[0 .. nb), part[nb .. 2 nb)
__global__ void __launch_bounds__(PF_BLOCK) k_pf_reduce(uint32_t P, uint32_t chunk, const PfPoint* __restrict__ pts, uint8_t* __restrict__ pkeep,
                                                        double* __restrict__ perr, unsigned long long* __restrict__ ctr,
                                                        unsigned long long* __restrict__ mg, double* __restrict__ part) {
  __shared__ double sh[2 * PF_BLOCK];
  const uint32_t lo = blockIdx.x * chunk, hi = min(P, lo + chunk);
  uint64_t c[PF_COUNTERS];
  for (int k = 0; k < PF_COUNTERS; ++k) c[k] = 0;
  double v[2] = {0.0, 0.0}, m[3] = {INFINITY, INFINITY, INFINITY};
  for (uint32_t i = lo + threadIdx.x; i < hi; i += PF_BLOCK) {
    const PfPoint q = pts[i];
    pkeep[i] = q.keep;
    perr[i] = q.err;
    for (int k = 0; k < 3; ++k) {
      c[PF_C_NF + k] += q.nf[k];
      c[PF_C_OD + k] += q.od[k];
      c[PF_C_PD + k] += q.delpass == k + 1;
    }
    c[PF_C_LEN4] += q.len4;
    c[PF_C_PAIRS] += q.pairs;
    c[PF_C_KEPT] += q.keep;
    c[PF_C_SEL] += q.sel;
    v[0] += q.sum4;
    if (q.keep && q.has_err) {
      c[PF_C_NERR] += 1;
      v[1] += q.err;
    }
    m[0] = fmin(m[0], q.mg_depth);
    m[1] = fmin(m[1], q.mg_e2);
    m[2] = fmin(m[2], q.mg_angle);
  }
  for (int k = 0; k < PF_COUNTERS; ++k) {
    const uint64_t s = wave_sum(c[k]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&ctr[k], (unsigned long long)s);
  }
  for (int k = 0; k < 3; ++k) {
    const double s = wave_fmin(m[k]);
    if ((threadIdx.x & 63) == 0) atomicMin(&mg[k], (unsigned long long)__double_as_longlong(s));
  }
  write_partials<PF_BLOCK, 2>(v, sh, part);
}
__global__ void __launch_bounds__(PF_BLOCK) k_pf_final(uint32_t nb, const double* __restrict__ part, double* __restrict__ sums) {
  __shared__ double sh[2 * PF_BLOCK];
  double out[2];
  sum_partials<PF_BLOCK, 2, uint32_t>(part, nb, out, sh);
  if (threadIdx.x == 0) {
    sums[0] = out[0];
    sums[1] = out[1];
  }
}

struct PfBufs {
  DevBuf cams, img_cam, img_q, img_t, reg, pose, xyz, toff, oimg, oxy, psel, isel, depth, e2, opoint, alive, alist, pts;
  DevBuf lane_list, wave_list, flag, pos, scan_s[4], scan_x[4], kobs, koff, okeep, img_has, cam_bogus, filtered, pkeep, perr, ctr, part;
};

// d.pos[0 .. n) = exclusive scan of d.flag[0 .. n) in fixed blocks: level l scans the block totals of level l - 1
hipError_t pf_scan(PfBufs& d, uint32_t n, hipStream_t st) {
  hipError_t e = d.pos.reserve((size_t)n * 4 + 16);
  std::vector<uint32_t> lens{n};
  while (lens.back() > PF_SCAN) lens.push_back((lens.back() + PF_SCAN - 1) / PF_SCAN);
  if (lens.size() > 4) return hipErrorInvalidValue;
  for (size_t l = 0; l < lens.size() && e == hipSuccess; ++l) {
    e = d.scan_s[l].reserve(((size_t)(lens[l] + PF_SCAN - 1) / PF_SCAN) * 4 + 16);
    if (e == hipSuccess) e = d.scan_x[l].reserve((size_t)lens[l] * 4 + 16);
  }
  if (e != hipSuccess) return e;
  std::vector<uint32_t*> outs;
  const uint32_t* in = d.flag.as<uint32_t>();
  for (size_t l = 0; l < lens.size(); ++l) {
    uint32_t* out = l == 0 ? d.pos.as<uint32_t>() : d.scan_x[l].as<uint32_t>();
    hipLaunchKernelGGL(k_pf_scan_block, dim3((lens[l] + PF_SCAN - 1) / PF_SCAN), dim3(PF_BLOCK), 0, st, lens[l], in, out,
                       d.scan_s[l].as<uint32_t>());
    outs.push_back(out);
    in = d.scan_s[l].as<uint32_t>();
  }
  for (size_t l = outs.size(); l-- > 1;)
    hipLaunchKernelGGL(k_pf_scan_add, dim3((lens[l - 1] + PF_BLOCK - 1) / PF_BLOCK), dim3(PF_BLOCK), 0, st, lens[l - 1], outs[l - 1], outs[l]);
  return hipGetLastError();
}


}  // namespace

extern "C" void dsm_default_point_filter_options(dsm_point_filter_options* o) {
  o->max_reproj_error = 4.0;        // IncrementalMapper::Options::filter_max_reproj_error, DistributedMapperController::Options
  o->min_tri_angle = 1.5;           // filter_min_tri_angle
  o->min_focal_length_ratio = 0.1;  // incremental_mapper.h:106-108
  o->max_focal_length_ratio = 10.0;
  o->max_extra_param = 1.0;
  o->passes = DSM_FILTER_REPROJECTION_ERROR | DSM_FILTER_TRIANGULATION_ANGLE;  // FilterAllPoints3D / FilterPoints3D
  o->reserved = 0;
}

extern "C" int dsm_filter_points3D(dsm_ctx* ctx, uint32_t num_cameras, const dsm_camera* cameras, uint32_t num_images,
                                   const uint32_t* image_camera, const double* image_qvec, const double* image_tvec,
                                   const uint8_t* image_registered, uint32_t num_points, const double* point_xyz,
                                   const uint32_t* track_offsets, const uint32_t* obs_image, const double* obs_xy,
                                   const uint8_t* point_selected, const uint8_t* image_selected,
                                   const dsm_point_filter_options* options, uint8_t* point_keep, uint8_t* obs_keep,
                                   double* point_error, uint32_t* kept_track_offsets, uint32_t* kept_obs, uint8_t* image_filtered,
                                   dsm_point_filter_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_filter_points3D", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  const uint32_t C = num_cameras, N = num_images, P = num_points;
  if (!track_offsets || (C && !cameras) || (N && (!image_camera || !image_qvec || !image_tvec)) || (P && !point_xyz))
    return fail("NULL argument");
  dsm_point_filter_options o;
  if (options)
    o = *options;
  else
    dsm_default_point_filter_options(&o);
  if (o.passes == 0 || o.passes > 15) return fail("passes must be 1 .. 15");
  for (double v : {o.max_reproj_error, o.min_tri_angle, o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param})
    if (!(v >= 0.0) || !std::isfinite(v)) return fail("a negative or non-finite threshold");
  if (track_offsets[0] != 0) return fail("track_offsets must start at 0");
  for (uint32_t i = 0; i < P; ++i)
    if (track_offsets[i + 1] < track_offsets[i]) return fail("track_offsets must ascend");
  const uint32_t n = track_offsets[P];
  if (n >= 0x7fffffffu) return fail("too many observations");
  if (n && (!obs_image || !obs_xy)) return fail("NULL argument");
  dsm_point_filter_report rep{};
  rep.num_points = P;
  rep.num_observations = n;
  rep.min_depth_margin = rep.min_error_margin = rep.min_angle_margin = rep.min_bogus_margin = INFINITY;
  rep.mean_reprojection_error = NAN;
  std::vector<uint8_t> cam_bogus(std::max<uint32_t>(C, 1), 0);
  for (uint32_t c = 0; c < C; ++c) {
    const dsm_camera& k = cameras[c];
    if (!cam_model_exists(k.model_id)) return fail("an unknown camera model");
    for (int i = 0; i < cam_num_params(k.model_id); ++i)
      if (!std::isfinite(k.params[i])) return fail("non-finite camera parameters");
    cam_bogus[c] = cam_has_bogus_params(k, o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param, &rep.min_bogus_margin);
  }
  for (uint32_t i = 0; i < N; ++i) {
    if (image_camera[i] >= C) return fail("an image on a camera index out of range");
    const double* qv = image_qvec + 4 * (size_t)i;
    for (int k = 0; k < 4; ++k)
      if (!std::isfinite(qv[k])) return fail("non-finite qvec");
    for (int k = 0; k < 3; ++k)
      if (!std::isfinite(image_tvec[3 * (size_t)i + k])) return fail("non-finite tvec");
    if (std::sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]) == 0) return fail("a zero qvec");
  }
  for (size_t i = 0; i < 3 * (size_t)P; ++i)
    if (!std::isfinite(point_xyz[i])) return fail("non-finite point xyz");
  for (uint32_t i = 0; i < n; ++i) {
    if (obs_image[i] >= N) return fail("an observation in an image index out of range");
    if (image_registered && !image_registered[obs_image[i]]) return fail("an observation in an unregistered image");
    if (!std::isfinite(obs_xy[2 * (size_t)i]) || !std::isfinite(obs_xy[2 * (size_t)i + 1])) return fail("non-finite observation");
  }
  // the path bins, by the input track length alone
  std::vector<uint32_t> lane_list, wave_list;
  lane_list.reserve(P);
  for (uint32_t i = 0; i < P; ++i) (track_offsets[i + 1] - track_offsets[i] <= PF_LANE_CUT ? lane_list : wave_list).push_back(i);
  rep.lane_path_tracks = lane_list.size();
  rep.wave_path_tracks = wave_list.size();
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  PfBufs d;
  DevEvents<8> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  HIPCHK(ctx, dev_upload(d.cams, cameras, (size_t)C * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.cam_bogus, cam_bogus.data(), cam_bogus.size(), st));
  HIPCHK(ctx, dev_upload(d.img_cam, image_camera, (size_t)N * 4, st));
  HIPCHK(ctx, dev_upload(d.img_q, image_qvec, (size_t)N * 32, st));
  HIPCHK(ctx, dev_upload(d.img_t, image_tvec, (size_t)N * 24, st));
  if (image_registered) HIPCHK(ctx, dev_upload(d.reg, image_registered, N, st));
  HIPCHK(ctx, dev_upload(d.xyz, point_xyz, (size_t)P * 24, st));
  HIPCHK(ctx, dev_upload(d.toff, track_offsets, ((size_t)P + 1) * 4, st));
  HIPCHK(ctx, dev_upload(d.oimg, obs_image, (size_t)n * 4, st));
  HIPCHK(ctx, dev_upload(d.oxy, obs_xy, (size_t)n * 16, st));
  if (point_selected) HIPCHK(ctx, dev_upload(d.psel, point_selected, P, st));
  if (image_selected) HIPCHK(ctx, dev_upload(d.isel, image_selected, N, st));
  HIPCHK(ctx, dev_upload(d.lane_list, lane_list.data(), lane_list.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.wave_list, wave_list.data(), wave_list.size() * 4, st));
  HIPCHK(ctx, d.pose.reserve(std::max<size_t>(N, 1) * PF_POSE * 8));
  HIPCHK(ctx, d.depth.reserve((size_t)n * 8 + 16));
  HIPCHK(ctx, d.e2.reserve((size_t)n * 8 + 16));
  HIPCHK(ctx, d.opoint.reserve((size_t)n * 4 + 16));
  HIPCHK(ctx, d.alive.reserve((size_t)n + 16));
  HIPCHK(ctx, d.alist.reserve((size_t)n * 4 + 16));
  HIPCHK(ctx, d.pts.reserve(std::max<size_t>(P, 1) * sizeof(PfPoint)));
  HIPCHK(ctx, d.flag.reserve(((size_t)n + 1) * 4 + 16));
  HIPCHK(ctx, d.kobs.reserve((size_t)n * 4 + 16));
  HIPCHK(ctx, d.koff.reserve(((size_t)P + 1) * 4 + 16));
  HIPCHK(ctx, d.okeep.reserve((size_t)n + 16));
  HIPCHK(ctx, dev_fill(d.img_has, 0, N, st));
  HIPCHK(ctx, d.filtered.reserve((size_t)N + 16));
  HIPCHK(ctx, d.pkeep.reserve((size_t)P + 16));
  HIPCHK(ctx, d.perr.reserve((size_t)P * 8 + 16));
  // counters, then the three margins' bit patterns (INFINITY), then the two sums
  const uint32_t nb = std::max<uint32_t>(1, std::min<uint32_t>(PF_REDUCE_BLOCKS, dsm_grid(P, PF_BLOCK)));
  const uint32_t chunk = (P + nb - 1) / nb;
  std::vector<unsigned long long> ctr0(PF_COUNTERS + 3 + 2, 0);
  {
    const double inf = INFINITY;
    for (int k = 0; k < 3; ++k) memcpy(&ctr0[PF_COUNTERS + k], &inf, 8);
  }
  HIPCHK(ctx, dev_upload(d.ctr, ctr0.data(), ctr0.size() * 8, st));
  HIPCHK(ctx, d.part.reserve((size_t)2 * nb * 8));

  PfParams prm;
  prm.N = N;
  prm.P = P;
  prm.n = n;
  prm.passes = o.passes;
  prm.thr2 = o.max_reproj_error * o.max_reproj_error;
  prm.min_angle = o.min_tri_angle * kPfDegToRad;
  prm.cams = d.cams.as<dsm_camera>();
  prm.img_cam = d.img_cam.as<uint32_t>();
  prm.img_q = d.img_q.as<double>();
  prm.img_t = d.img_t.as<double>();
  prm.pose = d.pose.as<double>();
  prm.xyz = d.xyz.as<double>();
  prm.toff = d.toff.as<uint32_t>();
  prm.oimg = d.oimg.as<uint32_t>();
  prm.oxy = d.oxy.as<double>();
  prm.psel = point_selected ? d.psel.as<uint8_t>() : nullptr;
  prm.isel = image_selected ? d.isel.as<uint8_t>() : nullptr;
  prm.depth = d.depth.as<double>();
  prm.e2 = d.e2.as<double>();
  prm.opoint = d.opoint.as<uint32_t>();
  prm.alive = d.alive.as<uint8_t>();
  prm.alist = d.alist.as<uint32_t>();
  prm.pts = d.pts.as<PfPoint>();
  const uint32_t nl = (uint32_t)lane_list.size(), nw = (uint32_t)wave_list.size();
  const uint32_t* ll = d.lane_list.as<uint32_t>();
  const uint32_t* wl = d.wave_list.as<uint32_t>();
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  if (N) hipLaunchKernelGGL(k_pf_images, dim3(dsm_grid(N, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm);
  if (n) hipLaunchKernelGGL(k_pf_residuals, dim3(dsm_grid(n, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm);
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  if (nl) hipLaunchKernelGGL(k_pf_lane<0>, dim3(dsm_grid(nl, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm, ll, nl);
  if (nw) hipLaunchKernelGGL(k_pf_wave<0>, dim3(nw), dim3(64), 0, st, prm, wl, nw);
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  if (o.passes & DSM_FILTER_TRIANGULATION_ANGLE) {
    if (nl) hipLaunchKernelGGL(k_pf_lane<1>, dim3(dsm_grid(nl, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm, ll, nl);
    if (nw) hipLaunchKernelGGL(k_pf_wave<1>, dim3(nw), dim3(64), 0, st, prm, wl, nw);
  }
  HIPCHK(ctx, hipEventRecord(ev[4], st));
  if (o.passes & DSM_FILTER_MEAN_ERROR) {
    if (nl) hipLaunchKernelGGL(k_pf_lane<2>, dim3(dsm_grid(nl, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm, ll, nl);
    if (nw) hipLaunchKernelGGL(k_pf_wave<2>, dim3(nw), dim3(64), 0, st, prm, wl, nw);
  }
  HIPCHK(ctx, hipEventRecord(ev[5], st));
  hipLaunchKernelGGL(k_pf_flags, dim3(dsm_grid((uint64_t)n + 1, PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm, d.flag.as<uint32_t>(), d.okeep.as<uint8_t>());
  HIPCHK(ctx, pf_scan(d, n + 1, st));
  hipLaunchKernelGGL(k_pf_emit, dim3(dsm_grid(std::max<uint64_t>(n, (uint64_t)P + 1), PF_BLOCK)), dim3(PF_BLOCK), 0, st, prm, d.flag.as<uint32_t>(),
                     d.pos.as<uint32_t>(), d.kobs.as<uint32_t>(), d.koff.as<uint32_t>(), d.img_has.as<uint8_t>());
  if (N)
    hipLaunchKernelGGL(k_pf_verdict, dim3(dsm_grid(N, PF_BLOCK)), dim3(PF_BLOCK), 0, st, N, prm.img_cam, image_registered ? d.reg.as<uint8_t>() : nullptr,
                       d.img_has.as<uint8_t>(), d.cam_bogus.as<uint8_t>(), d.filtered.as<uint8_t>());
  unsigned long long* ctr = d.ctr.as<unsigned long long>();
  hipLaunchKernelGGL(k_pf_reduce, dim3(nb), dim3(PF_BLOCK), 0, st, P, chunk, prm.pts, d.pkeep.as<uint8_t>(), d.perr.as<double>(), ctr,
                     ctr + PF_COUNTERS, d.part.as<double>());
  hipLaunchKernelGGL(k_pf_final, dim3(1), dim3(PF_BLOCK), 0, st, nb, d.part.as<double>(), reinterpret_cast<double*>(ctr + PF_COUNTERS + 3));
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[6], st));
  std::vector<unsigned long long> ctr1(ctr0.size());
  std::vector<uint8_t> filt(N);
  uint32_t kept_total = 0;
  HIPCHK(ctx, hipMemcpyAsync(ctr1.data(), d.ctr.p, ctr1.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(&kept_total, d.koff.as<uint32_t>() + P, 4, hipMemcpyDeviceToHost, st));
  if (N) HIPCHK(ctx, hipMemcpyAsync(filt.data(), d.filtered.p, N, hipMemcpyDeviceToHost, st));
  if (point_keep && P) HIPCHK(ctx, hipMemcpyAsync(point_keep, d.pkeep.p, P, hipMemcpyDeviceToHost, st));
  if (point_error && P) HIPCHK(ctx, hipMemcpyAsync(point_error, d.perr.p, (size_t)P * 8, hipMemcpyDeviceToHost, st));
  if (obs_keep && n) HIPCHK(ctx, hipMemcpyAsync(obs_keep, d.okeep.p, n, hipMemcpyDeviceToHost, st));
  if (kept_track_offsets) HIPCHK(ctx, hipMemcpyAsync(kept_track_offsets, d.koff.p, ((size_t)P + 1) * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  if (kept_obs && kept_total) HIPCHK(ctx, hipMemcpyAsync(kept_obs, d.kobs.p, (size_t)kept_total * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[7], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (int k = 0; k < 3; ++k) {
    rep.num_filtered[k] = ctr1[PF_C_NF + k];
    rep.points_deleted[k] = ctr1[PF_C_PD + k];
    rep.observations_deleted[k] = ctr1[PF_C_OD + k];
  }
  rep.num_selected = ctr1[PF_C_SEL];
  rep.num_points_kept = ctr1[PF_C_KEPT];
  rep.num_observations_kept = kept_total;
  rep.pairs_evaluated = ctr1[PF_C_PAIRS];
  rep.mean_error_observations = ctr1[PF_C_LEN4];
  double mg[3], sums[2];
  memcpy(mg, &ctr1[PF_COUNTERS], 24);
  memcpy(sums, &ctr1[PF_COUNTERS + 3], 16);
  rep.min_depth_margin = mg[0];
  rep.min_error_margin = mg[1];
  rep.min_angle_margin = mg[2];
  if (o.passes & DSM_FILTER_MEAN_ERROR) rep.mean_reprojection_error = sums[0] / (double)ctr1[PF_C_LEN4];  // 0 / 0 = NaN, as the reference's
  rep.mean_point_error = ctr1[PF_C_NERR] ? sums[1] / (double)ctr1[PF_C_NERR] : 0.0;
  for (uint32_t i = 0; i < N; ++i) {
    rep.num_images_filtered += filt[i];
    if (image_filtered) image_filtered[i] = filt[i];
  }
  double t[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 7; ++i) HIPCHK(ctx, ev.ms(i, i + 1, &t[i]));
  HIPCHK(ctx, ev.ms(0, 7, &rep.device_ms));
  rep.upload_ms = t[0];
  rep.residuals_ms = t[1];
  rep.tracks_ms = t[2] + t[4];
  rep.angles_ms = t[3];
  rep.compaction_ms = t[5];
  rep.download_ms = t[6];
  if (report) *report = rep;
  return DSM_OK;
}
