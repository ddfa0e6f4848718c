// rt_loransac.h -- EstimateTriangulation on one lane, once, for the kernels of retriangulation.hip (Create: the
// angular residual) and of track_update.hip (CompleteImage: the reprojection residual).
//   EstimateTriangulation, TriangulationEstimator                   src/estimators/triangulation.cc
//   LORANSAC + InlierSupportMeasurer + CombinationSampler           src/optim/loransac.h:91-233, combination_sampler.cc
//   TriangulatePoint / TriangulateMultiViewPoint / CalculateTriangulationAngle   src/base/triangulation.cc
// The residual is a compile-time parameter of the lane (RtLaneT<Res>): Res()(view, feature, X, max_residual, margins) returns
// the squared residual of one entry and, where margins is not NULL, folds the margin of its inlier test into them.  The
// sampler, the two-view and the multi-view estimate, the depth test, the angle and the support comparison do not depend on it.
// The includer includes ctx.h / dagsfm_mi355x.h first.
#ifndef DAGSFM_AMD_CSRC_RT_LORANSAC_H_
#define DAGSFM_AMD_CSRC_RT_LORANSAC_H_

#include <float.h>
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "tri_angle.h"
#include "verify_camera.h"
#include "verify_linalg.h"

namespace {

constexpr int kRtMargins = 5;                  // residual, support, angle, depth, continue
constexpr double kRtCosineEdge = 1.0 - 8 * DBL_EPSILON;  // above: acos may be NaN by rounding alone (margin 0)
constexpr double kRtDegToRad = 0.0174532925199432954743716805978692718032360229492187;  // DegToRad, util/math.h

struct RtParams {
  double max_residual;        // create_max_angle_error^2 (rad^2), or complete_max_reproj_error^2 (px^2)
  double min_tri_angle;       // rad
  double continue_max_error;  // rad
  int32_t ignore_two_view;
  int32_t max_trials;         // ransac max_num_trials
  uint32_t tab_n;             // dynamic-trial table covers n <= tab_n
  uint32_t num_points;        // existing points: internal ids < num_points, new points num_points + slot
};

// Camera::ImageToWorld of every feature of a usable image (registered, camera without bogus parameters)
__global__ void k_rt_normalize(uint32_t F, const uint32_t* __restrict__ feat_img, const uint8_t* __restrict__ img_ok,
                               const uint32_t* __restrict__ img_cam, const dsm_camera* __restrict__ cams, const double* __restrict__ xy,
                               double* __restrict__ uv) {
  const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  const uint32_t im = feat_img[f];
  double u = NAN, v = NAN;
  if (img_ok[im]) {
    const dsm_camera cam = cams[img_cam[im]];
    image_to_world(cam, xy[2 * f], xy[2 * f + 1], &u, &v);
  }
  uv[2 * f] = u;
  uv[2 * f + 1] = v;
}

// ------------------------------------------------------------------ geometry (one lane)
struct RtView {
  double P[12];  // row-major 3 x 4
  double C[3];
  double u, v;
};

__device__ inline void rt_load(uint32_t f, const uint32_t* feat_img, const double* img_P, const double* img_C, const double* uv, RtView* w) {
  const uint32_t im = feat_img[f];
#pragma unroll
  for (int i = 0; i < 12; ++i) w->P[i] = img_P[12 * im + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) w->C[i] = img_C[3 * im + i];
  w->u = uv[2 * f];
  w->v = uv[2 * f + 1];
}

__device__ inline double rt_row(const double* P, int r, const double* X) {
  return P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3];
}

// CalculateNormalizedAngularError (projection.cc:185-191), squared; *cosine = the argument of acos.  A cosine that rounds
// above 1 gives NaN (an outlier, as in the reference) where the exact value is an inlier.
__device__ inline double rt_residual(const RtView& w, const double* X, double* cosine = nullptr) {
  const double r1n = sqrt((w.u * w.u + w.v * w.v) + 1.0);
  const double a0 = rt_row(w.P, 0, X), a1 = rt_row(w.P, 1, X), a2 = rt_row(w.P, 2, X);
  const double r2n = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
  const double d = ((w.u / r1n) * (a0 / r2n) + (w.v / r1n) * (a1 / r2n)) + (1.0 / r1n) * (a2 / r2n);
  if (cosine) *cosine = d;
  const double e = acos(d);
  return e * e;
}

// ResidualType::ANGULAR_ERROR: the residual of Create's estimates
struct RtAngular {
  __device__ inline double operator()(const RtView& w, uint32_t, const double* X, double max_residual, double* mg) const {
    if (!mg) return rt_residual(w, X);
    double d;
    const double r = rt_residual(w, X, &d);
    const double m = d <= kRtCosineEdge ? fabs(r - max_residual) / max_residual : 0.0;  // NaN or rounding to NaN
    if (m < mg[0]) mg[0] = m;
    return r;
  }
};

// HasPointPositiveDepth (projection.cc:199-203)
__device__ inline bool rt_depth(const RtView& w, const double* X, double* margin) {
  const double z = rt_row(w.P, 2, X);
  const double m = fabs(z - DBL_EPSILON) / fmax(fabs(z), DBL_EPSILON);
  if (m < *margin) *margin = m;
  return z >= DBL_EPSILON;
}

__device__ inline bool rt_angle_ok(double angle, double min_angle, double* margin) {
  const double m = fabs(angle - min_angle) / min_angle;
  if (m < *margin) *margin = m;
  return angle >= min_angle;
}

// the eigenvector of the smallest eigenvalue of a symmetric 4 x 4 matrix (cyclic Jacobi; SelfAdjointEigenSolver's col(0))
__device__ void rt_sym4_min_vec(double* A, double* x) {
  double V[16];
  for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 32; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < 4; ++p) {
      diag += A[5 * p] * A[5 * p];
      for (int q = p + 1; q < 4; ++q) off += A[4 * p + q] * A[4 * p + q];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[4 * p + q];
        if (apq == 0.0) continue;
        const double theta = (A[5 * q] - A[5 * p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < 4; ++k) {  // A <- A J (columns p, q)
          const double akp = A[4 * k + p], akq = A[4 * k + q];
          A[4 * k + p] = c * akp - s * akq;
          A[4 * k + q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {  // A <- J^T A (rows p, q)
          const double apk = A[4 * p + k], aqk = A[4 * q + k];
          A[4 * p + k] = c * apk - s * aqk;
          A[4 * q + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[4 * k + p], vkq = V[4 * k + q];
          V[4 * k + p] = c * vkp - s * vkq;
          V[4 * k + q] = s * vkp + c * vkq;
        }
      }
  }
  int m = 0;
  for (int i = 1; i < 4; ++i)
    if (A[5 * i] < A[5 * m]) m = i;
  x[0] = V[m] / V[12 + m];
  x[1] = V[4 + m] / V[12 + m];
  x[2] = V[8 + m] / V[12 + m];
}

// TriangulateMultiViewPoint (triangulation.cc:72-89) accumulated one view at a time
__device__ void rt_accumulate(const RtView& w, double* A) {
  const double n = sqrt((w.u * w.u + w.v * w.v) + 1.0);
  const double p[3] = {w.u / n, w.v / n, 1.0 / n};
  double T[12];
  for (int c = 0; c < 4; ++c) {
    const double pP = (p[0] * w.P[c] + p[1] * w.P[4 + c]) + p[2] * w.P[8 + c];
    for (int r = 0; r < 3; ++r) T[4 * r + c] = w.P[4 * r + c] - p[r] * pP;
  }
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) A[4 * i + j] += (T[i] * T[j] + T[4 + i] * T[4 + j]) + T[8 + i] * T[8 + j];
}

template <class Res>
struct RtLaneT {
  const uint32_t* feat_img;
  const double* img_P;
  const double* img_C;
  const double* uv;
  const int32_t* clist;  // this problem's create list (features)
  const int32_t* idx;    // the current level's entries (positions in clist)
  int n;
  RtParams prm;
  double mg[kRtMargins];
  Res res;
};
using RtLane = RtLaneT<RtAngular>;

template <class Res>
__device__ inline uint32_t rt_feature(const RtLaneT<Res>& L, int i) {
  return (uint32_t)L.clist[L.idx[i]];
}

template <class Res>
__device__ inline void rt_view(const RtLaneT<Res>& L, int i, RtView* w) {
  rt_load(rt_feature(L, i), L.feat_img, L.img_P, L.img_C, L.uv, w);
}

// support of X over the level's n entries: count and residual sum in entry order; residual margins recorded
template <class Res>
__device__ void rt_support(RtLaneT<Res>& L, const double* X, uint32_t* cnt, double* sum) {
  uint32_t c = 0;
  double s = 0.0;
  for (int i = 0; i < L.n; ++i) {
    RtView w;
    rt_view(L, i, &w);
    const double r = L.res(w, rt_feature(L, i), X, L.prm.max_residual, L.mg);
    if (r <= L.prm.max_residual) {
      ++c;
      s += r;
    }
  }
  *cnt = c;
  *sum = s;
}

template <class Res>
__device__ inline bool rt_better(RtLaneT<Res>& L, uint32_t c1, double s1, uint32_t c2, double s2) {
  if (c1 > c2) return true;
  if (c1 == c2 && c1 > 0 && s2 != DBL_MAX) {  // a tie of two models without an inlier cannot change the outcome
    const double m = fabs(s1 - s2) / fmax(fmax(s1, s2), DBL_MIN);
    if (m < L.mg[1]) L.mg[1] = m;
  }
  return c1 == c2 && s1 < s2;
}

// TriangulationEstimator::Estimate on the multi-view set of the level's entries whose residual of X0 is within max_residual;
// returns false when no model passes
template <class Res>
__device__ bool rt_estimate_multi(RtLaneT<Res>& L, const double* X0, double* X) {
  double A[16];
  for (int i = 0; i < 16; ++i) A[i] = 0.0;
  for (int i = 0; i < L.n; ++i) {
    RtView w;
    rt_view(L, i, &w);
    if (L.res(w, rt_feature(L, i), X0, L.prm.max_residual, nullptr) <= L.prm.max_residual) rt_accumulate(w, A);
  }
  rt_sym4_min_vec(A, X);
  for (int i = 0; i < L.n; ++i) {
    RtView w;
    rt_view(L, i, &w);
    if (L.res(w, rt_feature(L, i), X0, L.prm.max_residual, nullptr) <= L.prm.max_residual && !rt_depth(w, X, &L.mg[3])) return false;
  }
  for (int i = 0; i < L.n; ++i) {
    RtView wi;
    rt_view(L, i, &wi);
    if (!(L.res(wi, rt_feature(L, i), X0, L.prm.max_residual, nullptr) <= L.prm.max_residual)) continue;
    for (int j = 0; j < i; ++j) {
      RtView wj;
      rt_view(L, j, &wj);
      if (!(L.res(wj, rt_feature(L, j), X0, L.prm.max_residual, nullptr) <= L.prm.max_residual)) continue;
      if (rt_angle_ok(tri_angle_libm(wi.C, wj.C, X), L.prm.min_tri_angle, &L.mg[2])) return true;
    }
  }
  return false;
}

// LORANSAC over the level's n entries; returns success and the best model.  carried_min_trials: RANSACOptions::min_num_trials
// of a list above the exhaustive-sampling threshold (15), where the caller's options keep the value of an earlier estimate
// (CompleteImage); Create's options are fresh per call, so it passes 0.
template <class Res>
__device__ bool rt_loransac(RtLaneT<Res>& L, const uint32_t* tab, const uint32_t* tab_off, double* best_X, uint32_t* trials,
                            uint64_t carried_min_trials = 0) {
  const int n = L.n;
  const uint64_t all = (uint64_t)n * (n - 1) / 2;
  const uint64_t max_trials = all < (uint64_t)L.prm.max_trials ? all : (uint64_t)L.prm.max_trials;
  const uint64_t min_trials = n <= 15 ? all : carried_min_trials;
  uint32_t best_c = 0;
  double best_s = DBL_MAX;
  uint64_t dyn = max_trials;
  bool abort = false;
  int si = 0, sj = 1;  // CombinationSampler: lexicographic pairs (never wraps: max_trials <= C(n, 2))
  uint64_t t = 0;
  for (t = 0; t < max_trials; ++t) {
    if (abort) {
      t += 1;
      break;
    }
    const int a = si, b = sj;
    if (++sj == n) {
      ++si;
      sj = si + 1;
    }
    RtView wa, wb;
    rt_view(L, a, &wa);
    rt_view(L, b, &wb);
    double X[3];
    triangulate_two_view(wa.P, wb.P, wa.u, wa.v, wb.u, wb.v, X);
    const bool d0 = rt_depth(wa, X, &L.mg[3]);
    const bool ok = d0 && rt_depth(wb, X, &L.mg[3]) && rt_angle_ok(tri_angle_libm(wa.C, wb.C, X), L.prm.min_tri_angle, &L.mg[2]);
    if (!ok) continue;
    uint32_t c;
    double s;
    rt_support(L, X, &c, &s);
    if (rt_better(L, c, s, best_c, best_s)) {
      best_c = c;
      best_s = s;
      best_X[0] = X[0], best_X[1] = X[1], best_X[2] = X[2];
      if (c > 2) {
        double XL[3];
        if (rt_estimate_multi(L, X, XL)) {
          uint32_t lc;
          double ls;
          rt_support(L, XL, &lc, &ls);
          if (rt_better(L, lc, ls, best_c, best_s)) {
            best_c = lc;
            best_s = ls;
            best_X[0] = XL[0], best_X[1] = XL[1], best_X[2] = XL[2];
          }
        }
      }
      dyn = (n <= (int)L.prm.tab_n) ? tab[tab_off[n] + best_c] : max_trials;
    }
    if (t >= dyn && t >= min_trials) abort = true;
  }
  *trials += (uint32_t)t;
  return best_c >= 2;
}

// ComputeNumTrials (ransac.h:151-167) for every (n, inliers), clamped to 32 bits; ceil(-inf) (no inlier) -> never abort
inline uint32_t rt_num_trials(uint32_t k, uint32_t n, double confidence) {
  const double ratio = k / static_cast<double>(n);
  const double nom = 1 - confidence;
  if (nom <= 0) return UINT32_MAX;
  const double denom = 1 - std::pow(ratio, 2);
  if (denom <= 0) return 1;
  const double v = std::ceil(std::log(nom) / std::log(denom));
  if (!(v >= 0.0) || v >= 4294967295.0) return UINT32_MAX;
  return static_cast<uint32_t>(v);
}

}  // namespace

#endif  // DAGSFM_AMD_CSRC_RT_LORANSAC_H_
