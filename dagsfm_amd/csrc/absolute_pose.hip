// absolute_pose.hip -- batched absolute pose estimation: EstimateAbsolutePose (src/estimators/pose.cc:48-158),
// LORANSAC<P3PEstimator, EPNPEstimator> (src/optim/loransac.h:91-233, src/estimators/absolute_pose.cc:47-609) per focal-length
// factor, for a batch of independent problems.
//
// The unit of work is the RUN = (problem, focal-length factor).  Three kernels:
//   k_ap_prepare  a thread per (run, point): Camera::ImageToWorld with the run's scaled camera, SoA
//   k_ap_ransac   a one-wave workgroup per run, the whole LO-RANSAC of the run in trial order: lane 0 draws the sample and
//                 solves P3P, the 64 lanes score every model over the run's points (count by a wave reduction; the in-order
//                 residual sum only where Compare needs it: a count at or above the best one), EPnP with its O(N) parts as
//                 fixed-order tree sums over the wave and its fixed-size parts (3 x 3 / 12 x 12 Jacobi SVD, the 6 x k SVD solves,
//                 the pivoted 6 x 4 QR solves) serial on lane 0
//   k_ap_choose   a thread per problem: the choice among the factors in factor order, the quaternion, the record; then
//   k_ap_mask     the winning run's inlier mask to the problem's output rows
// Nothing is speculated: a run's trials are sequential, the batch supplies the parallelism (B x 31 runs with the focal sweep).
// DESIGN.md 14 says why this schedule was taken instead of the verification's speculate + replay, and what it costs.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "ctx.h"
#include "std_mt19937.h"
#include "verify_camera.h"
#include "verify_linalg.h"
#include "wave_reduce.h"

namespace {

constexpr int AP_MARGINS = DSM_ABSOLUTE_POSE_MARGINS;

struct ApRun {
  uint64_t poff;        // first point of the problem (points2D / points3D rows)
  uint64_t roff;        // first run-point (uv, sidx, mask, alphas rows)
  uint32_t N;
  uint32_t seed;
  uint32_t tab_off;     // ComputeNumTrials table of this N
  uint32_t problem;
  double max_residual;  // ImageToWorldThreshold(max_error)^2 of the scaled camera
  dsm_camera cam;       // the scaled camera
};

struct ApOut {
  uint32_t success, num_trials, num_inliers, is_local, num_models, num_lo;
  double model[12];
  double margins[AP_MARGINS];
};

struct ApParams {
  const ApRun* runs;
  uint32_t n_runs;
  const double* xy;     // [points][2] pixels
  const double* X;      // [points][3]
  double* un;           // [run-points] normalised x
  double* vn;           // [run-points] normalised y
  uint32_t* sidx;       // [run-points] RandomSampler's index array
  uint8_t* mask;        // [run-points] inliers of the run's current best model (EPnP's input), at the end the run's final mask
  double* alphas;       // [run-points][4]
  const uint32_t* tab;  // ComputeNumTrials(k, N, confidence), k = 0 .. N, per distinct N (host libm)
  uint32_t max_trials, min_trials;
  ApOut* out;
};

// ------------------------------------------------------------------------------------ std::mt19937 + libstdc++ uniform_int (lane 0)
// std_mt19937.h, the seeding and the draw out of line as this file's kernel was built with
__device__ __noinline__ void ap_mt_seed(StdMt19937* s, uint32_t seed) { std_mt19937_seed(s, seed); }
__device__ __noinline__ uint32_t ap_mt_next(StdMt19937* s) { return std_mt19937_next(s); }

struct ApShared {
  StdMt19937 gen;
  double models[4][12];  // P3P's models of the current trial, row-major 3 x 4
  int nm;
  int ok;
  double best[12], loc[12];
  double mg[AP_MARGINS];  // lane 0's margins (3 .. 8); 0 .. 2 are reduced from the lanes' registers
  // EPnP
  double cws[4][3], ccs[4][3], cinv[9], c0[3], pc0[3], pw0[3];
  double red[12];
  double MtM[144], U[144], V[144];
  double Rt[3][12];      // the three candidates (R | t), row-major 3 x 4
  double err[3];
};

__device__ inline void ap_min(double* m, double v) {
  if (v < *m) *m = v;  // NaN never lowers a margin
}

// ComputeSquaredReprojectionError (src/estimators/utils.cc:133-180) of one point; margins: the depth test, relative
__device__ inline double ap_residual(const double* P, double x0, double x1, double X0, double X1, double X2, double* depth_margin) {
  const double px_2 = P[8] * X0 + P[9] * X1 + P[10] * X2 + P[11];
  const double apz = fabs(px_2);
  ap_min(depth_margin, fabs(px_2 - DBL_EPSILON) / (apz > DBL_EPSILON ? apz : DBL_EPSILON));
  if (px_2 > DBL_EPSILON) {
    const double px_0 = P[0] * X0 + P[1] * X1 + P[2] * X2 + P[3];
    const double px_1 = P[4] * X0 + P[5] * X1 + P[6] * X2 + P[7];
    const double inv_px_2 = 1.0 / px_2;
    const double dx_0 = x0 - px_0 * inv_px_2;
    const double dx_1 = x1 - px_1 * inv_px_2;
    return dx_0 * dx_0 + dx_1 * dx_1;
  }
  return DBL_MAX;
}

struct ApView {  // a run's data as the lanes see it
  const double* un;
  const double* vn;
  const double* X;
  uint8_t* mask;
  double* alphas;
  int N;
  double thr;
};

// InlierSupportMeasurer's count of model P over the run's points (every lane returns it); mode 1 also writes the mask
__device__ __noinline__ int ap_count(const ApView& v, const double* P, int lane, int write_mask, double* mg_res, double* mg_depth) {
  double Pl[12];
  for (int i = 0; i < 12; ++i) Pl[i] = P[i];
  int cnt = 0;
  for (int i = lane; i < v.N; i += 64) {
    const double r = ap_residual(Pl, v.un[i], v.vn[i], v.X[3 * i], v.X[3 * i + 1], v.X[3 * i + 2], mg_depth);
    if (r != DBL_MAX) ap_min(mg_res, fabs(r - v.thr) / v.thr);
    const int in = r <= v.thr;
    cnt += in;
    if (write_mask) v.mask[i] = (uint8_t)in;
  }
  return wave_sum(cnt);
}
// ... and its residual sum, accumulated in point order like the reference's loop
__device__ __noinline__ double ap_sum(const ApView& v, const double* P, int lane) {
  double Pl[12];
  for (int i = 0; i < 12; ++i) Pl[i] = P[i];
  double dummy = INFINITY;
  return wv_seq_sum(0.0, v.N, lane, [&](int i) {
    const double r = ap_residual(Pl, v.un[i], v.vn[i], v.X[3 * i], v.X[3 * i + 1], v.X[3 * i + 2], &dummy);
    return r <= v.thr ? r : 0.0;
  });
}

// Eigen's 3 x 3 determinant (bruteforce_det3_helper order), row-major
__device__ inline double ap_det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[7] * m[5]) - m[3] * (m[1] * m[8] - m[7] * m[2]) + m[6] * (m[1] * m[5] - m[4] * m[2]);
}

__device__ __noinline__ void ap_svd3(const double* A_rowmajor, double* U, double* V, double* sv) {
  pl_jacobi_svd_square<3, true>(A_rowmajor, U, V, sv);
}

// Eigen::umeyama(world, camera, false) of three points (DESIGN.md 14 fixes the order inside): out = 3 x 4 row-major
__device__ __noinline__ void ap_umeyama3(const double (*src)[3], const double (*dst)[3], double* out) {
  const double third = 1.0 / 3.0;
  double ms[3], md[3], sig[9];
  for (int k = 0; k < 3; ++k) {
    ms[k] = ((src[0][k] + src[1][k]) + src[2][k]) * third;
    md[k] = ((dst[0][k] + dst[1][k]) + dst[2][k]) * third;
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j)
      sig[i * 3 + j] = ((third * (dst[0][i] - md[i])) * (src[0][j] - ms[j]) + (third * (dst[1][i] - md[i])) * (src[1][j] - ms[j])) +
                       (third * (dst[2][i] - md[i])) * (src[2][j] - ms[j]);
  double U[9], V[9], sv[3], Ur[9], Vr[9];
  ap_svd3(sig, U, V, sv);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      Ur[r * 3 + c] = U[c * 3 + r];
      Vr[r * 3 + c] = V[c * 3 + r];
    }
  double S[3] = {1.0, 1.0, 1.0};
  if (ap_det3(Ur) * ap_det3(Vr) < 0.0) S[2] = -1.0;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      out[i * 4 + j] = ((Ur[i * 3 + 0] * S[0]) * Vr[j * 3 + 0] + (Ur[i * 3 + 1] * S[1]) * Vr[j * 3 + 1]) + (Ur[i * 3 + 2] * S[2]) * Vr[j * 3 + 2];
    out[i * 4 + 3] = md[i] - ((out[i * 4 + 0] * ms[0] + out[i * 4 + 1] * ms[1]) + out[i * 4 + 2] * ms[2]);
  }
}

// P3PEstimator::Estimate (absolute_pose.cc:47-174) on lane 0: x = normalised 2D points, Xw = world points of the sample
__device__ __noinline__ int ap_p3p(const double (*x)[2], const double (*Xw)[3], double (*models)[12], double* mg) {
  double uvw[3][3];
  for (int k = 0; k < 3; ++k) {
    const double s = sqrt((x[k][0] * x[k][0] + x[k][1] * x[k][1]) + 1);
    uvw[k][0] = x[k][0] / s;
    uvw[k][1] = x[k][1] / s;
    uvw[k][2] = 1.0 / s;
  }
  const double* u = uvw[0];
  const double* v = uvw[1];
  const double* w = uvw[2];
  const double cos_uv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
  const double cos_uw = (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2];
  const double cos_vw = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
  auto d2 = [&](int i, int j) {
    const double a0 = Xw[i][0] - Xw[j][0], a1 = Xw[i][1] - Xw[j][1], a2 = Xw[i][2] - Xw[j][2];
    return (a0 * a0 + a1 * a1) + a2 * a2;
  };
  const double dist_AB_2 = d2(0, 1), dist_AC_2 = d2(0, 2), dist_BC_2 = d2(1, 2);
  const double dist_AB = sqrt(dist_AB_2);
  const double a = dist_BC_2 / dist_AB_2;
  const double b = dist_AC_2 / dist_AB_2;
  const double a2 = a * a;
  const double b2 = b * b;
  const double p = 2 * cos_vw;
  const double q = 2 * cos_uw;
  const double r = 2 * cos_uv;
  const double p2 = p * p;
  const double p3 = p2 * p;
  const double q2 = q * q;
  const double r2 = r * r;
  const double r3 = r2 * r;
  const double r4 = r3 * r;
  const double r5 = r4 * r;
  double coeffs[5];
  coeffs[0] = -2 * b + b2 + a2 + 1 + a * b * (2 - r2) - 2 * a;
  coeffs[1] = -2 * q * a2 - r * p * b2 + 4 * q * a + (2 * q + p * r) * b + (r2 * q - 2 * q + r * p) * a * b - 2 * q;
  coeffs[2] = (2 + q2) * a2 + (p2 + r2 - 2) * b2 - (4 + 2 * q2) * a - (p * q * r + p2) * b - (p * q * r + r2) * a * b + q2 + 2;
  coeffs[3] = -2 * q * a2 - r * p * b2 + 4 * q * a + (p * r + q * p2 - 2 * q) * b + (r * p + 2 * q) * a * b - 2 * q;
  coeffs[4] = a2 + b2 - 2 * a + (2 - p2) * b - 2 * a * b + 1;
  for (int i = 0; i < 5; ++i)
    if (!isfinite(coeffs[i])) return 0;  // a repeated world point: the reference's eigen-solver fails on the NaN matrix
  double re[5], im[5];
  const int nr = pl_poly_roots<5>(coeffs, 5, re, im);
  if (nr < 0) return 0;
  int nm = 0;
  for (int i = 0; i < nr; ++i) {
    ap_min(&mg[3], fabs(fabs(im[i]) - 1e-10) / 1e-10);
    if (fabs(im[i]) > 1e-10) continue;
    const double x_ = re[i];
    ap_min(&mg[4], fabs(x_));
    if (x_ < 0) continue;
    const double x2 = x_ * x_;
    const double x3 = x2 * x_;
    const double bb1 = (p2 - p * q * r + r2) * a + (p2 - r2) * b - p2 + p * q * r - r2;
    const double b1 = b * bb1 * bb1;
    const double b0 =
        ((1 - a - b) * x2 + (a - 1) * q * x_ - a + b + 1) *
        (r3 * (a2 + b2 - 2 * a - 2 * b + (2 - r2) * a * b + 1) * x3 +
         r2 * (p + p * a2 - 2 * r * q * a * b + 2 * r * q * b - 2 * r * q - 2 * p * a - 2 * p * b + p * r2 * b + 4 * r * q * a + q * r3 * a * b -
               2 * r * q * a2 + 2 * p * a * b + p * b2 - r2 * p * b2) *
             x2 +
         (r5 * (b2 - a * b) - r4 * p * q * b + r3 * (q2 - 4 * a - 2 * q2 * a + q2 * a2 + 2 * a2 - 2 * b2 + 2) +
          r2 * (4 * p * q * a - 2 * p * q * a * b + 2 * p * q * b - 2 * p * q - 2 * p * q * a2) +
          r * (p2 * b2 - 2 * p2 * b + 2 * p2 * a * b - 2 * p2 * a + p2 + p2 * a2)) *
             x_ +
         (2 * p * r2 - 2 * r3 * q + p3 - 2 * p2 * q * r + p * q2 * r2) * a2 + (p3 - 2 * p * r2) * b2 +
         (4 * q * r3 - 4 * p * r2 - 2 * p3 + 4 * p2 * q * r - 2 * p * q2 * r2) * a + (-2 * q * r3 + p * r4 + 2 * p2 * q * r - 2 * p3) * b +
         (2 * p3 + 2 * q * r3 - 2 * p2 * q * r) * a * b + p * q2 * r2 - 2 * p2 * q * r + 2 * p * r2 + p3 - 2 * r3 * q);
    const double y = b0 / b1;
    const double y2 = y * y;
    const double nu = x2 + y2 - 2 * x_ * y * cos_uv;
    const double dist_PC = dist_AB / sqrt(nu);
    const double dist_PB = y * dist_PC;
    const double dist_PA = x_ * dist_PC;
    double cam[3][3];
    for (int k = 0; k < 3; ++k) {
      cam[0][k] = u[k] * dist_PA;
      cam[1][k] = v[k] * dist_PB;
      cam[2][k] = w[k] * dist_PC;
    }
    ap_umeyama3(Xw, cam, models[nm]);
    ++nm;
  }
  return nm;
}

// ColPivHouseholderQR::computeInPlace with the permutation (rows x cols, rows >= cols <= 5, column-major): pl_colpiv_qr's
// operations plus perm[k] = the original column now at k and *nzp = nonzeroPivots()
__device__ __noinline__ void ap_colpiv_qr(double* qr, int rows, int cols, double* hco, int* perm, int* nzp) {
  double nu[5], nd[5];
  for (int k = 0; k < cols; ++k) {
    double s = 0.0;
    for (int i = 0; i < rows; ++i) s += qr[k * rows + i] * qr[k * rows + i];
    nd[k] = nu[k] = sqrt(s);
    perm[k] = k;
  }
  double maxn = 0.0;
  for (int k = 0; k < cols; ++k) maxn = nu[k] > maxn ? nu[k] : maxn;
  const double thr_helper = (maxn * DBL_EPSILON) * (maxn * DBL_EPSILON) / (double)rows;
  const double downdate = sqrt(DBL_EPSILON);
  *nzp = cols;
  for (int k = 0; k < cols; ++k) {
    int big = k;
    double mx = nu[k];
    for (int j = k + 1; j < cols; ++j)
      if (nu[j] > mx) {
        mx = nu[j];
        big = j;
      }
    if (*nzp == cols && mx * mx < thr_helper * (double)(rows - k)) *nzp = k;
    if (k != big) {
      for (int i = 0; i < rows; ++i) {
        const double t = qr[k * rows + i];
        qr[k * rows + i] = qr[big * rows + i];
        qr[big * rows + i] = t;
      }
      double t = nu[k];
      nu[k] = nu[big];
      nu[big] = t;
      t = nd[k];
      nd[k] = nd[big];
      nd[big] = t;
      const int ti = perm[k];
      perm[k] = perm[big];
      perm[big] = ti;
    }
    double tau, beta;
    pl_make_householder<1>(qr + k * rows + k, rows - k, &tau, &beta);
    hco[k] = tau;
    qr[k * rows + k] = beta;
    pl_apply_householder_left<1, 1>(qr, rows, k, k + 1, rows - k, cols - k - 1, qr + k * rows + k + 1, tau);
    for (int j = k + 1; j < cols; ++j) {
      if (nu[j] != 0.0) {
        double temp = fabs(qr[j * rows + k]) / nu[j];
        temp = (1.0 + temp) * (1.0 - temp);
        temp = temp < 0.0 ? 0.0 : temp;
        const double ratio = nu[j] / nd[j];
        const double temp2 = temp * (ratio * ratio);
        if (temp2 <= downdate) {
          double s = 0.0;
          for (int i = k + 1; i < rows; ++i) s += qr[j * rows + i] * qr[j * rows + i];
          nd[j] = nu[j] = sqrt(s);
        } else {
          nu[j] *= sqrt(temp);
        }
      }
    }
  }
}
// c = Q^T b: the reflectors applied in order
__device__ __noinline__ void ap_apply_qt(const double* qr, int rows, int cols, const double* hco, double* c) {
  for (int k = 0; k < cols; ++k) {
    const int nr = rows - k;
    const double tau = hco[k];
    if (nr == 1) {
      c[k] *= (1.0 - tau);
    } else if (tau != 0.0) {
      double tmp = 0.0;
      for (int i = 1; i < nr; ++i) tmp += qr[k * rows + k + i] * c[k + i];
      tmp += c[k];
      c[k] -= tau * tmp;
      for (int i = 1; i < nr; ++i) c[k + i] -= tau * qr[k * rows + k + i] * tmp;
    }
  }
}

// A.colPivHouseholderQr().solve(b) for the 6 x 4 Gauss-Newton system (A column-major, destroyed)
__device__ __noinline__ void ap_qr_solve64(double* A, const double* b, double* x) {
  double hco[4], c[6];
  int perm[4], nzp;
  ap_colpiv_qr(A, 6, 4, hco, perm, &nzp);
  for (int i = 0; i < 6; ++i) c[i] = b[i];
  ap_apply_qt(A, 6, 4, hco, c);
  for (int i = nzp - 1; i >= 0; --i) {  // back substitution on the leading nzp x nzp triangle
    double s = c[i];
    for (int j = i + 1; j < nzp; ++j) s -= A[j * 6 + i] * c[j];
    c[i] = s / A[i * 6 + i];
  }
  for (int i = 0; i < 4; ++i) x[i] = 0.0;
  for (int i = 0; i < nzp; ++i) x[perm[i]] = c[i];
}

// JacobiSVD<6 x K>(A).solve(b): the pivoted QR preconditioner of A / max|A|, the Jacobi sweeps on its K x K triangle, then
// V_r diag(1 / s) U_r^T (Q^T b) over the numerical rank
template <int K>
__device__ __noinline__ void ap_svd_solve6(const double* A_colmajor, const double* b, double* x) {
  double qr[6 * K], hco[K], c[6];
  int perm[K], nzp;
  double scale = 0.0;
  for (int i = 0; i < 6 * K; ++i) scale = fabs(A_colmajor[i]) > scale ? fabs(A_colmajor[i]) : scale;
  if (scale == 0.0) scale = 1.0;
  for (int i = 0; i < 6 * K; ++i) qr[i] = A_colmajor[i] / scale;
  ap_colpiv_qr(qr, 6, K, hco, perm, &nzp);
  double R[K * K], U[K * K], V[K * K], sv[K];
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j) R[i * K + j] = j >= i ? qr[j * 6 + i] : 0.0;  // row-major
  if constexpr (K == 3)
    ap_svd3(R, U, V, sv);
  else
    pl_jacobi_svd_square<K, true>(R, U, V, sv);
  for (int i = 0; i < 6; ++i) c[i] = b[i];
  ap_apply_qt(qr, 6, K, hco, c);
  const double t0 = sv[0] * ((double)K * DBL_EPSILON);
  const double thr = t0 > DBL_MIN ? t0 : DBL_MIN;
  int rank = K;
  while (rank > 0 && sv[rank - 1] < thr) --rank;
  double tmp[K];
  for (int j = 0; j < rank; ++j) {
    double s = 0.0;
    for (int i = 0; i < K; ++i) s += U[j * K + i] * c[i];
    tmp[j] = (1.0 / (sv[j] * scale)) * s;
  }
  for (int i = 0; i < K; ++i) {
    double s = 0.0;
    for (int j = 0; j < rank; ++j) s += V[j * K + i] * tmp[j];
    x[perm[i]] = s;
  }
}

__device__ __noinline__ void ap_svd12(const double* A, double* U, double* V, double* sv) { pl_jacobi_svd_square<12, true>(A, U, V, sv); }

__device__ __noinline__ void ap_gauss_newton(const double (*L)[10], const double* rho, double* be) {
  for (int it = 0; it < 5; ++it) {
    double A[24], bb[6], x[4];
    for (int i = 0; i < 6; ++i) {
      A[0 * 6 + i] = 2 * L[i][0] * be[0] + L[i][1] * be[1] + L[i][3] * be[2] + L[i][6] * be[3];
      A[1 * 6 + i] = L[i][1] * be[0] + 2 * L[i][2] * be[1] + L[i][4] * be[2] + L[i][7] * be[3];
      A[2 * 6 + i] = L[i][3] * be[0] + L[i][4] * be[1] + 2 * L[i][5] * be[2] + L[i][8] * be[3];
      A[3 * 6 + i] = L[i][6] * be[0] + L[i][7] * be[1] + L[i][8] * be[2] + 2 * L[i][9] * be[3];
      bb[i] = rho[i] - (L[i][0] * be[0] * be[0] + L[i][1] * be[0] * be[1] + L[i][2] * be[1] * be[1] + L[i][3] * be[0] * be[2] +
                        L[i][4] * be[1] * be[2] + L[i][5] * be[2] * be[2] + L[i][6] * be[0] * be[3] + L[i][7] * be[1] * be[3] +
                        L[i][8] * be[2] * be[3] + L[i][9] * be[3] * be[3]);
    }
    ap_qr_solve64(A, bb, x);
    for (int i = 0; i < 4; ++i) be[i] += x[i];
  }
}

__device__ inline void ap_sign_margin(double* mg, const double* b, int n, int which) {
  double mx = 0.0;
  for (int i = 0; i < n; ++i) mx = fabs(b[i]) > mx ? fabs(b[i]) : mx;
  if (mx > 0.0) ap_min(&mg[6], fabs(b[which]) / mx);
}

// lane 0, between the two wave phases of EPnP: SVD of MtM, L6x10, rho, the three beta vectors (sm->red[0 .. 11] = betas)
__device__ __noinline__ void ap_epnp_betas(ApShared* sm, double (*betas)[4]) {
  double sv[12];
  ap_svd12(sm->MtM, sm->U, sm->V, sv);
  const double* U = sm->U;  // column-major: Ut(r, c) = U[r * 12 + c]
  double L[6][10], rho[6];
  {
    double dv[4][6][3];
    for (int i = 0; i < 4; ++i) {
      int a = 0, b = 1;
      for (int j = 0; j < 6; ++j) {
        for (int k = 0; k < 3; ++k) dv[i][j][k] = U[(11 - i) * 12 + 3 * a + k] - U[(11 - i) * 12 + 3 * b + k];
        b += 1;
        if (b > 3) {
          a += 1;
          b = a + 1;
        }
      }
    }
    auto dot = [&](int p, int q, int i) { return (dv[p][i][0] * dv[q][i][0] + dv[p][i][1] * dv[q][i][1]) + dv[p][i][2] * dv[q][i][2]; };
    for (int i = 0; i < 6; ++i) {
      L[i][0] = dot(0, 0, i);
      L[i][1] = 2.0 * dot(0, 1, i);
      L[i][2] = dot(1, 1, i);
      L[i][3] = 2.0 * dot(0, 2, i);
      L[i][4] = 2.0 * dot(1, 2, i);
      L[i][5] = dot(2, 2, i);
      L[i][6] = 2.0 * dot(0, 3, i);
      L[i][7] = 2.0 * dot(1, 3, i);
      L[i][8] = 2.0 * dot(2, 3, i);
      L[i][9] = dot(3, 3, i);
    }
    int k = 0;
    for (int a = 0; a < 4; ++a)
      for (int b = a + 1; b < 4; ++b) {
        const double d0 = sm->cws[a][0] - sm->cws[b][0], d1 = sm->cws[a][1] - sm->cws[b][1], d2 = sm->cws[a][2] - sm->cws[b][2];
        rho[k++] = (d0 * d0 + d1 * d1) + d2 * d2;
      }
  }
  double A[30];
  {  // FindBetasApprox1: columns 0, 1, 3, 6
    const int cols[4] = {0, 1, 3, 6};
    double b4[4];
    for (int c = 0; c < 4; ++c)
      for (int i = 0; i < 6; ++i) A[c * 6 + i] = L[i][cols[c]];
    ap_svd_solve6<4>(A, rho, b4);
    ap_sign_margin(sm->mg, b4, 4, 0);
    double* be = betas[0];
    if (b4[0] < 0) {
      be[0] = sqrt(-b4[0]);
      be[1] = -b4[1] / be[0];
      be[2] = -b4[2] / be[0];
      be[3] = -b4[3] / be[0];
    } else {
      be[0] = sqrt(b4[0]);
      be[1] = b4[1] / be[0];
      be[2] = b4[2] / be[0];
      be[3] = b4[3] / be[0];
    }
    ap_gauss_newton(L, rho, be);
  }
  {  // FindBetasApprox2: columns 0, 1, 2
    double b3[3];
    for (int c = 0; c < 3; ++c)
      for (int i = 0; i < 6; ++i) A[c * 6 + i] = L[i][c];
    ap_svd_solve6<3>(A, rho, b3);
    for (int w = 0; w < 3; ++w) ap_sign_margin(sm->mg, b3, 3, w);
    double* be = betas[1];
    if (b3[0] < 0) {
      be[0] = sqrt(-b3[0]);
      be[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
      be[0] = sqrt(b3[0]);
      be[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) be[0] = -be[0];
    be[2] = 0.0;
    be[3] = 0.0;
    ap_gauss_newton(L, rho, be);
  }
  {  // FindBetasApprox3: columns 0 .. 4
    double b5[5];
    for (int c = 0; c < 5; ++c)
      for (int i = 0; i < 6; ++i) A[c * 6 + i] = L[i][c];
    ap_svd_solve6<5>(A, rho, b5);
    for (int w = 0; w < 3; ++w) ap_sign_margin(sm->mg, b5, 5, w);
    double* be = betas[2];
    if (b5[0] < 0) {
      be[0] = sqrt(-b5[0]);
      be[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
      be[0] = sqrt(b5[0]);
      be[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) be[0] = -be[0];
    be[2] = b5[3] / be[0];
    be[3] = 0.0;
    ap_gauss_newton(L, rho, be);
  }
}

// sum over the run's points in a FIXED order: lane l accumulates the terms of points l, l + 64, ... in
// order, the 64 partial sums are combined by the xor butterfly 32, 16, ..., 1; a point outside the input set adds +0.0
template <int NC, typename F>
__device__ inline void ap_tree_sums(const ApView& v, int lane, double* out, F term) {
  double acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) acc[c] = 0.0;
  for (int i = lane; i < v.N; i += 64) {
    const bool in = v.mask[i] != 0;
    double t[NC];
    term(i, t);
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] += in ? t[c] : 0.0;
  }
  wave_sum(acc);
#pragma unroll
  for (int c = 0; c < NC; ++c) out[c] = acc[c];
}

// EPNPEstimator::ComputePose (absolute_pose.cc:204-609) on the points with mask != 0 (n of them); every lane returns
// whether a model was written to sm->loc.  All 64 lanes call it.
__device__ __noinline__ bool ap_epnp(const ApView& v, int n, ApShared* sm, int lane, double* mg_depth) {
  const double dn = (double)n;
  double r3[3], r6[6], r12[12];
  // ChooseControlPoints
  ap_tree_sums<3>(v, lane, r3, [&](int i, double* t) {
    for (int k = 0; k < 3; ++k) t[k] = v.X[3 * i + k];
  });
  const double c0[3] = {r3[0] / dn, r3[1] / dn, r3[2] / dn};
  ap_tree_sums<6>(v, lane, r6, [&](int i, double* t) {
    const double d0 = v.X[3 * i] - c0[0], d1 = v.X[3 * i + 1] - c0[1], d2 = v.X[3 * i + 2] - c0[2];
    t[0] = d0 * d0;
    t[1] = d0 * d1;
    t[2] = d0 * d2;
    t[3] = d1 * d1;
    t[4] = d1 * d2;
    t[5] = d2 * d2;
  });
  // first inlier (pcs_[0] of SolveForSign)
  int first = v.N;
  for (int i = lane; i < v.N; i += 64)
    if (v.mask[i]) {
      first = i;
      break;
    }
  first = wave_min(first);
  if (lane == 0) {
    const double A[9] = {r6[0], r6[1], r6[2], r6[1], r6[3], r6[4], r6[2], r6[4], r6[5]};
    double U[9], V[9], D[3];
    ap_svd3(A, U, V, D);
    for (int k = 0; k < 3; ++k) sm->cws[0][k] = c0[k];
    for (int i = 1; i < 4; ++i) {
      const double kk = sqrt(D[i - 1] / dn);
      for (int k = 0; k < 3; ++k) sm->cws[i][k] = c0[k] + kk * U[(i - 1) * 3 + k];
    }
    // ComputeBarycentricCoordinates: the rank of CC by pivoted QR, then its inverse
    double CC[9], qr[9], hco[3];
    int perm[3], nzp;
    for (int i = 0; i < 3; ++i)
      for (int j = 1; j < 4; ++j) {
        CC[i * 3 + (j - 1)] = sm->cws[j][i] - sm->cws[0][i];
        qr[(j - 1) * 3 + i] = CC[i * 3 + (j - 1)];
      }
    ap_colpiv_qr(qr, 3, 3, hco, perm, &nzp);
    double maxpiv = 0.0;
    for (int i = 0; i < 3; ++i) maxpiv = fabs(qr[i * 3 + i]) > maxpiv ? fabs(qr[i * 3 + i]) : maxpiv;
    const double thr = maxpiv * (3.0 * DBL_EPSILON);
    int rank = 0;
    for (int i = 0; i < nzp; ++i) {
      const double piv = fabs(qr[i * 3 + i]);
      rank += piv > thr;
      if (thr > 0.0) ap_min(&sm->mg[5], fabs(piv - thr) / thr);
    }
    sm->ok = rank >= 3;
    if (sm->ok) m3_inverse(CC, sm->cinv);
  }
  __syncthreads();
  if (!sm->ok) return false;
  // alphas
  for (int i = lane; i < v.N; i += 64) {
    if (!v.mask[i]) continue;
    const double d0 = v.X[3 * i] - sm->cws[0][0], d1 = v.X[3 * i + 1] - sm->cws[0][1], d2 = v.X[3 * i + 2] - sm->cws[0][2];
    double al[4];
    for (int j = 0; j < 3; ++j) al[1 + j] = (sm->cinv[j * 3 + 0] * d0 + sm->cinv[j * 3 + 1] * d1) + sm->cinv[j * 3 + 2] * d2;
    al[0] = 1.0 - al[1] - al[2] - al[3];
    for (int j = 0; j < 4; ++j) v.alphas[4 * i + j] = al[j];
  }
  // MtM(a, b) = sum over the points of M(2i, a) M(2i, b) + M(2i + 1, a) M(2i + 1, b), row a at a time
  for (int a = 0; a < 12; ++a) {
    ap_tree_sums<12>(v, lane, r12, [&](int i, double* t) {
      const double x = v.un[i], y = v.vn[i];
      const double aa = v.alphas[4 * i + a / 3];
      const int ca = a % 3;
      const double m0a = ca == 0 ? aa : (ca == 1 ? 0.0 : -aa * x);
      const double m1a = ca == 0 ? 0.0 : (ca == 1 ? aa : -aa * y);
#pragma unroll
      for (int b = 0; b < 12; ++b) {
        const double ab = v.alphas[4 * i + b / 3];
        const int cb = b % 3;
        const double m0b = cb == 0 ? ab : (cb == 1 ? 0.0 : -ab * x);
        const double m1b = cb == 0 ? 0.0 : (cb == 1 ? ab : -ab * y);
        t[b] = m0a * m0b + m1a * m1b;
      }
    });
    if (lane == 0)
      for (int b = 0; b < 12; ++b) sm->MtM[a * 12 + b] = r12[b];
  }
  __syncthreads();
  double (*betas)[4] = reinterpret_cast<double (*)[4]>(sm->red);
  if (lane == 0) ap_epnp_betas(sm, betas);
  __syncthreads();
  // ComputeRT for the three beta vectors
  for (int cnd = 0; cnd < 3; ++cnd) {
    if (lane == 0) {
      for (int j = 0; j < 4; ++j)
        for (int k = 0; k < 3; ++k) {
          double s = 0.0;
          for (int i = 0; i < 4; ++i) s += betas[cnd][i] * sm->U[(11 - i) * 12 + 3 * j + k];
          sm->ccs[j][k] = s;
        }
      // SolveForSign as the reference has it: negate whenever the first point's depth is non-zero
      const double* al = &v.alphas[4 * first];
      const double z = ((al[0] * sm->ccs[0][2] + al[1] * sm->ccs[1][2]) + al[2] * sm->ccs[2][2]) + al[3] * sm->ccs[3][2];
      if (z < 0.0 || z > 0.0)
        for (int j = 0; j < 4; ++j)
          for (int k = 0; k < 3; ++k) sm->ccs[j][k] = -sm->ccs[j][k];
    }
    __syncthreads();
    auto pcs = [&](int i, double* pc) {
      const double* al = &v.alphas[4 * i];
      for (int k = 0; k < 3; ++k) pc[k] = ((al[0] * sm->ccs[0][k] + al[1] * sm->ccs[1][k]) + al[2] * sm->ccs[2][k]) + al[3] * sm->ccs[3][k];
    };
    ap_tree_sums<6>(v, lane, r6, [&](int i, double* t) {
      pcs(i, t);
      for (int k = 0; k < 3; ++k) t[3 + k] = v.X[3 * i + k];
    });
    double pc0[3], pw0[3], r9[9];
    for (int k = 0; k < 3; ++k) {
      pc0[k] = r6[k] / dn;
      pw0[k] = r6[3 + k] / dn;
    }
    ap_tree_sums<9>(v, lane, r9, [&](int i, double* t) {
      double pc[3];
      pcs(i, pc);
      for (int j = 0; j < 3; ++j)
        for (int c = 0; c < 3; ++c) t[j * 3 + c] = (pc[j] - pc0[j]) * (v.X[3 * i + c] - pw0[c]);
    });
    if (lane == 0) {
      double U[9], V[9], sv[3], R[9];
      ap_svd3(r9, U, V, sv);
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = (U[0 * 3 + i] * V[0 * 3 + j] + U[1 * 3 + i] * V[1 * 3 + j]) + U[2 * 3 + i] * V[2 * 3 + j];
      const double det = ap_det3(R);
      ap_min(&sm->mg[8], fabs(det));
      if (det < 0)
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) R[i * 3 + j] = (U[0 * 3 + i] * V[0 * 3 + j] + U[1 * 3 + i] * V[1 * 3 + j]) + U[2 * 3 + i] * (-V[2 * 3 + j]);
      double* P = sm->Rt[cnd];
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) P[i * 4 + j] = R[i * 3 + j];
        P[i * 4 + 3] = pc0[i] - ((R[i * 3 + 0] * pw0[0] + R[i * 3 + 1] * pw0[1]) + R[i * 3 + 2] * pw0[2]);
      }
    }
    __syncthreads();
    double e1[1], Pl[12];
    for (int i = 0; i < 12; ++i) Pl[i] = sm->Rt[cnd][i];
    ap_tree_sums<1>(v, lane, e1, [&](int i, double* t) {
      double dm = INFINITY;
      t[0] = sqrt(ap_residual(Pl, v.un[i], v.vn[i], v.X[3 * i], v.X[3 * i + 1], v.X[3 * i + 2], &dm));
      if (v.mask[i]) ap_min(mg_depth, dm);
    });
    if (lane == 0) sm->err[cnd] = e1[0];
    __syncthreads();
  }
  if (lane == 0) {
    int bi = 0;
    // the margin skips what rounding cannot flip: equal errors saturated by points behind the camera, and two candidates
    // that are one model up to rounding (closer than 1e-10, max-abs, relative) -- DESIGN.md 14
    auto cmp = [&](int i, int j) {
      const double x = sm->err[i], y = sm->err[j];
      if (x == y && x >= 1e150) return;
      double dmax = 0.0, amax = 0.0;
      for (int k = 0; k < 12; ++k) {
        dmax = fmax(dmax, fabs(sm->Rt[i][k] - sm->Rt[j][k]));
        amax = fmax(amax, fabs(sm->Rt[j][k]));
      }
      if (dmax <= 1e-10 * amax) return;
      const double mx = fabs(x) > fabs(y) ? fabs(x) : fabs(y);
      if (mx > 0.0) ap_min(&sm->mg[7], fabs(x - y) / mx);
    };
    cmp(1, 0);
    if (sm->err[1] < sm->err[0]) bi = 1;
    cmp(2, bi);
    if (sm->err[2] < sm->err[bi]) bi = 2;
    for (int i = 0; i < 12; ++i) sm->loc[i] = sm->Rt[bi][i];
  }
  __syncthreads();
  return true;
}

__global__ void __launch_bounds__(256) k_ap_prepare(ApParams p) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  for (uint32_t r = blockIdx.y; r < p.n_runs; r += gridDim.y) {
    const ApRun& run = p.runs[r];
    if (i >= run.N) continue;
    double u, v;
    image_to_world(run.cam, p.xy[2 * (run.poff + i)], p.xy[2 * (run.poff + i) + 1], &u, &v);
    p.un[run.roff + i] = u;
    p.vn[run.roff + i] = v;
    p.sidx[run.roff + i] = i;
    p.mask[run.roff + i] = 0;
  }
}

// LORANSAC<P3PEstimator, EPNPEstimator>::Estimate (loransac.h:91-233) of one run per one-wave workgroup
__global__ void __launch_bounds__(64) k_ap_ransac(ApParams p) {
  __shared__ ApShared sm;
  const int lane = threadIdx.x;
  const uint32_t r = blockIdx.x;
  const ApRun run = p.runs[r];
  ApOut* out = &p.out[r];
  ApView v;
  v.un = p.un + run.roff;
  v.vn = p.vn + run.roff;
  v.X = p.X + 3 * run.poff;
  v.mask = p.mask + run.roff;
  v.alphas = p.alphas + 4 * run.roff;
  v.N = (int)run.N;
  v.thr = run.max_residual;
  uint32_t* sidx = p.sidx + run.roff;
  const uint32_t* tab = p.tab + run.tab_off;
  double mg_res = INFINITY, mg_depth = INFINITY, mg_tie = INFINITY;
  if (lane == 0) {
    for (int i = 0; i < AP_MARGINS; ++i) sm.mg[i] = INFINITY;
    ap_mt_seed(&sm.gen, run.seed);
  }
  uint32_t nt = 0, nmodels = 0, nlo = 0;
  int best_cnt = 0, is_local = 0;
  double best_sum = DBL_MAX;
  if (v.N >= 3) {
    bool abort = false;
    uint32_t dyn = p.max_trials;
    for (nt = 0; nt < p.max_trials; ++nt) {
      if (abort) {
        nt += 1;
        break;
      }
      if (lane == 0) {
        double x[3][2], Xw[3][3];
        for (uint32_t i = 0; i < 3; ++i) {  // RandomSampler::Sample: a partial Fisher-Yates shuffle of the persistent index array
          const uint32_t j = std_uniform_u32([] { return ap_mt_next(&sm.gen); }, i, run.N - 1);
          const uint32_t t = sidx[i];
          sidx[i] = sidx[j];
          sidx[j] = t;
        }
        for (int i = 0; i < 3; ++i) {
          const uint32_t s = sidx[i];
          x[i][0] = v.un[s];
          x[i][1] = v.vn[s];
          for (int k = 0; k < 3; ++k) Xw[i][k] = v.X[3 * s + k];
        }
        sm.nm = ap_p3p(x, Xw, sm.models, sm.mg);
      }
      __syncthreads();
      const int nm = sm.nm;
      for (int m = 0; m < nm; ++m) {
        ++nmodels;
        const int cnt = ap_count(v, sm.models[m], lane, 0, &mg_res, &mg_depth);
        bool better = cnt > best_cnt;
        double sum = 0.0;
        if (cnt >= best_cnt) {  // Compare needs the residual sum: on a tie now, or on a later tie with this model as the best one
          sum = ap_sum(v, sm.models[m], lane);
          if (cnt == best_cnt) {
            const double mx = fabs(sum) > fabs(best_sum) ? fabs(sum) : fabs(best_sum);
            if (best_sum != DBL_MAX && mx > 0.0) ap_min(&mg_tie, fabs(sum - best_sum) / mx);
            better = sum < best_sum;
          }
        }
        if (better) {
          best_cnt = cnt;
          best_sum = sum;
          is_local = 0;
          if (lane == 0)
            for (int i = 0; i < 12; ++i) sm.best[i] = sm.models[m][i];
          if (cnt > 3 && cnt >= 4) {
            ++nlo;
            double d0 = INFINITY, d1 = INFINITY;
            (void)ap_count(v, sm.models[m], lane, 1, &d0, &d1);  // the inliers of the new best model: EPnP's input
            __syncthreads();
            if (ap_epnp(v, cnt, &sm, lane, &mg_depth)) {
              ++nmodels;
              const int lcnt = ap_count(v, sm.loc, lane, 0, &mg_res, &mg_depth);
              bool lbetter = lcnt > best_cnt;
              if (lcnt >= best_cnt) {
                const double lsum = ap_sum(v, sm.loc, lane);
                if (lcnt == best_cnt) {
                  const double mx = fabs(lsum) > fabs(best_sum) ? fabs(lsum) : fabs(best_sum);
                  if (mx > 0.0) ap_min(&mg_tie, fabs(lsum - best_sum) / mx);
                  lbetter = lsum < best_sum;
                }
                if (lbetter) {
                  best_cnt = lcnt;
                  best_sum = lsum;
                  is_local = 1;
                  if (lane == 0)
                    for (int i = 0; i < 12; ++i) sm.best[i] = sm.loc[i];
                }
              }
            }
          }
          dyn = tab[best_cnt];
        }
        if (nt >= dyn && nt >= p.min_trials) {
          abort = true;
          break;
        }
      }
      __syncthreads();
    }
  }
  __syncthreads();
  const bool success = best_cnt >= 3;
  if (success) {
    double d0 = INFINITY, d1 = INFINITY;
    (void)ap_count(v, sm.best, lane, 1, &d0, &d1);  // the final mask from the best model's residuals
  }
  mg_res = wave_fmin(mg_res);
  mg_depth = wave_fmin(mg_depth);
  if (lane == 0) {
    out->success = success;
    out->num_trials = nt;
    out->num_inliers = (uint32_t)best_cnt;
    out->is_local = is_local;
    out->num_models = nmodels;
    out->num_lo = nlo;
    for (int i = 0; i < 12; ++i) out->model[i] = best_cnt > 0 ? sm.best[i] : 0.0;
    out->margins[0] = mg_res;
    out->margins[1] = mg_depth;
    out->margins[2] = mg_tie;
    for (int i = 3; i < AP_MARGINS; ++i) out->margins[i] = sm.mg[i];
  }
}

// Quaterniond(R) -> (w, x, y, z), Eigen/src/Geometry/Quaternion.h (RotationMatrixToQuaternion, src/base/pose.cc:70-73); R(r, c) = P[4 r + c]
__device__ __noinline__ void ap_quaternion(const double* P, double* q) {
  auto R = [&](int r, int c) { return P[4 * r + c]; };
  double t = R(0, 0) + R(1, 1) + R(2, 2);
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R(2, 1) - R(1, 2)) * t;
    q[2] = (R(0, 2) - R(2, 0)) * t;
    q[3] = (R(1, 0) - R(0, 1)) * t;
  } else {
    int i = 0;
    if (R(1, 1) > R(0, 0)) i = 1;
    if (R(2, 2) > R(i, i)) i = 2;
    const int j = (i + 1) % 3;
    const int k = (j + 1) % 3;
    t = sqrt(R(i, i) - R(j, j) - R(k, k) + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R(k, j) - R(j, k)) * t;
    q[1 + j] = (R(j, i) + R(i, j)) * t;
    q[1 + k] = (R(k, i) + R(i, k)) * t;
  }
}

// EstimateAbsolutePose's choice among the factors (pose.cc:120-157), a thread per problem
__global__ void k_ap_choose(uint32_t B, const uint32_t* run0, const ApOut* outs, const double* factors, const dsm_camera* cams,
                            const uint8_t* flags, dsm_absolute_pose_result* res, int32_t* win_run, double* margins) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  dsm_absolute_pose_result o;
  o.success = 0;
  o.factor_index = -1;
  o.num_inliers = 0;
  o.num_trials = 0;
  o.model_is_local = 0;
  o.reserved = 0;
  o.focal_length_factor = 0.0;
  for (int i = 0; i < 12; ++i) o.proj_matrix[i] = 0.0;
  for (int i = 0; i < 4; ++i) o.qvec[i] = 0.0;
  for (int i = 0; i < 3; ++i) o.tvec[i] = 0.0;
  int32_t win = -1;
  double mg[AP_MARGINS];
  for (int i = 0; i < AP_MARGINS; ++i) mg[i] = INFINITY;
  for (uint32_t r = run0[b]; r < run0[b + 1]; ++r) {
    const ApOut& q = outs[r];
    for (int i = 0; i < AP_MARGINS; ++i) mg[i] = fmin(mg[i], q.margins[i]);
    if (q.success && q.num_inliers > o.num_inliers) {
      o.num_inliers = q.num_inliers;
      win = (int32_t)r;
    }
  }
  const dsm_camera& cam = cams[b];
  const bool two = cam_two_focal(cam.model_id);
  o.focal_params[0] = cam.params[0];
  o.focal_params[1] = two ? cam.params[1] : cam.params[0];
  if (win >= 0) {
    const ApOut& q = outs[win];
    o.factor_index = win - (int32_t)run0[b];
    o.focal_length_factor = flags[b] ? factors[o.factor_index] : 1.0;
    o.num_trials = q.num_trials;
    o.model_is_local = (int32_t)q.is_local;
    for (int i = 0; i < 12; ++i) o.proj_matrix[i] = q.model[i];
    if (flags[b]) {
      o.focal_params[0] = cam.params[0] * o.focal_length_factor;
      o.focal_params[1] = two ? cam.params[1] * o.focal_length_factor : o.focal_params[0];
    }
    ap_quaternion(o.proj_matrix, o.qvec);
    for (int i = 0; i < 3; ++i) o.tvec[i] = o.proj_matrix[4 * i + 3];
    bool nan = false;
    for (int i = 0; i < 4; ++i) nan = nan || isnan(o.qvec[i]);
    for (int i = 0; i < 3; ++i) nan = nan || isnan(o.tvec[i]);
    o.success = nan ? 0 : 1;
  }
  res[b] = o;
  win_run[b] = o.success ? win : -1;
  for (int i = 0; i < AP_MARGINS; ++i) margins[(size_t)b * AP_MARGINS + i] = mg[i];
}

__global__ void __launch_bounds__(256) k_ap_mask(uint32_t B, const uint64_t* offsets, const int32_t* win_run, const ApRun* runs,
                                                 const uint8_t* mask, uint8_t* out) {
  for (uint32_t b = blockIdx.y; b < B; b += gridDim.y) {
    const uint64_t n = offsets[b + 1] - offsets[b];
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) continue;
    const int32_t w = win_run[b];
    out[offsets[b] + i] = w >= 0 ? mask[runs[w].roff + i] : (uint8_t)0;
  }
}

// ComputeNumTrials (ransac.h:151-167) with kMinNumSamples = 3, clamped to 32 bits (UINT32_MAX: never below the trial count)
uint32_t ap_num_trials(uint64_t k, uint64_t n, double confidence) {
  const double ratio = k / static_cast<double>(n);
  const double nom = 1 - confidence;
  if (nom <= 0) return UINT32_MAX;
  const double denom = 1 - std::pow(ratio, 3);
  if (denom <= 0) return 1;
  const double v = std::ceil(std::log(nom) / std::log(denom));
  if (!(v >= 0.0) || v >= 4294967295.0) return UINT32_MAX;
  return static_cast<uint32_t>(v);
}

bool ap_options_ok(const dsm_absolute_pose_options& o) {
  // AbsolutePoseEstimationOptions::Check (pose.h:72-75) and RANSACOptions::Check (ransac.h:65-70); non-finite values fail
  return o.num_focal_length_samples > 0 && o.min_focal_length_ratio > 0 && o.max_focal_length_ratio > 0 &&
         o.min_focal_length_ratio < o.max_focal_length_ratio && std::isfinite(o.max_focal_length_ratio) && o.max_error > 0 &&
         std::isfinite(o.max_error) && o.min_inlier_ratio >= 0 && o.min_inlier_ratio <= 1 && o.confidence >= 0 && o.confidence <= 1 &&
         o.min_num_trials <= o.max_num_trials;
}

struct ApBufs {
  DevBuf runs, xy, X, un, vn, sidx, mask, alphas, tab, out, run0, factors, cams, flags, res, win, margins, offsets, omask;
};

}  // namespace

extern "C" void dsm_default_absolute_pose_options(dsm_absolute_pose_options* o) {
  o->num_focal_length_samples = 30;   // incremental_mapper.cc:440
  o->reserved = 0;
  o->min_focal_length_ratio = 0.1;    // incremental_mapper.h:106
  o->max_focal_length_ratio = 10.0;   // incremental_mapper.h:107
  o->max_error = 12.0;                // abs_pose_max_error, incremental_mapper.h:84
  o->min_inlier_ratio = 0.25;         // abs_pose_min_inlier_ratio, incremental_mapper.h:90
  o->confidence = 0.9999;             // incremental_mapper.cc:449
  o->min_num_trials = 30;             // incremental_mapper.cc:448
  o->max_num_trials = UINT64_MAX;     // RANSACOptions' default (ransac.h:62); the constructor's cap makes it 585
  o->random_seed = 0;
  o->reserved2 = 0;
}

extern "C" uint32_t dsm_absolute_pose_seed(uint32_t problem, uint32_t factor_index, uint32_t user_seed) {
  // two 32-bit indices through the 64-bit finaliser dsm_pair_seed uses
  uint64_t h = ((uint64_t)problem << 32) | (uint64_t)factor_index;
  h += 0x9e3779b97f4a7c15ull;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return (uint32_t)h ^ user_seed;
}

extern "C" uint32_t dsm_absolute_pose_factors(const dsm_absolute_pose_options* options, double* factors_out, uint32_t capacity) {
  dsm_absolute_pose_options o;
  if (options)
    o = *options;
  else
    dsm_default_absolute_pose_options(&o);
  if (!ap_options_ok(o)) return 0;
  // pose.cc:92-98 as written: the loop's length is decided by the accumulated rounding of f += fstep
  const double fstep = 1.0 / o.num_focal_length_samples;
  const double fscale = o.max_focal_length_ratio - o.min_focal_length_ratio;
  uint32_t n = 0;
  for (double f = 0; f <= 1.0; f += fstep) {
    if (factors_out && n < capacity) factors_out[n] = o.min_focal_length_ratio + fscale * f * f;
    ++n;
    if (n > DSM_ABSOLUTE_POSE_MAX_FACTORS) break;
  }
  return n;
}

extern "C" uint64_t dsm_absolute_pose_max_trials(const dsm_absolute_pose_options* options) {
  dsm_absolute_pose_options o;
  if (options)
    o = *options;
  else
    dsm_default_absolute_pose_options(&o);
  const uint64_t kNumSamples = 100000;
  const uint32_t dyn = ap_num_trials(static_cast<uint64_t>(o.min_inlier_ratio * kNumSamples), kNumSamples, o.confidence);
  return dyn == UINT32_MAX ? o.max_num_trials : std::min<uint64_t>(o.max_num_trials, dyn);
}

extern "C" int dsm_estimate_absolute_poses(dsm_ctx* ctx, uint32_t num_problems, const dsm_camera* cameras,
                                           const uint8_t* estimate_focal_length, const uint64_t* offsets, const double* points2D,
                                           const double* points3D, const dsm_absolute_pose_options* options, const uint32_t* seeds,
                                           dsm_absolute_pose_result* results_out, uint8_t* inlier_mask_out, double* margins_out,
                                           dsm_absolute_pose_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_estimate_absolute_poses", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  const uint32_t B = num_problems;
  if (!offsets || (B && (!cameras || !estimate_focal_length || !results_out))) return fail("NULL argument");
  dsm_absolute_pose_options o;
  if (options)
    o = *options;
  else
    dsm_default_absolute_pose_options(&o);
  if (!ap_options_ok(o)) return fail("option out of range");
  if (offsets[0] != 0) return fail("offsets must start at 0");
  for (uint32_t b = 0; b < B; ++b) {
    if (offsets[b + 1] < offsets[b]) return fail("offsets must ascend");
    if (offsets[b + 1] - offsets[b] > DSM_ABSOLUTE_POSE_MAX_POINTS) return fail("more than 1048576 correspondences in one problem");
  }
  const uint64_t T = offsets[B];
  if (T && (!points2D || !points3D || !inlier_mask_out)) return fail("NULL argument");
  for (uint64_t i = 0; i < 2 * T; ++i)
    if (!std::isfinite(points2D[i])) return fail("non-finite points2D");
  for (uint64_t i = 0; i < 3 * T; ++i)
    if (!std::isfinite(points3D[i])) return fail("non-finite points3D");
  for (uint32_t b = 0; b < B; ++b) {
    const dsm_camera& k = cameras[b];
    if (!cam_model_exists(k.model_id)) return fail("an unknown camera model");
    for (int i = 0; i < cam_num_params(k.model_id); ++i)
      if (!std::isfinite(k.params[i])) return fail("non-finite camera parameters");
  }
  const uint32_t S = dsm_absolute_pose_factors(&o, nullptr, 0);
  if (S == 0 || S > DSM_ABSOLUTE_POSE_MAX_FACTORS) return fail("more than 1024 focal-length factors");
  std::vector<double> factors(S);
  dsm_absolute_pose_factors(&o, factors.data(), S);
  const uint64_t max_trials64 = dsm_absolute_pose_max_trials(&o);
  if (max_trials64 > DSM_ABSOLUTE_POSE_MAX_TRIALS)
    return fail("the options leave a run's trial count above 1000000 (confidence = 1 or min_inlier_ratio = 0): set max_num_trials");
  const uint32_t max_trials = (uint32_t)std::min<uint64_t>(max_trials64, 0xfffffff0u);
  const uint32_t min_trials = (uint32_t)std::min<uint64_t>(o.min_num_trials, 0xfffffff0u);

  // the runs, the ComputeNumTrials tables (one per distinct N, host libm)
  std::vector<ApRun> runs;
  std::vector<uint32_t> run0(B + 1, 0), tab;
  std::map<uint32_t, uint32_t> tab_of;
  uint64_t RP = 0;
  uint32_t maxN = 0;
  for (uint32_t b = 0; b < B; ++b) {
    const uint32_t N = (uint32_t)(offsets[b + 1] - offsets[b]);
    maxN = std::max(maxN, N);
    auto it = tab_of.find(N);
    if (it == tab_of.end()) {
      it = tab_of.emplace(N, (uint32_t)tab.size()).first;
      for (uint32_t k = 0; k <= N; ++k) tab.push_back(N ? ap_num_trials(k, N, o.confidence) : UINT32_MAX);
    }
    const uint32_t ns = estimate_focal_length[b] ? S : 1;
    for (uint32_t s = 0; s < ns; ++s) {
      ApRun r;
      r.poff = offsets[b];
      r.roff = RP;
      r.N = N;
      r.seed = seeds ? seeds[(size_t)b * S + s] : dsm_absolute_pose_seed(b, s, o.random_seed);
      r.tab_off = it->second;
      r.problem = b;
      r.cam = cameras[b];
      const double f = estimate_focal_length[b] ? factors[s] : 1.0;
      const bool two = cam_two_focal(r.cam.model_id);
      r.cam.params[0] *= f;  // FocalLengthIdxs
      if (two) r.cam.params[1] *= f;
      // ImageToWorldThreshold (camera_models.h:535-543) of the scaled camera, then LORANSAC's max_error^2
      double mean_focal = 0;
      if (two) {
        mean_focal += r.cam.params[0];
        mean_focal += r.cam.params[1];
        mean_focal /= 2;
      } else {
        mean_focal += r.cam.params[0];
        mean_focal /= 1;
      }
      const double me = o.max_error / mean_focal;
      r.max_residual = me * me;
      runs.push_back(r);
      RP += N;
    }
    run0[b + 1] = (uint32_t)runs.size();
  }
  const uint32_t R = (uint32_t)runs.size();
  if (RP >= 0x80000000ull) return fail("too many correspondences times factors in one call (2^31)");
  const double setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();

  dsm_absolute_pose_report rep{};
  rep.num_problems = B;
  rep.num_factors = S;
  rep.num_runs = R;
  for (int i = 0; i < AP_MARGINS; ++i) rep.min_margin[i] = INFINITY;
  rep.setup_ms = setup_ms;
  if (B == 0) {
    if (report) *report = rep;
    return DSM_OK;
  }

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  ApBufs d;
  DevEvents<4> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  const size_t RP1 = std::max<uint64_t>(RP, 1), T1 = std::max<uint64_t>(T, 1);
  HIPCHK(ctx, dev_upload(d.runs, runs.data(), runs.size() * sizeof(ApRun), st));
  HIPCHK(ctx, dev_upload(d.xy, points2D, T * 16, st));
  HIPCHK(ctx, dev_upload(d.X, points3D, T * 24, st));
  HIPCHK(ctx, dev_upload(d.tab, tab.data(), tab.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.run0, run0.data(), run0.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.factors, factors.data(), factors.size() * 8, st));
  HIPCHK(ctx, dev_upload(d.cams, cameras, (size_t)B * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.flags, estimate_focal_length, B, st));
  HIPCHK(ctx, dev_upload(d.offsets, offsets, ((size_t)B + 1) * 8, st));
  for (DevBuf* b : {&d.un, &d.vn}) HIPCHK(ctx, b->reserve(RP1 * 8));
  HIPCHK(ctx, d.sidx.reserve(RP1 * 4));
  HIPCHK(ctx, d.mask.reserve(RP1));
  HIPCHK(ctx, d.alphas.reserve(RP1 * 32));
  HIPCHK(ctx, d.out.reserve((size_t)R * sizeof(ApOut)));
  HIPCHK(ctx, d.res.reserve((size_t)B * sizeof(dsm_absolute_pose_result)));
  HIPCHK(ctx, d.win.reserve((size_t)B * 4));
  HIPCHK(ctx, d.margins.reserve((size_t)B * AP_MARGINS * 8));
  HIPCHK(ctx, d.omask.reserve(T1));
  ApParams prm;
  prm.runs = d.runs.as<ApRun>();
  prm.n_runs = R;
  prm.xy = d.xy.as<double>();
  prm.X = d.X.as<double>();
  prm.un = d.un.as<double>();
  prm.vn = d.vn.as<double>();
  prm.sidx = d.sidx.as<uint32_t>();
  prm.mask = d.mask.as<uint8_t>();
  prm.alphas = d.alphas.as<double>();
  prm.tab = d.tab.as<uint32_t>();
  prm.max_trials = max_trials;
  prm.min_trials = min_trials;
  prm.out = d.out.as<ApOut>();
  if (maxN)
    hipLaunchKernelGGL(k_ap_prepare, dim3((maxN + 255) / 256, std::min<uint32_t>(R, 65535u)), dim3(256), 0, st, prm);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  hipLaunchKernelGGL(k_ap_ransac, dim3(R), dim3(64), 0, st, prm);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  hipLaunchKernelGGL(k_ap_choose, dim3((B + 63) / 64), dim3(64), 0, st, B, d.run0.as<uint32_t>(), d.out.as<ApOut>(), d.factors.as<double>(),
                     d.cams.as<dsm_camera>(), d.flags.as<uint8_t>(), d.res.as<dsm_absolute_pose_result>(), d.win.as<int32_t>(),
                     d.margins.as<double>());
  if (maxN)
    hipLaunchKernelGGL(k_ap_mask, dim3((maxN + 255) / 256, std::min<uint32_t>(B, 65535u)), dim3(256), 0, st, B, d.offsets.as<uint64_t>(),
                       d.win.as<int32_t>(), d.runs.as<ApRun>(), d.mask.as<uint8_t>(), d.omask.as<uint8_t>());
  HIPCHK(ctx, hipGetLastError());
  std::vector<ApOut> outs(R);
  std::vector<double> margins((size_t)B * AP_MARGINS);
  HIPCHK(ctx, hipMemcpyAsync(results_out, d.res.p, (size_t)B * sizeof(dsm_absolute_pose_result), hipMemcpyDeviceToHost, st));
  if (T) HIPCHK(ctx, hipMemcpyAsync(inlier_mask_out, d.omask.p, T, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(outs.data(), d.out.p, (size_t)R * sizeof(ApOut), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(margins.data(), d.margins.p, margins.size() * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (const ApOut& q : outs) {
    rep.num_trials += q.num_trials;
    rep.num_models += q.num_models;
    rep.num_local_optimizations += q.num_lo;
  }
  for (uint32_t b = 0; b < B; ++b)
    for (int i = 0; i < AP_MARGINS; ++i) {
      rep.min_margin[i] = std::min(rep.min_margin[i], margins[(size_t)b * AP_MARGINS + i]);
      if (margins_out) margins_out[(size_t)b * AP_MARGINS + i] = margins[(size_t)b * AP_MARGINS + i];
    }
  HIPCHK(ctx, ev.ms(0, 1, &rep.prepare_ms));
  HIPCHK(ctx, ev.ms(1, 2, &rep.ransac_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rep.choice_ms));
  HIPCHK(ctx, ev.ms(0, 3, &rep.device_ms));
  if (report) *report = rep;
  return DSM_OK;
}
