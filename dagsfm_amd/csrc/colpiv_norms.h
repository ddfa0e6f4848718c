// colpiv_norms.h -- the column-norm bookkeeping of Eigen's ColPivHouseholderQR, kept as CERTIFIED DECISIONS instead of as
// exact bits ("pivot norms").
//
// Eigen tracks per remaining column j an updated norm nu_j and the norm nd_j of its last direct computation.  Nothing that
// reaches a model reads either: they decide (P) which column is the next pivot -- the first largest nu --, (Z) whether a
// column is skipped (nu_j == 0) and (R) whether nu_j is recomputed (temp2 <= sqrt(DBL_EPSILON)).  Per step and column the
// exact form costs two IEEE divisions, one IEEE square root and about ten further operations.  The tracker below keeps the
// SQUARES, s_j ~ nu_j^2 and sd_j ~ nd_j^2, with one multiply and one subtract per step and column, and says for every
// decision whether it is provably the one Eigen's sequence takes.  A solver that sees one uncertain decision discards its
// result and runs the exact form; where all are certain the pivots, skips and recomputes are Eigen's, and since the
// Householder arithmetic is not touched the factorisation has the same bits.
//
// ---------------------------------------------------------------------------------------------------------- derivation
// u = 2^-53; eps_i are roundings, |eps_i| <= u.  One column, since its last direct computation (start, or a recompute):
//   both forms compute the SAME ss = fl(sum a_i^2) (same operations, same order); Eigen keeps nd = nu = fl(sqrt(ss)), the
//   tracker sd = s = ss.  Range guard: ss == 0, or 2^-500 <= ss <= 2^500; anything else (NaN, Inf included) is uncertain.
//   Inside the guard no square, quotient or product below underflows or overflows by more than 2^-1074 absolute, which is
//   below u^2 sd and is left out of the bounds.
//   (Z) fl(sqrt(ss)) == 0 iff ss == 0, and a non-zero nu never becomes zero by a downdate (it is multiplied by
//       sqrt(temp) > 2^-14, see (R)), so "nu_j == 0" is exactly "sd_j == 0": no margin needed.
//   e := nu^2 - s.  At the direct computation nu^2 = ss (1 + eps)^2, so |e| <= 2.1 u sd, and nd^2 = sd (1 + d), |d| <= 2.1 u.
//   One downdate with x = |a[j][K]|, r = x / nu:
//     Eigen   t = r (1 + eps1);  temp = fl(fl(1 + t) fl(1 - t)) = (1 - t^2)(1 + eps2)(1 + eps3)(1 + eps4), clamped at 0.
//             If t >= 1 the clamp (or the exact zero) gives temp2 = 0: RECOMPUTE.  Otherwise 0 < 1 - t^2 <= 1, r < 1 + 2u and
//               temp = 1 - r^2 + eta,  |eta| <= 2.1 u r^2 + 3.1 u (1 - t^2) <= 5.3 u
//             P := nu^2 temp = nu^2 - x^2 + eta nu^2                                   (a real number, no rounding)
//             temp2 = fl(temp fl(ratio ratio)), ratio = fl(nu / nd):  temp2 = P / nd^2 (1 + th'), |th'| <= 4.1 u
//             recompute iff temp2 <= 2^-26, i.e. iff P <= 2^-26 sd (1 + k), |k| <= 6.3 u                       ... (R)
//             else nu' = fl(nu fl(sqrt(temp))): nu'^2 = P (1 + th), |th| <= 4.1 u.  temp <= 1 + 2u gives nu'^2 <= nu^2 (1 + 7u),
//             so nu^2 <= 1.01 nd^2 throughout the at most 7 downdates of a 9 x M factorisation, M <= 8.
//     tracker s1 = fl(s - fl(x x)) = s - x^2 + z, |z| <= u x^2 + 1.01 u max(s, x^2) <= 2.2 u nd^2
//             (x^2 <= 1.01 nu^2 when t < 1, s <= nu^2 + |e|).  A contracted s1 = fma(-x, x, s) has the smaller error of the two.
//     So |P - s1| <= |e| + 5.3 u nu^2 + 2.2 u nd^2  and  |nu'^2 - s1| <= |P - s1| + 4.1 u P:  each downdate adds at most
//     12 u nd^2 to |e|, and after 7 of them   |e| <= (2.1 + 7 * 12) u nd^2 < 100 u sd =: E sd,   |P - s1| <= E sd  as well.
//     In the case t >= 1: x^2 >= nu^2 (1 - 2u), so s1 <= |e| + 2 u nu^2 + z <= (E + 5u) sd, far below 2^-26 sd.
//   Certificates, with the margin MU = 2^-44 = 512 u > 5 E  (the factor 5 is slack, not measurement):
//   (R) s1 > (2^-26 + MU) sd  =>  P > 2^-26 sd + (MU - E) sd > 2^-26 sd (1 + k): Eigen does not recompute (and t < 1).
//       s1 < (2^-26 - MU) sd  =>  either t >= 1, or P < 2^-26 sd (1 + k): Eigen recomputes.  Between the two: uncertain.
//       (The two products with sd round once each, 2^-79 sd: nothing against MU - E.)
//   (P) the pivot is the first largest s; it is certified when every other remaining column j has
//       s_b - s_j > MU (sd_b + sd_j):  then nu_b^2 - nu_j^2 > (MU (1 - 4u) - 1.01 E)(sd_b + sd_j) >= 0, so nu_b > nu_j strictly
//       and Eigen's first-largest scan ends on b whichever side of b the column j stands.  A tie, exact or within the
//       margin, is never certified -- two zero columns included.
//   By induction over the steps: as long as every decision was certified both forms permuted, skipped and recomputed alike, so
//   they hold the same matrix bits and the bounds above apply to the next step.
// The comparisons are written so that a NaN fails the certificate.
#ifndef DAGSFM_AMD_CSRC_COLPIV_NORMS_H_
#define DAGSFM_AMD_CSRC_COLPIV_NORMS_H_

#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define DSM_CPN static __host__ __device__ __forceinline__
#else
#define DSM_CPN static inline
#endif

constexpr double kCpnMargin = 0x1p-44;                    // MU
constexpr double kCpnRecomputeBelow = 0x1p-26 - 0x1p-44;  // exact: 2^-26 (1 - 2^-18)
constexpr double kCpnKeepAbove = 0x1p-26 + 0x1p-44;
constexpr double kCpnRangeLo = 0x1p-500, kCpnRangeHi = 0x1p500;

// a directly computed squared norm the bounds hold for
DSM_CPN bool cpn_range_ok(double ss) { return ss == 0.0 || (ss >= kCpnRangeLo && ss <= kCpnRangeHi); }

// (P) is column j certainly below the chosen pivot b?
DSM_CPN bool cpn_pivot_clear(double s_b, double sd_b, double s_j, double sd_j) { return s_b - s_j > kCpnMargin * (sd_b + sd_j); }

// (Z) + (R) for a column with sd != 0: s becomes the downdated value; returns whether the column is to be recomputed directly
// and clears `certain` where that is too close to call
DSM_CPN bool cpn_downdate(double& s, double sd, double x, bool& certain) {
  s -= x * x;
  const bool recompute = s < kCpnRecomputeBelow * sd;
  certain = certain && (recompute || s > kCpnKeepAbove * sd);
  return recompute;
}

// ---------------------------------------------------------------------------------------------------------- decision traces
// ColPivHouseholderQR::computeInPlace of a 9 x m column-major matrix (m <= 8), loops in Eigen's order with plain divisions (the
// values the solvers' shared-divisor quotients reproduce), with the bookkeeping of choice; what the host build
// (colpiv_norms_host.cpp) exports and tests/test_colpiv_norms_cpu.py compares.  pivots[k]: the column taken at step k;
// recomputes[k * 8 + j]: 1 where the column standing at position j after step k's swap was recomputed directly, else 0.
// Returns whether every decision was certified (the exact form: always 1).
DSM_CPN void cpn_householder_step(double* qr, int m, int k, double* hco) {
  double tail_sq = 0.0;
  for (int i = k + 1; i < 9; ++i) tail_sq += qr[k * 9 + i] * qr[k * 9 + i];
  const double c0 = qr[k * 9 + k];
  double tau, beta;
  if (tail_sq <= DBL_MIN) {
    tau = 0.0;
    beta = c0;
    for (int i = k + 1; i < 9; ++i) qr[k * 9 + i] = 0.0;
  } else {
    double b = sqrt(c0 * c0 + tail_sq);
    if (c0 >= 0.0) b = -b;
    for (int i = k + 1; i < 9; ++i) qr[k * 9 + i] = qr[k * 9 + i] / (c0 - b);
    tau = (b - c0) / b;
    beta = b;
  }
  hco[k] = tau;
  qr[k * 9 + k] = beta;
  if (tau != 0.0) {
    for (int j = k + 1; j < m; ++j) {
      double tmp = 0.0;
      for (int i = k + 1; i < 9; ++i) tmp += qr[k * 9 + i] * qr[j * 9 + i];
      tmp += qr[j * 9 + k];
      qr[j * 9 + k] -= tau * tmp;
      for (int i = k + 1; i < 9; ++i) qr[j * 9 + i] -= tau * qr[k * 9 + i] * tmp;
    }
  }
}
DSM_CPN void cpn_swap_columns(double* qr, int a, int b) {
  for (int i = 0; i < 9; ++i) {
    const double t = qr[a * 9 + i];
    qr[a * 9 + i] = qr[b * 9 + i];
    qr[b * 9 + i] = t;
  }
}

DSM_CPN int cpn_trace_exact(double* qr, int m, int* pivots, int* recomputes) {
  double nu[8], nd[8], hco[8];
  for (int k = 0; k < m; ++k) {
    double ss = 0.0;
    for (int i = 0; i < 9; ++i) ss += qr[k * 9 + i] * qr[k * 9 + i];
    nd[k] = sqrt(ss);
    nu[k] = nd[k];
  }
  const double thr = sqrt(DBL_EPSILON);
  for (int k = 0; k < m; ++k) {
    int biggest = k;
    double mx = nu[k];
    for (int j = k + 1; j < m; ++j)
      if (nu[j] > mx) {
        mx = nu[j];
        biggest = j;
      }
    pivots[k] = biggest;
    if (biggest != k) {
      cpn_swap_columns(qr, k, biggest);
      double t = nu[k];
      nu[k] = nu[biggest];
      nu[biggest] = t;
      t = nd[k];
      nd[k] = nd[biggest];
      nd[biggest] = t;
    }
    cpn_householder_step(qr, m, k, hco);
    for (int j = 0; j < 8; ++j) recomputes[k * 8 + j] = 0;
    for (int j = k + 1; j < m; ++j) {
      if (nu[j] != 0.0) {
        double temp = fabs(qr[j * 9 + k]) / nu[j];
        temp = (1.0 + temp) * (1.0 - temp);
        temp = temp < 0.0 ? 0.0 : temp;
        const double ratio = nu[j] / nd[j];
        const double temp2 = temp * (ratio * ratio);
        if (temp2 <= thr) {
          double ss = 0.0;
          for (int i = k + 1; i < 9; ++i) ss += qr[j * 9 + i] * qr[j * 9 + i];
          nd[j] = sqrt(ss);
          nu[j] = nd[j];
          recomputes[k * 8 + j] = 1;
        } else {
          nu[j] *= sqrt(temp);
        }
      }
    }
  }
  return 1;
}

DSM_CPN int cpn_trace_certified(double* qr, int m, int* pivots, int* recomputes) {
  double s[8], sd[8], hco[8];
  bool certain = true;
  for (int k = 0; k < m; ++k) {
    double ss = 0.0;
    for (int i = 0; i < 9; ++i) ss += qr[k * 9 + i] * qr[k * 9 + i];
    s[k] = sd[k] = ss;
    certain = certain && cpn_range_ok(ss);
  }
  for (int k = 0; k < m; ++k) {
    int biggest = k;
    double mx = s[k];
    for (int j = k + 1; j < m; ++j)
      if (s[j] > mx) {
        mx = s[j];
        biggest = j;
      }
    pivots[k] = biggest;
    if (biggest != k) {
      cpn_swap_columns(qr, k, biggest);
      double t = s[k];
      s[k] = s[biggest];
      s[biggest] = t;
      t = sd[k];
      sd[k] = sd[biggest];
      sd[biggest] = t;
    }
    for (int j = k + 1; j < m; ++j) certain = certain && cpn_pivot_clear(s[k], sd[k], s[j], sd[j]);
    cpn_householder_step(qr, m, k, hco);
    for (int j = 0; j < 8; ++j) recomputes[k * 8 + j] = 0;
    for (int j = k + 1; j < m; ++j) {
      if (sd[j] != 0.0) {
        if (cpn_downdate(s[j], sd[j], fabs(qr[j * 9 + k]), certain)) {
          double ss = 0.0;
          for (int i = k + 1; i < 9; ++i) ss += qr[j * 9 + i] * qr[j * 9 + i];
          s[j] = sd[j] = ss;
          certain = certain && cpn_range_ok(ss);
          recomputes[k * 8 + j] = 1;
        }
      }
    }
  }
  return certain ? 1 : 0;
}

#endif  // DAGSFM_AMD_CSRC_COLPIV_NORMS_H_
