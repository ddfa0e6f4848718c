// exact_acos.h -- acos restated so that the device, the host build and tests/source_selection_ref.py agree on every bit.
//
// CalculateTriangulationAngle (the reference's src/base/triangulation.cc:122-145) calls std::acos, and the source selection
// of DESIGN.md 28 compares the float rounding of its result with a threshold and takes order statistics of it.  The reference
// pins no libm; the contract is exact_trig.h's: the CORRECTLY ROUNDED value, computed in double-double arithmetic (~100 bits).
//
//   s = sqrt((1 - q)(1 + q))       1 - q and 1 + q are exact double-doubles (two_sum), so s keeps its relative accuracy at |q| -> 1
//   acos(q) = atan(s / q)          q >  s   (the quotient is in [0, 1))
//           = pi/2 - atan(q / s)   |q| <= s (the quotient is in [-1, 1])
//           = pi + atan(s / q)     q < -s   (the quotient is in (-1, 0])
// with atan of a double-double argument by dsm_atan's own reduction (nearest eighth, 16 series terms).  Every step has a
// relative error below ~2^-98, so hi is the correctly rounded double except where acos(q) lies within 2^-45 ulps of a rounding
// boundary.  tests/test_source_selection_cpu.py holds the host build to mpmath at 300 bits with equality, and to the host libm
// within 1 ulp.
//
// Plain IEEE double operations and the correctly rounded IEEE square root, in a fixed order, no FMA (both builds use
// -ffp-contract=off).  The includer defines DSM_XT and DSM_XT_CONST as for exact_trig.h, which this header includes.
#ifndef DAGSFM_AMD_CSRC_EXACT_ACOS_H_
#define DAGSFM_AMD_CSRC_EXACT_ACOS_H_

#include "exact_trig.h"

namespace dsm_xt {

// sqrt of a double-double a >= 0: one Newton step on the double root, the residual taken exactly
DSM_XT dd dd_sqrt(dd a) {
  if (!(a.hi > 0.0)) return dd{0.0, 0.0};
  const double x = __builtin_sqrt(a.hi);
  const dd r = dd_add(a, dd_neg(two_prod(x, x)));
  return quick_two_sum(x, r.hi / (2.0 * x));
}

// atan of a double-double |y| <= 1 (dsm_atan's reduction and series)
DSM_XT dd dd_atan_unit(dd y) {
  const bool neg = y.hi < 0.0;
  if (neg) y = dd_neg(y);
  const int k = (int)(y.hi * 8.0 + 0.5);  // nearest eighth, 0 .. 8
  const double c = (double)k * 0.125;
  // t = (y - c) / (1 + y c), |t| <= ~1/16;  atan(y) = atan(c) + atan(t)
  const dd num = dd_add_d(y, -c);
  const dd den = dd_add_d(dd_mul_d(y, c), 1.0);
  const dd t = dd_div(num, den);
  const dd t2 = dd_mul(t, t);
  dd s = dd{kInvOdd[15][0], kInvOdd[15][1]};
  for (int n = 14; n >= 0; --n) {
    s = dd_mul(s, t2);
    s = dd_add(dd{kInvOdd[n][0], kInvOdd[n][1]}, dd_neg(s));
  }
  const dd r = dd_add(dd{kAtanEighths[k][0], kAtanEighths[k][1]}, dd_mul(s, t));
  return neg ? dd_neg(r) : r;
}

}  // namespace dsm_xt

// acos(q): correctly rounded (see the header comment); NaN for |q| > 1 and for NaN
DSM_XT double dsm_acos(double q) {
  using namespace dsm_xt;
  if (!(q >= -1.0 && q <= 1.0)) return __builtin_nan("");
  if (q == 1.0) return 0.0;
  const dd s = dd_sqrt(dd_mul(two_sum(1.0, -q), two_sum(1.0, q)));
  const dd pio2 = dd{kPio2DD[0], kPio2DD[1]};
  const double aq = q < 0.0 ? -q : q;
  if (aq <= s.hi) return dd_add(pio2, dd_neg(dd_atan_unit(dd_div(dd{q, 0.0}, s)))).hi;
  const dd a = dd_atan_unit(dd_div(s, dd{q, 0.0}));
  if (q > 0.0) return a.hi;
  return dd_add(dd_add(pio2, pio2), a).hi;
}

#endif  // DAGSFM_AMD_CSRC_EXACT_ACOS_H_
