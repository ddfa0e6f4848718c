// tri_angle.h -- CalculateTriangulationAngle (triangulation.cc:122-145) with the device libm's acos, for the stages whose
// parity tests hold them to it (re-triangulation, the point filters).
//
// initial_pair.h's ip_tri_angle is the deliberately different statement: it takes acos from exact_acos.h (dsm_acos), because
// the initial pair and the next-image ranking sort and take medians of these angles and are held to their host builds bit
// for bit, which a libm acos that differs between host and device cannot give.  Do not merge the two, and do not change
// which acos a stage uses.
#ifndef DAGSFM_AMD_CSRC_TRI_ANGLE_H_
#define DAGSFM_AMD_CSRC_TRI_ANGLE_H_

#include <hip/hip_runtime.h>
#include <math.h>

// the angle at X between the rays to the centres c1 and c2, folded to [0, pi / 2]; NaN when the ratio rounds outside [-1, 1],
// as the reference's
__device__ inline double tri_angle_libm(const double* c1, const double* c2, const double* X) {
  const double b0 = c1[0] - c2[0], b1 = c1[1] - c2[1], b2 = c1[2] - c2[2];
  const double r0 = X[0] - c1[0], r1 = X[1] - c1[1], r2 = X[2] - c1[2];
  const double s0 = X[0] - c2[0], s1 = X[1] - c2[1], s2 = X[2] - c2[2];
  const double base2 = (b0 * b0 + b1 * b1) + b2 * b2;
  const double ray1 = (r0 * r0 + r1 * r1) + r2 * r2, ray2 = (s0 * s0 + s1 * s1) + s2 * s2;
  const double den = 2.0 * sqrt(ray1 * ray2);
  if (den == 0.0) return 0.0;
  const double nom = (ray1 + ray2) - base2;
  const double a = fabs(acos(nom / den));
  const double c = M_PI - a;
  return c < a ? c : a;  // std::min(a, c): NaN stays NaN
}

#endif  // DAGSFM_AMD_CSRC_TRI_ANGLE_H_
