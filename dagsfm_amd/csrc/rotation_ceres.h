// rotation_ceres.h -- ceres' rotation conversions (ceres/rotation.h), restated from the published formulas for the device:
// QuaternionToAngleAxis, AngleAxisToRotationMatrix (row-major here) and RotationMatrixToQuaternion.  The reference's
// RotationMatrixToAngleAxis is RotationMatrixToQuaternion followed by QuaternionToAngleAxis.  Shared by the view-graph
// kernels (view_graph.hip: the rotation-cycle filter; rotation_averaging.hip: global rotation averaging).
#ifndef DSM_ROTATION_CERES_H_
#define DSM_ROTATION_CERES_H_
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>

static __device__ inline void ceres_quaternion_to_angle_axis(const double* q, double* aa) {
  const double q1 = q[1], q2 = q[2], q3 = q[3];
  const double sin_squared_theta = q1 * q1 + q2 * q2 + q3 * q3;
  double k = 2.0;
  if (sin_squared_theta > 0.0) {
    const double sin_theta = sqrt(sin_squared_theta);
    const double cos_theta = q[0];
    const double two_theta = 2.0 * ((cos_theta < 0.0) ? atan2(-sin_theta, -cos_theta) : atan2(sin_theta, cos_theta));
    k = two_theta / sin_theta;
  }
  aa[0] = q1 * k;
  aa[1] = q2 * k;
  aa[2] = q3 * k;
}
static __device__ inline void ceres_angle_axis_to_rotation(const double* aa, double* R) {  // row-major
  const double theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2 > DBL_EPSILON) {
    const double theta = sqrt(theta2);
    const double wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    const double costheta = cos(theta), sintheta = sin(theta);
    R[0] = costheta + wx * wx * (1.0 - costheta);
    R[3] = wz * sintheta + wx * wy * (1.0 - costheta);
    R[6] = -wy * sintheta + wx * wz * (1.0 - costheta);
    R[1] = wx * wy * (1.0 - costheta) - wz * sintheta;
    R[4] = costheta + wy * wy * (1.0 - costheta);
    R[7] = wx * sintheta + wy * wz * (1.0 - costheta);
    R[2] = wy * sintheta + wx * wz * (1.0 - costheta);
    R[5] = -wx * sintheta + wy * wz * (1.0 - costheta);
    R[8] = costheta + wz * wz * (1.0 - costheta);
  } else {
    R[0] = 1.0; R[3] = aa[2]; R[6] = -aa[1];
    R[1] = -aa[2]; R[4] = 1.0; R[7] = aa[0];
    R[2] = aa[1]; R[5] = -aa[0]; R[8] = 1.0;
  }
}
static __device__ inline void ceres_rotation_to_quaternion(const double* R, double* q) {
  const double trace = R[0] + R[4] + R[8];
  if (trace >= 0.0) {
    double t = sqrt(trace + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (R[7] - R[5]) * t;
    q[2] = (R[2] - R[6]) * t;
    q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 3 + i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    double t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i + 1] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j + 1] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k + 1] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}

// ---------------------------------------------------------------- the same conversions over forward-mode dual numbers
// (nonlinear_rotation.hip).  ceres differentiates these functions with Jets, and a Jet compares by its value part: the
// derivative is that of the branch that is evaluated, not the limit of the other one.  The templates below restate the three
// functions above operation by operation over T = RotDual<N>; the double functions above are what every other kernel calls.
template <int N>
struct RotDual {
  double v;
  double d[N];
};
template <int N>
__device__ inline RotDual<N> rd_const(double c) {
  RotDual<N> r;
  r.v = c;
  for (int k = 0; k < N; ++k) r.d[k] = 0.0;
  return r;
}
template <int N>
__device__ inline RotDual<N> operator+(const RotDual<N>& a, const RotDual<N>& b) {
  RotDual<N> r;
  r.v = a.v + b.v;
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] + b.d[k];
  return r;
}
template <int N>
__device__ inline RotDual<N> operator-(const RotDual<N>& a, const RotDual<N>& b) {
  RotDual<N> r;
  r.v = a.v - b.v;
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] - b.d[k];
  return r;
}
template <int N>
__device__ inline RotDual<N> operator-(const RotDual<N>& a) {
  RotDual<N> r;
  r.v = -a.v;
  for (int k = 0; k < N; ++k) r.d[k] = -a.d[k];
  return r;
}
template <int N>
__device__ inline RotDual<N> operator*(const RotDual<N>& a, const RotDual<N>& b) {
  RotDual<N> r;
  r.v = a.v * b.v;
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
  return r;
}
template <int N>
__device__ inline RotDual<N> operator*(const RotDual<N>& a, double b) {
  RotDual<N> r;
  r.v = a.v * b;
  for (int k = 0; k < N; ++k) r.d[k] = a.d[k] * b;
  return r;
}
template <int N>
__device__ inline RotDual<N> operator+(const RotDual<N>& a, double b) {
  RotDual<N> r = a;
  r.v = a.v + b;
  return r;
}
template <int N>
__device__ inline RotDual<N> operator/(const RotDual<N>& a, const RotDual<N>& b) {
  RotDual<N> r;
  r.v = a.v / b.v;
  for (int k = 0; k < N; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) / b.v;
  return r;
}
template <int N>
__device__ inline RotDual<N> rd_chain(const RotDual<N>& a, double f, double df) {
  RotDual<N> r;
  r.v = f;
  for (int k = 0; k < N; ++k) r.d[k] = df * a.d[k];
  return r;
}
template <int N>
__device__ inline RotDual<N> rd_sqrt(const RotDual<N>& a) {
  const double s = sqrt(a.v);
  return rd_chain(a, s, 0.5 / s);
}
template <int N>
__device__ inline RotDual<N> rd_atan2(const RotDual<N>& y, const RotDual<N>& x) {
  RotDual<N> r;
  r.v = atan2(y.v, x.v);
  const double den = x.v * x.v + y.v * y.v;
  for (int k = 0; k < N; ++k) r.d[k] = (x.v * y.d[k] - y.v * x.d[k]) / den;
  return r;
}

template <int N>
static __device__ inline void ceres_angle_axis_to_rotation(const RotDual<N>* aa, RotDual<N>* R) {  // row-major
  typedef RotDual<N> T;
  const T theta2 = aa[0] * aa[0] + aa[1] * aa[1] + aa[2] * aa[2];
  if (theta2.v > DBL_EPSILON) {
    const T theta = rd_sqrt(theta2);
    const T wx = aa[0] / theta, wy = aa[1] / theta, wz = aa[2] / theta;
    const T costheta = rd_chain(theta, cos(theta.v), -sin(theta.v)), sintheta = rd_chain(theta, sin(theta.v), cos(theta.v));
    const T omc = -costheta + 1.0;
    R[0] = costheta + wx * wx * omc;
    R[3] = wz * sintheta + wx * wy * omc;
    R[6] = -(wy * sintheta) + wx * wz * omc;
    R[1] = wx * wy * omc - wz * sintheta;
    R[4] = costheta + wy * wy * omc;
    R[7] = wx * sintheta + wy * wz * omc;
    R[2] = wy * sintheta + wx * wz * omc;
    R[5] = -(wx * sintheta) + wy * wz * omc;
    R[8] = costheta + wz * wz * omc;
  } else {
    const T one = rd_const<N>(1.0);
    R[0] = one; R[3] = aa[2]; R[6] = -aa[1];
    R[1] = -aa[2]; R[4] = one; R[7] = aa[0];
    R[2] = aa[1]; R[5] = -aa[0]; R[8] = one;
  }
}
template <int N>
static __device__ inline void ceres_rotation_to_quaternion(const RotDual<N>* R, RotDual<N>* q) {
  typedef RotDual<N> T;
  const T trace = R[0] + R[4] + R[8];
  if (trace.v >= 0.0) {
    T t = rd_sqrt(trace + 1.0);
    q[0] = t * 0.5;
    t = rd_const<N>(0.5) / t;
    q[1] = (R[7] - R[5]) * t;
    q[2] = (R[2] - R[6]) * t;
    q[3] = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4].v > R[0].v) i = 1;
    if (R[8].v > R[i * 3 + i].v) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    T t = rd_sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    q[i + 1] = t * 0.5;
    t = rd_const<N>(0.5) / t;
    q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    q[j + 1] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    q[k + 1] = (R[k * 3 + i] + R[i * 3 + k]) * t;
  }
}
template <int N>
static __device__ inline void ceres_quaternion_to_angle_axis(const RotDual<N>* q, RotDual<N>* aa) {
  typedef RotDual<N> T;
  const T q1 = q[1], q2 = q[2], q3 = q[3];
  const T sin_squared_theta = q1 * q1 + q2 * q2 + q3 * q3;
  T k = rd_const<N>(2.0);
  if (sin_squared_theta.v > 0.0) {
    const T sin_theta = rd_sqrt(sin_squared_theta);
    const T cos_theta = q[0];
    const T two_theta = (cos_theta.v < 0.0 ? rd_atan2(-sin_theta, -cos_theta) : rd_atan2(sin_theta, cos_theta)) * 2.0;
    k = two_theta / sin_theta;
  }
  aa[0] = q1 * k;
  aa[1] = q2 * k;
  aa[2] = q3 * k;
}

#endif  // DSM_ROTATION_CERES_H_
