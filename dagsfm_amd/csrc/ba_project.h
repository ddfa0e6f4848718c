// ba_project.h -- CameraModel::WorldToImage for the eleven camera models (src/base/camera_models.h), generic over the scalar
// so that one body gives both the residual (double) and its derivatives (BaDual: forward-mode dual numbers over u, v and the
// camera parameters).  Restated from the reference's formulas, in the order it writes them; the model table (ids, parameter
// counts, focal indices) is verify_camera.h's.  One runtime switch on the model id, no instantiation per model.
// Below it, what the three reprojection solvers (bundle_adjustment.hip, local_bundle.hip, pose_refinement.hip) share around the
// projection: ceres' quaternion rotation and its matrix, QuaternionParameterization::Plus, the projection seeded for its
// derivatives, and the chain from the pixel back to the camera-frame point and the quaternion's tangent.
#ifndef DAGSFM_AMD_CSRC_BA_PROJECT_H_
#define DAGSFM_AMD_CSRC_BA_PROJECT_H_

#include <float.h>
#include <math.h>

#include "verify_camera.h"

#define BA_ND 14  // derivative slots: u, v, up to 12 camera parameters

struct BaDual {
  double v;
  double d[BA_ND];
};

__device__ inline BaDual bd_const(double x) {
  BaDual r;
  r.v = x;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = 0.0;
  return r;
}
__device__ inline BaDual bd_var(double x, int slot) {
  BaDual r = bd_const(x);
  r.d[slot] = 1.0;
  return r;
}
__device__ inline BaDual operator+(const BaDual& a, const BaDual& b) {
  BaDual r;
  r.v = a.v + b.v;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = a.d[i] + b.d[i];
  return r;
}
__device__ inline BaDual operator-(const BaDual& a, const BaDual& b) {
  BaDual r;
  r.v = a.v - b.v;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = a.d[i] - b.d[i];
  return r;
}
__device__ inline BaDual operator-(const BaDual& a) {
  BaDual r;
  r.v = -a.v;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = -a.d[i];
  return r;
}
__device__ inline BaDual operator*(const BaDual& a, const BaDual& b) {
  BaDual r;
  r.v = a.v * b.v;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = a.d[i] * b.v + a.v * b.d[i];
  return r;
}
__device__ inline BaDual operator/(const BaDual& a, const BaDual& b) {
  BaDual r;
  const double inv = 1.0 / b.v;
  r.v = a.v / b.v;  // the value exactly as the double instantiation divides: residuals of both paths are the same bytes
  for (int i = 0; i < BA_ND; ++i) r.d[i] = (a.d[i] - r.v * b.d[i]) * inv;
  return r;
}
__device__ inline BaDual operator+(const BaDual& a, double b) { return a + bd_const(b); }
__device__ inline BaDual operator+(double a, const BaDual& b) { return bd_const(a) + b; }
__device__ inline BaDual operator-(const BaDual& a, double b) { return a - bd_const(b); }
__device__ inline BaDual operator-(double a, const BaDual& b) { return bd_const(a) - b; }
__device__ inline BaDual operator*(double a, const BaDual& b) {
  BaDual r;
  r.v = a * b.v;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = a * b.d[i];
  return r;
}
__device__ inline BaDual operator*(const BaDual& a, double b) { return b * a; }
__device__ inline BaDual operator/(const BaDual& a, double b) { return a / bd_const(b); }
__device__ inline BaDual operator/(double a, const BaDual& b) { return bd_const(a) / b; }
// the chain rule of a scalar function: value f, derivative df
__device__ inline BaDual bd_chain(const BaDual& a, double f, double df) {
  BaDual r;
  r.v = f;
  for (int i = 0; i < BA_ND; ++i) r.d[i] = df * a.d[i];
  return r;
}
__device__ inline BaDual sqrt(const BaDual& a) {
  const double s = ::sqrt(a.v);
  return bd_chain(a, s, 0.5 / s);
}
__device__ inline BaDual atan(const BaDual& a) { return bd_chain(a, ::atan(a.v), 1.0 / (1.0 + a.v * a.v)); }
__device__ inline BaDual tan(const BaDual& a) {
  const double t = ::tan(a.v);
  return bd_chain(a, t, 1.0 + t * t);
}
__device__ inline double ba_val(double x) { return x; }
__device__ inline double ba_val(const BaDual& x) { return x.v; }

// CameraModel::Distortion of the models that add (du, dv) to (u, v)
template <typename T>
__device__ inline void ba_distortion(int id, const T* e, const T& u, const T& v, T* du, T* dv) {
  switch (id) {
    case 2: {  // SIMPLE_RADIAL
      const T r2 = u * u + v * v;
      const T radial = e[0] * r2;
      *du = u * radial;
      *dv = v * radial;
      return;
    }
    case 3: {  // RADIAL
      const T r2 = u * u + v * v;
      const T radial = e[0] * r2 + e[1] * r2 * r2;
      *du = u * radial;
      *dv = v * radial;
      return;
    }
    case 4: {  // OPENCV
      const T u2 = u * u, uv = u * v, v2 = v * v;
      const T r2 = u2 + v2;
      const T radial = e[0] * r2 + e[1] * r2 * r2;
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2);
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2);
      return;
    }
    case 5:    // OPENCV_FISHEYE
    case 8:    // SIMPLE_RADIAL_FISHEYE
    case 9: {  // RADIAL_FISHEYE
      const T r = sqrt(u * u + v * v);
      if (ba_val(r) > DBL_EPSILON) {
        const T theta = atan(r);
        const T theta2 = theta * theta;
        T thetad;
        if (id == 8) {
          thetad = theta * (1.0 + e[0] * theta2);
        } else if (id == 9) {
          const T theta4 = theta2 * theta2;
          thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4);
        } else {
          const T theta4 = theta2 * theta2;
          const T theta6 = theta4 * theta2;
          const T theta8 = theta4 * theta4;
          thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4 + e[2] * theta6 + e[3] * theta8);
        }
        *du = u * thetad / r - u;
        *dv = v * thetad / r - v;
      } else {
        *du = u * 0.0;
        *dv = v * 0.0;
      }
      return;
    }
    case 6: {  // FULL_OPENCV
      const T u2 = u * u, uv = u * v, v2 = v * v;
      const T r2 = u2 + v2;
      const T r4 = r2 * r2;
      const T r6 = r4 * r2;
      const T radial = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6);
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u;
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v;
      return;
    }
    case 10: {  // THIN_PRISM_FISHEYE
      const T u2 = u * u, uv = u * v, v2 = v * v;
      const T r2 = u2 + v2;
      const T r4 = r2 * r2;
      const T r6 = r4 * r2;
      const T r8 = r6 * r2;
      const T radial = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8;
      *du = u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2;
      *dv = v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2;
      return;
    }
    default:
      *du = u * 0.0;
      *dv = v * 0.0;
      return;
  }
}

// CameraModel::WorldToImage(params, u, v, &x, &y)
template <typename T>
__device__ inline void ba_world_to_image(int id, const T* p, T u, T v, T* x, T* y) {
  if (!cam_two_focal(id)) {  // f cx cy [extra]
    T du, dv;
    ba_distortion<T>(id, p + 3, u, v, &du, &dv);
    *x = p[0] * (u + du) + p[1];
    *y = p[0] * (v + dv) + p[2];
    return;
  }
  if (id == 7) {  // FOV: Distortion writes the distorted coordinates themselves
    const T omega = p[4];
    const T radius2 = u * u + v * v;
    const T omega2 = omega * omega;
    T factor;
    if (ba_val(omega2) < 1e-4) {
      factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0;
    } else if (ba_val(radius2) < 1e-4) {
      const T tan_half_omega = tan(omega / 2.0);
      factor = (-2.0 * tan_half_omega * (4.0 * radius2 * tan_half_omega * tan_half_omega - 3.0)) / (3.0 * omega);
    } else {
      const T radius = sqrt(radius2);
      const T numerator = atan(radius * 2.0 * tan(omega / 2.0));
      factor = numerator / (radius * omega);
    }
    *x = p[0] * (u * factor) + p[2];
    *y = p[1] * (v * factor) + p[3];
    return;
  }
  if (id == 10) {  // THIN_PRISM_FISHEYE: onto the equidistant sphere first
    const T r = sqrt(u * u + v * v);
    if (ba_val(r) > DBL_EPSILON) {
      const T theta = atan(r);
      const T uu = theta * u / r, vv = theta * v / r;
      u = uu;
      v = vv;
    }
  }
  T du, dv;
  ba_distortion<T>(id, p + 4, u, v, &du, &dv);
  *x = p[0] * (u + du) + p[2];
  *y = p[1] * (v + dv) + p[3];
}

// ceres::UnitQuaternionRotatePoint (rotation.h)
__device__ inline void ba_rotate(const double* q, const double* X, double* out) {
  const double t2 = q[0] * q[1], t3 = q[0] * q[2], t4 = q[0] * q[3], t5 = -q[1] * q[1], t6 = q[1] * q[2], t7 = q[1] * q[3];
  const double t8 = -q[2] * q[2], t9 = q[2] * q[3], t1 = -q[3] * q[3];
  out[0] = 2.0 * ((t8 + t1) * X[0] + (t6 - t4) * X[1] + (t3 + t7) * X[2]) + X[0];
  out[1] = 2.0 * ((t4 + t6) * X[0] + (t5 + t1) * X[1] + (t9 - t2) * X[2]) + X[1];
  out[2] = 2.0 * ((t7 - t3) * X[0] + (t2 + t9) * X[1] + (t5 + t8) * X[2]) + X[2];
}
// its matrix, row-major.  Not ba_rotate of the unit vectors: that adds the products with the two zero components first and
// rounds differently; local_bundle.hip builds its R that way and keeps doing so.
__device__ inline void ba_quat_R(const double* q, double* R) {
  const double t2 = q[0] * q[1], t3 = q[0] * q[2], t4 = q[0] * q[3], t5 = -q[1] * q[1], t6 = q[1] * q[2], t7 = q[1] * q[3];
  const double t8 = -q[2] * q[2], t9 = q[2] * q[3], t1 = -q[3] * q[3];
  R[0] = 2.0 * (t8 + t1) + 1.0; R[1] = 2.0 * (t6 - t4);       R[2] = 2.0 * (t3 + t7);
  R[3] = 2.0 * (t4 + t6);       R[4] = 2.0 * (t5 + t1) + 1.0; R[5] = 2.0 * (t9 - t2);
  R[6] = 2.0 * (t7 - t3);       R[7] = 2.0 * (t2 + t9);       R[8] = 2.0 * (t5 + t8) + 1.0;
}
// QuaternionParameterization::Plus: [cos|d|, sin|d| d / |d|] (x) x
__device__ inline void ba_quat_plus(const double* x, const double* d, double* out) {
  const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (!(n > 0.0)) {
    for (int i = 0; i < 4; ++i) out[i] = x[i];
    return;
  }
  const double s = sin(n) / n;
  const double a0 = cos(n), a1 = s * d[0], a2 = s * d[1], a3 = s * d[2];
  out[0] = a0 * x[0] - a1 * x[1] - a2 * x[2] - a3 * x[3];
  out[1] = a0 * x[1] + a1 * x[0] + a2 * x[3] - a3 * x[2];
  out[2] = a0 * x[2] - a1 * x[3] + a2 * x[0] + a3 * x[1];
  out[3] = a0 * x[3] + a1 * x[2] - a2 * x[1] + a3 * x[0];
}

// WorldToImage with its derivatives: slots 0 and 1 are u and v, slot 2 + j is camera parameter j (np of them).  The value is
// the double instantiation's.
__device__ inline void ba_project_dual(int model, int np, const double* prm, double u, double v, BaDual* x, BaDual* y) {
  BaDual pd[BA_ND - 2];
  for (int j = 0; j < BA_ND - 2; ++j) pd[j] = j < np ? bd_var(prm[j], 2 + j) : bd_const(0.0);
  ba_world_to_image<BaDual>(model, pd, bd_var(u, 0), bd_var(v, 1), x, y);
}

// From the pixel (x, y) of ba_project_dual at (u, v) = (P[0], P[1]) / P[2], P = w + tvec, w the rotated point:
// JP = d(x, y) / dP, and Dq = dP / d(delta) = -2 [w]x, the tangent of QuaternionParameterization, row-major.
__device__ inline void ba_pixel_jacobian(const BaDual& x, const BaDual& y, double P0, double P1, double P2, const double* w,
                                         double JP[2][3], double* Dq) {
  const double iz = 1.0 / P2;
  const double duP[3] = {iz, 0.0, -P0 * iz * iz}, dvP[3] = {0.0, iz, -P1 * iz * iz};
  for (int a = 0; a < 3; ++a) {
    JP[0][a] = x.d[0] * duP[a] + x.d[1] * dvP[a];
    JP[1][a] = y.d[0] * duP[a] + y.d[1] * dvP[a];
  }
  Dq[0] = 0.0;         Dq[1] = 2.0 * w[2];  Dq[2] = -2.0 * w[1];
  Dq[3] = -2.0 * w[2]; Dq[4] = 0.0;         Dq[5] = 2.0 * w[0];
  Dq[6] = 2.0 * w[1];  Dq[7] = -2.0 * w[0]; Dq[8] = 0.0;
}

#endif  // DAGSFM_AMD_CSRC_BA_PROJECT_H_
