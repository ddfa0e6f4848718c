// ba_project.h -- CameraModel::WorldToImage for the eleven camera models (src/base/camera_models.h), generic over the scalar
// so that one body gives both the residual (double) and its derivatives (BaDual: forward-mode dual numbers over u, v and the
// camera parameters).  Restated from the reference's formulas, in the order it writes them; the model table (ids, parameter
// counts, focal indices) is verify_camera.h's.  One runtime switch on the model id, no instantiation per model.
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

#endif  // DAGSFM_AMD_CSRC_BA_PROJECT_H_
