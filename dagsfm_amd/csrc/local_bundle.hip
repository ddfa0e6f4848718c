// local_bundle.hip -- batched local bundle adjustment: IncrementalMapper::AdjustLocalBundle's BundleAdjuster::Solve()
// (src/sfm/incremental_mapper.cc:562-656, src/optim/bundle_adjustment.cc:258-526) with LocalBundleAdjustment()'s options, for a
// batch of independent problems.  The residual, the parameterisations (ba_project.h) and the trust-region
// rulings (trust_region.h) are DESIGN.md 12's; new here are the robust loss (Ceres' Corrector, first branch), cameras
// constant per camera, and the DENSE_SCHUR branch: the points are eliminated, the reduced camera system S is formed
// explicitly in LDS and factored by an unpivoted Cholesky.
//
// One kernel, k_lb_adjust: a workgroup of 256 threads (four waves) per problem runs the whole Levenberg-Marquardt loop; no host
// round trip, no floating-point atomics.  Every sum has an order that is a function of the problem alone:
//   cost, model_cost_change, norms   thread t adds its observations t, t + 256, ... in order; the xor butterfly 32 .. 1 inside a
//                                    wave; then ((w0 + w1) + w2) + w3
//   E'E, E'r of a point              one thread, the track in canonical order
//   F'F entry (a, b), (F'r)_a        one thread, the observations that carry the columns (its image's or camera's list) in canonical order
//   S entry (a, b), rhs_a            one thread: the scaled F'F entry (+ damping), then the points' W'V^-1 W terms subtracted in
//                                    canonical point order (the workgroup stages 8 points at a time in LDS)
//   Cholesky, triangular solves      right-looking; every entry is updated by one thread, pivot columns ascending
// The host sorts every problem into its canonical order first (points by id, images by content, cameras by first use), which is
// what makes the result independent of the order the caller lists them in.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "ba_project.h"
#include "ctx.h"
#include "trust_region.h"
#include "wave_reduce.h"

namespace {

constexpr int LB_T = 256;     // threads of a workgroup
constexpr int LB_TP = 8;      // points staged per tile (32 threads each)
constexpr int LB_FS = 18;     // f slots of an observation: qvec 3, tvec 3, camera 12
constexpr int LB_ROW = 6 + 2 * LB_FS + 2;  // workspace doubles per observation: E 2 x 3, F 2 x 18, the corrected residual
constexpr int LB_PT = 24;     // workspace doubles per point: E'E 6, E'r 3, scale 3, D 3, V^-1 6, delta 3
constexpr int LB_RMAX = DSM_LOCAL_BUNDLE_MAX_REDUCED_DIM;
constexpr int LB_MARGINS = DSM_LOCAL_BUNDLE_MARGINS;
constexpr int LB_TRACE = DSM_LOCAL_BUNDLE_TRACE_COLUMNS;

// one problem in canonical order; the o* fields are offsets into the batch arrays
struct LbProblem {
  uint32_t n_img, n_cam, n_pt, n_obs, R, n_var_pt;
  uint64_t o_img, o_cam, o_pt, o_obs, o_track, o_G, o_ilist, o_clist;
};

struct LbParams {
  uint32_t B;
  int loss, rs;  // rs: the LDS stride (the largest R of the batch, rounded up to even)
  TrOptions tr;
  double b, c;
  const LbProblem* prob;
  // the batch arrays; the kernel moves every pointer to its problem's first element (LbView)
  const uint32_t* img_cam;
  const int32_t* img_qcol;  // first qvec column or -1
  const int32_t* img_tcol;  // [3] per image, -1 = constant
  double* img_q;            // current state, then the result
  double* img_t;
  double* img_cq;           // the candidate
  double* img_ct;
  const int32_t* cam_model;
  const int32_t* cam_col;   // first column or -1
  const int32_t* cam_k;     // free parameters
  const uint8_t* cam_fr;    // [12] per camera: their indices
  double* cam_prm;          // [12] per camera
  double* cam_cprm;
  double* X;
  double* cX;
  const uint8_t* pt_var;
  const uint32_t* var_pt;   // the variable points in canonical order (n_var_pt per problem, stored at the problem's points)
  const uint32_t* track;    // n_pt + 1 per problem, local
  const uint32_t* obs_img;
  const uint32_t* obs_pt;
  const double* obs_xy;
  const uint32_t* img_list;  // n_img + 1 offsets per problem, then img_obs: every image's observations in canonical order
  const uint32_t* img_obs;
  const uint32_t* cam_list;  // the same per camera
  const uint32_t* cam_obs;
  double* wo;               // [LB_ROW][n_obs] per problem: the observations' corrected rows
  double* wp;               // [LB_PT][n_pt] per problem
  double* G;                // R (R + 1) / 2 per problem, packed by columns: (a, b), a <= b, at b (b + 1) / 2 + a
  dsm_local_bundle_result* res;
  double* margins;  // [B][LB_MARGINS]
  double* trace;    // [B][tr.max_iterations + 1][LB_TRACE]
};

struct LbCtrl : TrState {
  double cand_cost, err, cand_err, mcc, s2, x2;
  double m_pivot, m_point;  // the smallest pivot of S, and of a point's block, relative to its diagonal entry
  int valid, ok;
};

// one problem as the device functions see it: the batch pointers moved to the problem, its sizes, the LDS arrays
struct LbView : LbParams {
  int n_img, n_cam, n_pt, n_obs, n_var, R;
  double* S;
  double* W;
  double* Z;
  double *g, *gs, *s, *D, *rhs, *delta, *diag;
  double* ge;
  double* red;
  unsigned long long* mask;
  int* colinfo;  // owner << 6 | slot << 1 | kind (0: the image's pose, 1: the camera)
};

__device__ inline int lb_idx(int a, int b) { return b * (b + 1) / 2 + a; }  // a <= b

// one copy each of the projection's dual instantiation and of Plus in this file's code (the library's size cap)
__device__ __noinline__ void lb_project(int model, int np, const double* prm, double u, double v, BaDual* x, BaDual* y) {
  ba_project_dual(model, np, prm, u, v, x, y);
}
__device__ __noinline__ void lb_quat_plus(const double* x, const double* d, double* out) { ba_quat_plus(x, d, out); }

// the workgroup's fixed-order sum / max / min (every thread returns it).  op 0: sum, 1: max, 2: min
__device__ __noinline__ double lb_reduce(double v, double* red, int tid, int op) {
  v = wave_reduce(v, [op](double a, double w) { return op == 0 ? a + w : (op == 1 ? fmax(a, w) : fmin(a, w)); });
  __syncthreads();
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (op == 0) return ((red[0] + red[1]) + red[2]) + red[3];
  if (op == 1) return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  return fmin(fmin(red[0], red[1]), fmin(red[2], red[3]));
}

// the column of f slot sl of an observation in image i (-1: constant)
__device__ inline int lb_col(const LbView& v, int i, int sl) {
  if (sl < 3) {
    const int qc = v.img_qcol[i];
    return qc < 0 ? -1 : qc + sl;
  }
  if (sl < 6) return v.img_tcol[3 * i + sl - 3];
  const int c = (int)v.img_cam[i];
  const int cc = v.cam_col[c];
  return (cc >= 0 && sl - 6 < v.cam_k[c]) ? cc + sl - 6 : -1;
}

// Per thread: the partial sums of 1/2 rho(|r|^2) and of |r| over the thread's observations of the state (cand: the
// candidate); with jac the corrected rows go to the workspace.  Corrector (ceres/internal/corrector.cc): SoftLOneLoss and
// CauchyLoss have rho'' < 0, so its first branch holds: residual and Jacobian rows are scaled by sqrt(rho').
__device__ __noinline__ void lb_eval(const LbView& v, bool cand, bool jac, int tid, double* cost_out, double* err_out) {
  const double* Q = cand ? v.img_cq : v.img_q;
  const double* T = cand ? v.img_ct : v.img_t;
  const double* XX = cand ? v.cX : v.X;
  const double* PR = cand ? v.cam_cprm : v.cam_prm;
  const size_t N = (size_t)v.n_obs;
  double acc = 0.0, err = 0.0;
  for (int o = tid; o < v.n_obs; o += LB_T) {
    const int i = (int)v.obs_img[o], p = (int)v.obs_pt[o], c = (int)v.img_cam[i];
    const int model = v.cam_model[c], np = cam_num_params(model);
    double q[4], X[3], prm[12], w[3];
    for (int a = 0; a < 4; ++a) q[a] = Q[4 * (size_t)i + a];
    for (int a = 0; a < 3; ++a) X[a] = XX[3 * (size_t)p + a];
    for (int a = 0; a < 12; ++a) prm[a] = PR[12 * (size_t)c + a];
    ba_rotate(q, X, w);
    const double P0 = w[0] + T[3 * (size_t)i], P1 = w[1] + T[3 * (size_t)i + 1], P2 = w[2] + T[3 * (size_t)i + 2];
    const double pu = P0 / P2, pv = P1 / P2;
    BaDual xx, yy;
    lb_project(model, np, prm, pu, pv, &xx, &yy);
    const double r0 = xx.v - v.obs_xy[2 * (size_t)o], r1 = yy.v - v.obs_xy[2 * (size_t)o + 1];
    const double s = r0 * r0 + r1 * r1;
    double rho = s, rho1 = 1.0;
    if (v.loss == DSM_LOSS_SOFT_L1) {  // SoftLOneLoss::Evaluate
      const double sum = 1.0 + s * v.c;
      const double tmp = sqrt(sum);
      rho = 2.0 * v.b * (tmp - 1.0);
      rho1 = fmax(DBL_MIN, 1.0 / tmp);
    } else if (v.loss == DSM_LOSS_CAUCHY) {  // CauchyLoss::Evaluate
      const double sum = 1.0 + s * v.c;
      const double inv = 1.0 / sum;
      rho = v.b * log(sum);
      rho1 = fmax(DBL_MIN, inv);
    }
    acc += 0.5 * rho;
    err += sqrt(s);
    if (!jac) continue;
    const double sq = v.loss == DSM_LOSS_TRIVIAL ? 1.0 : sqrt(rho1);
    double JP[2][3], Dq[9];
    ba_pixel_jacobian(xx, yy, P0, P1, P2, w, JP, Dq);
    // dP / dX = R, column a = R e_a (not ba_quat_R: the rotated unit vectors round differently, and these are the bytes)
    double Rm[9];
    for (int a = 0; a < 3; ++a) {
      const double e[3] = {a == 0 ? 1.0 : 0.0, a == 1 ? 1.0 : 0.0, a == 2 ? 1.0 : 0.0};
      double col[3];
      ba_rotate(q, e, col);
      Rm[a] = col[0];
      Rm[3 + a] = col[1];
      Rm[6 + a] = col[2];
    }
    double* row = v.wo + o;
    const int k = v.cam_k[c];
    const uint8_t* fr = v.cam_fr + 12 * (size_t)c;
    for (int r = 0; r < 2; ++r) {
      const BaDual& dd = r ? yy : xx;
      for (int a = 0; a < 3; ++a) {
        row[(size_t)(r * 3 + a) * N] = sq * (JP[r][0] * Rm[a] + JP[r][1] * Rm[3 + a] + JP[r][2] * Rm[6 + a]);
        row[(size_t)(6 + r * LB_FS + a) * N] = sq * (JP[r][0] * Dq[a] + JP[r][1] * Dq[3 + a] + JP[r][2] * Dq[6 + a]);
        row[(size_t)(6 + r * LB_FS + 3 + a) * N] = sq * JP[r][a];
      }
      for (int j = 0; j < 12; ++j) {
        double dj = 0.0;
        if (j < k) dj = dd.d[2 + fr[j]];
        row[(size_t)(6 + r * LB_FS + 6 + j) * N] = sq * dj;
      }
    }
    row[(size_t)(LB_ROW - 2) * N] = sq * r0;
    row[(size_t)(LB_ROW - 1) * N] = sq * r1;
  }
  *cost_out = acc;
  *err_out = err;
}

// after lb_eval(jac): per variable point E'E and E'r (the track in order); per S entry F'F and per column F'r (the
// observations in order); the Jacobi scaling from the first Jacobian; D; the gradient max-norm.  Ends with the group in step.
__device__ __noinline__ void lb_normal(const LbView& v, LbCtrl* ct, int tid, bool first) {
  const size_t N = (size_t)v.n_obs, NP = (size_t)v.n_pt;
  const int R = v.R;
  for (int p = tid; p < v.n_pt; p += LB_T) {
    if (!v.pt_var[p]) continue;
    double a00 = 0, a10 = 0, a11 = 0, a20 = 0, a21 = 0, a22 = 0, g0 = 0, g1 = 0, g2 = 0;
    for (uint32_t o = v.track[p]; o < v.track[p + 1]; ++o) {
      const double* row = v.wo + o;
      const double e00 = row[0], e01 = row[N], e02 = row[2 * N], e10 = row[3 * N], e11 = row[4 * N], e12 = row[5 * N];
      const double r0 = row[(size_t)(LB_ROW - 2) * N], r1 = row[(size_t)(LB_ROW - 1) * N];
      a00 += e00 * e00 + e10 * e10;
      a10 += e01 * e00 + e11 * e10;
      a11 += e01 * e01 + e11 * e11;
      a20 += e02 * e00 + e12 * e10;
      a21 += e02 * e01 + e12 * e11;
      a22 += e02 * e02 + e12 * e12;
      g0 += e00 * r0 + e10 * r1;
      g1 += e01 * r0 + e11 * r1;
      g2 += e02 * r0 + e12 * r1;
    }
    double* w = v.wp + p;
    w[0] = a00; w[NP] = a10; w[2 * NP] = a11; w[3 * NP] = a20; w[4 * NP] = a21; w[5 * NP] = a22;
    w[6 * NP] = g0; w[7 * NP] = g1; w[8 * NP] = g2;
    const double cn[3] = {a00, a11, a22};
    for (int c = 0; c < 3; ++c) {
      if (first) w[(9 + c) * NP] = 1.0 / (1.0 + sqrt(cn[c]));
      const double se = w[(9 + c) * NP];
      w[(12 + c) * NP] = fmin(fmax((se * se) * cn[c], kLmMinDiag), kLmMaxDiag);
    }
  }
  // F'F entry (a, b): the observations that carry both columns, in canonical order -- those of a's image when a is a pose
  // column, of b's image when b is, of the camera when both are camera columns (the list's order is the canonical one)
  const int ti = tid & 15, tj = tid >> 4;
  for (int a = ti; a < R; a += 16) {
    const int ia = v.colinfo[a], ka = ia & 1, sa = (ia >> 1) & 31, oa = ia >> 6;
    for (int b = a + ((tj - a) & 15); b < R; b += 16) {
      const int ib = v.colinfo[b], kb = ib & 1, sb = (ib >> 1) & 31, ob = ib >> 6;
      double acc = 0.0;
      // two poses or two cameras that differ never share an observation
      if (!(ka == kb && oa != ob)) {
        const bool by_img = !ka || !kb;
        const int own = !ka ? oa : ob;
        const uint32_t* list = by_img ? v.img_list : v.cam_list;
        const uint32_t* lobs = by_img ? v.img_obs : v.cam_obs;
        for (uint32_t x = list[own]; x < list[own + 1]; ++x) {
          const int o = (int)lobs[x], i = (int)v.obs_img[o];
          if ((ka ? (int)v.img_cam[i] : i) != oa) continue;
          if ((kb ? (int)v.img_cam[i] : i) != ob) continue;
          const double* row = v.wo + o;
          acc += row[(size_t)(6 + sa) * N] * row[(size_t)(6 + sb) * N] + row[(size_t)(6 + LB_FS + sa) * N] * row[(size_t)(6 + LB_FS + sb) * N];
        }
      }
      v.G[lb_idx(a, b)] = acc;
    }
  }
  for (int a = tid; a < R; a += LB_T) {
    const int ia = v.colinfo[a], ka = ia & 1, sa = (ia >> 1) & 31, oa = ia >> 6;
    const uint32_t* list = ka ? v.cam_list : v.img_list;
    const uint32_t* lobs = ka ? v.cam_obs : v.img_obs;
    double acc = 0.0;
    for (uint32_t x = list[oa]; x < list[oa + 1]; ++x) {
      const double* row = v.wo + lobs[x];
      acc += row[(size_t)(6 + sa) * N] * row[(size_t)(LB_ROW - 2) * N] + row[(size_t)(6 + LB_FS + sa) * N] * row[(size_t)(LB_ROW - 1) * N];
    }
    v.g[a] = acc;
  }
  __syncthreads();
  for (int a = tid; a < R; a += LB_T) {
    const double cn = v.G[lb_idx(a, a)];
    if (first) v.s[a] = 1.0 / (1.0 + sqrt(cn));
    v.gs[a] = v.s[a] * v.g[a];
    v.D[a] = fmin(fmax((v.s[a] * v.s[a]) * cn, kLmMinDiag), kLmMaxDiag);
  }
  // |x - Plus(x, -g)|inf over the variable blocks, g unscaled
  double m = 0.0;
  for (int p = tid; p < v.n_pt; p += LB_T) {
    if (!v.pt_var[p]) continue;
    for (int c = 0; c < 3; ++c) {
      const double x = v.X[3 * (size_t)p + c];
      m = fmax(m, fabs(x - (x - v.wp[(6 + c) * NP + p])));
    }
  }
  for (int i = tid; i < v.n_img; i += LB_T) {
    const int qc = v.img_qcol[i];
    if (qc < 0) continue;
    const double ng[3] = {-v.g[qc], -v.g[qc + 1], -v.g[qc + 2]};
    double qp[4];
    lb_quat_plus(v.img_q + 4 * (size_t)i, ng, qp);
    for (int a = 0; a < 4; ++a) m = fmax(m, fabs(v.img_q[4 * (size_t)i + a] - qp[a]));
    for (int a = 0; a < 3; ++a) {
      const int tc = v.img_tcol[3 * i + a];
      if (tc < 0) continue;
      const double x = v.img_t[3 * (size_t)i + a];
      m = fmax(m, fabs(x - (x - v.g[tc])));
    }
  }
  for (int c = tid; c < v.n_cam; c += LB_T) {
    const int cc = v.cam_col[c];
    if (cc < 0) continue;
    for (int j = 0; j < v.cam_k[c]; ++j) {
      const double x = v.cam_prm[12 * (size_t)c + v.cam_fr[12 * (size_t)c + j]];
      m = fmax(m, fabs(x - (x - v.g[cc + j])));
    }
  }
  m = lb_reduce(m, v.red, tid, 1);
  if (tid == 0) ct->gnorm = m;
  __syncthreads();
}

// The step of one iteration: V^-1 per point, S and its right-hand side, the Cholesky factor, the two triangular solves, the
// points' back-substitution, model_cost_change, the candidate.  Leaves ct->valid.
__device__ __noinline__ void lb_step(const LbView& v, LbCtrl* ct, int tid) {
  const size_t N = (size_t)v.n_obs, NP = (size_t)v.n_pt;
  const int R = v.R, rs = v.rs;
  const double radius = ct->radius;
  // V = s E'E s + (sqrt(D / radius))^2 by LDL'; a pivot that is not positive and finite makes the step invalid
  double pm = INFINITY;
  int bad = 0;
  for (int p = tid; p < v.n_pt; p += LB_T) {
    if (!v.pt_var[p]) continue;
    double* w = v.wp + p;
    const double s0 = w[9 * NP], s1 = w[10 * NP], s2 = w[11 * NP];
    const double l0 = sqrt(w[12 * NP] / radius), l1 = sqrt(w[13 * NP] / radius), l2 = sqrt(w[14 * NP] / radius);
    const double v00 = (s0 * w[0]) * s0 + l0 * l0, v10 = (s1 * w[NP]) * s0, v11 = (s1 * w[2 * NP]) * s1 + l1 * l1;
    const double v20 = (s2 * w[3 * NP]) * s0, v21 = (s2 * w[4 * NP]) * s1, v22 = (s2 * w[5 * NP]) * s2 + l2 * l2;
    const double d0 = v00;
    const double m10 = v10 / d0, m20 = v20 / d0;
    const double d1 = v11 - m10 * v10;
    const double m21 = (v21 - m20 * v10) / d1;
    const double d2 = (v22 - m20 * v20) - m21 * (m21 * d1);
    const double dd[3] = {d0, d1, d2}, vd[3] = {v00, v11, v22};
    for (int c = 0; c < 3; ++c) {
      pm = fmin(pm, isfinite(dd[c]) && vd[c] > 0.0 ? fabs(dd[c]) / vd[c] : 0.0);
      if (!(dd[c] > 0.0) || !isfinite(dd[c])) bad = 1;
    }
    // V^-1 = M' diag(1 / d) M with M = L^-1
    const double n20 = m10 * m21 - m20;
    const double i0 = 1.0 / d0, i1 = 1.0 / d1, i2 = 1.0 / d2;
    w[15 * NP] = (i0 + (m10 * m10) * i1) + (n20 * n20) * i2;  // 00
    w[16 * NP] = -m10 * i1 - (n20 * m21) * i2;                // 10
    w[17 * NP] = i1 + (m21 * m21) * i2;                       // 11
    w[18 * NP] = n20 * i2;                                    // 20
    w[19 * NP] = -m21 * i2;                                   // 21
    w[20 * NP] = i2;                                          // 22
  }
  pm = lb_reduce(pm, v.red, tid, 2);
  const double anybad = lb_reduce((double)bad, v.red, tid, 1);
  // S = s F'F s + (sqrt(D / radius))^2, rhs = -gs
  const int ti = tid & 15, tj = tid >> 4;
  for (int a = ti; a < R; a += 16)
    for (int b = a + ((tj - a) & 15); b < R; b += 16) {
      double x = (v.s[a] * v.G[lb_idx(a, b)]) * v.s[b];
      if (a == b) {
        const double l = sqrt(v.D[a] / radius);
        x += l * l;
      }
      v.S[lb_idx(a, b)] = x;
    }
  for (int a = tid; a < R; a += LB_T) v.rhs[a] = -v.gs[a];
  if (tid == 0) {
    ct->valid = 0;
    ct->mcc = 0.0;
    ct->ok = anybad == 0.0;
    tr_min(&ct->m_point, pm);
  }
  __syncthreads();
  if (anybad != 0.0) return;
  // the points, eight at a time: W = s_e E'F s_f and Z = V^-1 W staged dense in LDS, then every S entry's owner subtracts
  const int grp = tid >> 5, l = tid & 31;
  if (R > 0) {
    for (int p0 = 0; p0 < v.n_var; p0 += LB_TP) {  // the variable points in canonical order
      const bool act = p0 + grp < v.n_var;
      const int p = act ? (int)v.var_pt[p0 + grp] : 0;
      double* Wp = v.W + (size_t)grp * 3 * rs;
      double* Zp = v.Z + (size_t)grp * 3 * rs;
      if (act) {
        for (int x = l; x < 3 * rs; x += 32) Wp[x] = 0.0;
        if (l < 3) v.ge[grp * 3 + l] = v.wp[(9 + l) * NP + p] * v.wp[(6 + l) * NP + p];
      }
      if (l == 0) {
        unsigned long long m0 = 0, m1 = 0;
        if (act)
          for (uint32_t o = v.track[p]; o < v.track[p + 1]; ++o)
            for (int sl = 0; sl < LB_FS; ++sl) {
              const int col = lb_col(v, (int)v.obs_img[o], sl);
              if (col >= 64) m1 |= 1ull << (col - 64);
              else if (col >= 0) m0 |= 1ull << col;
            }
        v.mask[2 * grp] = m0;
        v.mask[2 * grp + 1] = m1;
      }
      __syncthreads();
      if (act && l < LB_FS)
        for (uint32_t o = v.track[p]; o < v.track[p + 1]; ++o) {
          const int col = lb_col(v, (int)v.obs_img[o], l);
          if (col < 0) continue;
          const double* row = v.wo + o;
          const double f0 = row[(size_t)(6 + l) * N], f1 = row[(size_t)(6 + LB_FS + l) * N];
          for (int c = 0; c < 3; ++c) Wp[c * rs + col] += row[(size_t)c * N] * f0 + row[(size_t)(3 + c) * N] * f1;
        }
      __syncthreads();
      if (act) {
        const double* w = v.wp + p;
        const double vi[6] = {w[15 * NP], w[16 * NP], w[17 * NP], w[18 * NP], w[19 * NP], w[20 * NP]};
        const double se[3] = {w[9 * NP], w[10 * NP], w[11 * NP]};
        for (int col = l; col < R; col += 32) {
          const double w0 = (se[0] * Wp[col]) * v.s[col], w1 = (se[1] * Wp[rs + col]) * v.s[col], w2 = (se[2] * Wp[2 * rs + col]) * v.s[col];
          Wp[col] = w0;
          Wp[rs + col] = w1;
          Wp[2 * rs + col] = w2;
          Zp[col] = (vi[0] * w0 + vi[1] * w1) + vi[3] * w2;
          Zp[rs + col] = (vi[1] * w0 + vi[2] * w1) + vi[4] * w2;
          Zp[2 * rs + col] = (vi[3] * w0 + vi[4] * w1) + vi[5] * w2;
        }
      }
      __syncthreads();
      const int np = min(LB_TP, v.n_var - p0);
      for (int a = ti; a < R; a += 16)
        for (int b = a + ((tj - a) & 15); b < R; b += 16) {
          double x = v.S[lb_idx(a, b)];
          for (int gI = 0; gI < np; ++gI) {
            const unsigned long long ma = a < 64 ? v.mask[2 * gI] >> a : v.mask[2 * gI + 1] >> (a - 64);
            const unsigned long long mb = b < 64 ? v.mask[2 * gI] >> b : v.mask[2 * gI + 1] >> (b - 64);
            if (!(ma & mb & 1ull)) continue;
            const double* Wg = v.W + (size_t)gI * 3 * rs;
            const double* Zg = v.Z + (size_t)gI * 3 * rs;
            x -= (Wg[a] * Zg[b] + Wg[rs + a] * Zg[rs + b]) + Wg[2 * rs + a] * Zg[2 * rs + b];
          }
          v.S[lb_idx(a, b)] = x;
        }
      for (int a = tid; a < R; a += LB_T) {
        double x = v.rhs[a];
        for (int gI = 0; gI < np; ++gI) {
          const unsigned long long ma = a < 64 ? v.mask[2 * gI] >> a : v.mask[2 * gI + 1] >> (a - 64);
          if (!(ma & 1ull)) continue;
          const double* Zg = v.Z + (size_t)gI * 3 * rs;
          x += (Zg[a] * v.ge[3 * gI] + Zg[rs + a] * v.ge[3 * gI + 1]) + Zg[2 * rs + a] * v.ge[3 * gI + 2];
        }
        v.rhs[a] = x;
      }
      __syncthreads();
    }
  }
  // S = U'U in place (right-looking), U' w = rhs, U x = w
  for (int a = tid; a < R; a += LB_T) v.diag[a] = v.S[lb_idx(a, a)];
  __syncthreads();
  for (int j = 0; j < R; ++j) {
    const double pv = v.S[lb_idx(j, j)];
    const bool okp = pv > 0.0 && isfinite(pv);
    if (tid == 0) {
      const double mg = isfinite(pv) && v.diag[j] > 0.0 ? fabs(pv) / v.diag[j] : 0.0;
      tr_min(&ct->m_pivot, mg);
      if (!okp) ct->ok = 0;
    }
    if (!okp) break;  // uniform: every thread read the same pivot
    __syncthreads();
    const double u = sqrt(pv);
    if (tid == 0) v.S[lb_idx(j, j)] = u;
    for (int b = j + 1 + tid; b < R; b += LB_T) v.S[lb_idx(j, b)] /= u;
    __syncthreads();
    for (int a = j + 1 + ((ti - j - 1) & 15); a < R; a += 16) {
      const double ua = v.S[lb_idx(j, a)];
      for (int b = a + ((tj - a) & 15); b < R; b += 16) v.S[lb_idx(a, b)] -= ua * v.S[lb_idx(j, b)];
    }
    __syncthreads();
  }
  __syncthreads();
  if (!ct->ok) return;
  for (int j = 0; j < R; ++j) {
    if (tid == 0) v.rhs[j] = v.rhs[j] / v.S[lb_idx(j, j)];
    __syncthreads();
    const double wj = v.rhs[j];
    for (int i = j + 1 + tid; i < R; i += LB_T) v.rhs[i] -= v.S[lb_idx(j, i)] * wj;
    __syncthreads();
  }
  for (int j = R - 1; j >= 0; --j) {
    if (tid == 0) v.rhs[j] = v.rhs[j] / v.S[lb_idx(j, j)];
    __syncthreads();
    const double xj = v.rhs[j];
    for (int i = tid; i < j; i += LB_T) v.rhs[i] -= v.S[lb_idx(i, j)] * xj;
    __syncthreads();
  }
  // rhs is the scaled step of the f columns; delta = s step
  double s2 = 0.0;
  for (int a = tid; a < R; a += LB_T) {
    v.delta[a] = v.s[a] * v.rhs[a];
    s2 += v.delta[a] * v.delta[a];
  }
  __syncthreads();
  // points: dy = -V^-1 (ge + W dz), W dz from the rows (the track in order)
  for (int p = tid; p < v.n_pt; p += LB_T) {
    if (!v.pt_var[p]) continue;
    double* w = v.wp + p;
    double t0 = 0.0, t1 = 0.0, t2 = 0.0;
    for (uint32_t o = v.track[p]; o < v.track[p + 1]; ++o) {
      const double* row = v.wo + o;
      const int i = (int)v.obs_img[o];
      double f0 = 0.0, f1 = 0.0;
      for (int sl = 0; sl < LB_FS; ++sl) {
        const int col = lb_col(v, i, sl);
        if (col < 0) continue;
        f0 += row[(size_t)(6 + sl) * N] * v.delta[col];
        f1 += row[(size_t)(6 + LB_FS + sl) * N] * v.delta[col];
      }
      t0 += row[0] * f0 + row[3 * N] * f1;
      t1 += row[N] * f0 + row[4 * N] * f1;
      t2 += row[2 * N] * f0 + row[5 * N] * f1;
    }
    const double se[3] = {w[9 * NP], w[10 * NP], w[11 * NP]};
    const double b0 = se[0] * (w[6 * NP] + t0), b1 = se[1] * (w[7 * NP] + t1), b2 = se[2] * (w[8 * NP] + t2);
    const double y0 = -((w[15 * NP] * b0 + w[16 * NP] * b1) + w[18 * NP] * b2);
    const double y1 = -((w[16 * NP] * b0 + w[17 * NP] * b1) + w[19 * NP] * b2);
    const double y2 = -((w[18 * NP] * b0 + w[19 * NP] * b1) + w[20 * NP] * b2);
    const double d0 = se[0] * y0, d1 = se[1] * y1, d2 = se[2] * y2;
    w[21 * NP] = d0;
    w[22 * NP] = d1;
    w[23 * NP] = d2;
    s2 += (d0 * d0 + d1 * d1) + d2 * d2;
  }
  s2 = lb_reduce(s2, v.red, tid, 0);
  // model_cost_change = -(J delta)'(r + J delta / 2) over the corrected rows
  double mc = 0.0;
  for (int o = tid; o < v.n_obs; o += LB_T) {
    const double* row = v.wo + o;
    const int i = (int)v.obs_img[o], p = (int)v.obs_pt[o];
    double j0 = 0.0, j1 = 0.0;
    if (v.pt_var[p])
      for (int c = 0; c < 3; ++c) {
        const double d = v.wp[(21 + c) * NP + p];
        j0 += row[(size_t)c * N] * d;
        j1 += row[(size_t)(3 + c) * N] * d;
      }
    for (int sl = 0; sl < LB_FS; ++sl) {
      const int col = lb_col(v, i, sl);
      if (col < 0) continue;
      j0 += row[(size_t)(6 + sl) * N] * v.delta[col];
      j1 += row[(size_t)(6 + LB_FS + sl) * N] * v.delta[col];
    }
    mc += j0 * (row[(size_t)(LB_ROW - 2) * N] + j0 / 2.0) + j1 * (row[(size_t)(LB_ROW - 1) * N] + j1 / 2.0);
  }
  mc = lb_reduce(mc, v.red, tid, 0);
  // |x|^2 over the variable blocks (the parameter tolerance) and the candidate
  double x2 = 0.0;
  for (int p = tid; p < v.n_pt; p += LB_T)
    for (int c = 0; c < 3; ++c) {
      const double x = v.X[3 * (size_t)p + c];
      if (v.pt_var[p]) {
        x2 += x * x;
        v.cX[3 * (size_t)p + c] = x + v.wp[(21 + c) * NP + p];
      } else {
        v.cX[3 * (size_t)p + c] = x;
      }
    }
  for (int i = tid; i < v.n_img; i += LB_T) {
    const int qc = v.img_qcol[i];
    const double* q = v.img_q + 4 * (size_t)i;
    const double* t = v.img_t + 3 * (size_t)i;
    double* cq = v.img_cq + 4 * (size_t)i;
    double* ctv = v.img_ct + 3 * (size_t)i;
    for (int a = 0; a < 4; ++a) cq[a] = q[a];
    for (int a = 0; a < 3; ++a) ctv[a] = t[a];
    if (qc < 0) continue;
    const double d[3] = {v.delta[qc], v.delta[qc + 1], v.delta[qc + 2]};
    lb_quat_plus(q, d, cq);
    for (int a = 0; a < 4; ++a) x2 += q[a] * q[a];
    for (int a = 0; a < 3; ++a) {
      x2 += t[a] * t[a];
      const int tc = v.img_tcol[3 * i + a];
      if (tc >= 0) ctv[a] = t[a] + v.delta[tc];
    }
  }
  for (int c = tid; c < v.n_cam; c += LB_T) {
    const int cc = v.cam_col[c];
    for (int j = 0; j < 12; ++j) v.cam_cprm[12 * (size_t)c + j] = v.cam_prm[12 * (size_t)c + j];
    if (cc < 0) continue;
    const int np = cam_num_params(v.cam_model[c]);
    for (int j = 0; j < np; ++j) x2 += v.cam_prm[12 * (size_t)c + j] * v.cam_prm[12 * (size_t)c + j];
    for (int j = 0; j < v.cam_k[c]; ++j) {
      const int f = v.cam_fr[12 * (size_t)c + j];
      v.cam_cprm[12 * (size_t)c + f] = v.cam_prm[12 * (size_t)c + f] + v.delta[cc + j];
    }
  }
  x2 = lb_reduce(x2, v.red, tid, 0);
  if (tid == 0) {
    ct->mcc = -mc;
    ct->s2 = s2;
    ct->x2 = x2;
    ct->valid = tr_step_usable(ct->mcc, s2);
  }
  __syncthreads();
}

// thread 0: the decision of one iteration (trust_region.h); the state itself is committed by the whole group
__device__ __noinline__ void lb_decide(LbCtrl* ct, const TrOptions& o) {
  if (tr_decide(ct, o, ct->valid != 0, ct->cand_cost, ct->mcc, ct->s2, ct->x2) == TR_ACCEPTED) ct->err = ct->cand_err;
}

// thread 0: the checks that end an iteration, then the trace row
__device__ inline void lb_finalize(LbCtrl* ct, const TrOptions& o, bool fresh, double* trace) {
  tr_end_iteration(ct, o, fresh);
  if (trace && ct->iter <= o.max_iterations) {
    double* row = trace + (size_t)ct->iter * LB_TRACE;
    row[0] = ct->cost;
    row[1] = ct->radius;
    row[2] = ct->iter == 0 ? NAN : ct->last_rho;
    row[3] = ct->iter == 0 ? 1.0 : (double)ct->accepted;
    row[4] = ct->gnorm;
  }
}

__global__ void __launch_bounds__(LB_T) k_lb_adjust(LbParams p) {
  extern __shared__ double lb_lds[];
  const int tid = threadIdx.x;
  const uint32_t b = blockIdx.x;
  if (b >= p.B) return;
  const LbProblem pb = p.prob[b];
  const int rs = p.rs;
  LbView v;
  static_cast<LbParams&>(v) = p;
  v.n_img = (int)pb.n_img; v.n_cam = (int)pb.n_cam; v.n_pt = (int)pb.n_pt; v.n_obs = (int)pb.n_obs; v.n_var = (int)pb.n_var_pt; v.R = (int)pb.R;
  v.img_cam += pb.o_img; v.img_qcol += pb.o_img; v.img_tcol += 3 * pb.o_img;
  v.img_q += 4 * pb.o_img; v.img_t += 3 * pb.o_img; v.img_cq += 4 * pb.o_img; v.img_ct += 3 * pb.o_img;
  v.cam_model += pb.o_cam; v.cam_col += pb.o_cam; v.cam_k += pb.o_cam; v.cam_fr += 12 * pb.o_cam;
  v.cam_prm += 12 * pb.o_cam; v.cam_cprm += 12 * pb.o_cam;
  v.X += 3 * pb.o_pt; v.cX += 3 * pb.o_pt; v.pt_var += pb.o_pt; v.var_pt += pb.o_pt; v.track += pb.o_track;
  v.obs_img += pb.o_obs; v.obs_pt += pb.o_obs; v.obs_xy += 2 * pb.o_obs;
  v.img_list += pb.o_ilist; v.img_obs += pb.o_obs; v.cam_list += pb.o_clist; v.cam_obs += pb.o_obs;
  v.wo += (size_t)LB_ROW * pb.o_obs; v.wp += (size_t)LB_PT * pb.o_pt; v.G += pb.o_G;
  double* at = lb_lds;
  v.S = at; at += rs * (rs + 1) / 2 + 1;
  v.W = at; at += LB_TP * 3 * rs;
  v.Z = at; at += LB_TP * 3 * rs;
  v.g = at; at += rs; v.gs = at; at += rs; v.s = at; at += rs; v.D = at; at += rs;
  v.rhs = at; at += rs; v.delta = at; at += rs; v.diag = at; at += rs;
  v.ge = at; at += LB_TP * 3;
  v.red = at; at += 4;
  v.mask = reinterpret_cast<unsigned long long*>(at); at += 2 * LB_TP;
  LbCtrl* ct = reinterpret_cast<LbCtrl*>(at); at += (sizeof(LbCtrl) + 7) / 8;
  v.colinfo = reinterpret_cast<int*>(at);
  double* trace = p.trace ? p.trace + (size_t)b * (size_t)(p.tr.max_iterations + 1) * LB_TRACE : nullptr;
  // the columns' owners: pose columns from the images, camera columns from the cameras
  for (int i = tid; i < v.n_img; i += LB_T) {
    const int qc = v.img_qcol[i];
    if (qc < 0) continue;
    for (int a = 0; a < 3; ++a) {
      v.colinfo[qc + a] = i << 6 | a << 1;
      const int tc = v.img_tcol[3 * i + a];
      if (tc >= 0) v.colinfo[tc] = i << 6 | (3 + a) << 1;
    }
  }
  for (int c = tid; c < v.n_cam; c += LB_T) {
    const int cc = v.cam_col[c];
    if (cc < 0) continue;
    for (int j = 0; j < v.cam_k[c]; ++j) v.colinfo[cc + j] = c << 6 | (6 + j) << 1 | 1;
  }
  if (tid == 0) {
    tr_init(ct, kTrInitialRadius);
    ct->m_pivot = ct->m_point = INFINITY;
    ct->err = 0.0;
  }
  __syncthreads();
  const uint64_t n_eff = 3ull * pb.n_var_pt + pb.R;
  double initial_cost = 0.0, initial_err = 0.0;
  if (v.n_obs > 0) {
    double c0, e0;
    lb_eval(v, false, n_eff > 0, tid, &c0, &e0);
    c0 = lb_reduce(c0, v.red, tid, 0);
    e0 = lb_reduce(e0, v.red, tid, 0);
    initial_cost = c0;
    initial_err = e0;
    if (tid == 0) {
      ct->cost = c0;
      ct->err = e0;
      if (n_eff == 0) ct->done = 1;  // Ceres reduces the problem to an empty program: CONVERGENCE, zero iterations
      if (!isfinite(c0)) tr_finish(ct, TR_FAILURE);
    }
    __syncthreads();
    if (!ct->done) {
      lb_normal(v, ct, tid, true);
      if (tid == 0) lb_finalize(ct, v.tr, true, trace);
    } else if (tid == 0 && trace) {
      trace[0] = c0;
      trace[1] = ct->radius;
      trace[2] = NAN;
      trace[3] = 1.0;
      trace[4] = 0.0;
    }
    __syncthreads();
    while (!ct->done) {  // at most max_iterations rounds: tr_decide counts every one, tr_end_iteration stops at the cap
      lb_step(v, ct, tid);
      double cc = INFINITY, ce = 0.0;
      const bool valid = ct->valid != 0;
      if (valid) {
        lb_eval(v, true, false, tid, &cc, &ce);
        cc = lb_reduce(cc, v.red, tid, 0);
        ce = lb_reduce(ce, v.red, tid, 0);
      }
      if (tid == 0) {
        ct->cand_cost = cc;
        ct->cand_err = ce;
        lb_decide(ct, v.tr);
      }
      __syncthreads();
      const bool acc = ct->accepted != 0;
      const bool fresh = acc && !ct->done;
      if (acc) {  // commit the candidate
        for (int x = tid; x < 3 * v.n_pt; x += LB_T) v.X[x] = v.cX[x];
        for (int x = tid; x < 4 * v.n_img; x += LB_T) v.img_q[x] = v.img_cq[x];
        for (int x = tid; x < 3 * v.n_img; x += LB_T) v.img_t[x] = v.img_ct[x];
        for (int x = tid; x < 12 * v.n_cam; x += LB_T) v.cam_prm[x] = v.cam_cprm[x];
        __syncthreads();
      }
      if (fresh) {
        double c1, e1;
        lb_eval(v, false, true, tid, &c1, &e1);
        __syncthreads();
        lb_normal(v, ct, tid, false);
      }
      if (tid == 0) lb_finalize(ct, v.tr, fresh, trace);
      __syncthreads();
    }
  }
  if (tid == 0) {
    dsm_local_bundle_result* out = &p.res[b];
    out->solved = v.n_obs > 0;
    out->termination = ct->term;
    out->num_iterations = (uint32_t)ct->iter;
    out->num_successful_steps = (uint32_t)ct->n_succ;
    out->num_invalid_steps = (uint32_t)ct->n_invalid_total;
    out->reduced_dim = pb.R;
    out->num_residuals = 2ull * pb.n_obs;
    out->num_effective_parameters = n_eff;
    out->initial_cost = initial_cost;
    out->final_cost = ct->cost;
    out->initial_mean_reprojection_error = v.n_obs ? initial_err / v.n_obs : 0.0;
    out->final_mean_reprojection_error = v.n_obs ? ct->err / v.n_obs : 0.0;
    const double mg[LB_MARGINS] = {ct->m_accept, ct->m_grad, ct->m_pivot, ct->m_point};
    for (int i = 0; i < LB_MARGINS; ++i) p.margins[(size_t)b * LB_MARGINS + i] = mg[i];
  }
}

size_t lb_lds_bytes(int rs) {
  size_t d = (size_t)rs * (rs + 1) / 2 + 1 + 2 * (size_t)LB_TP * 3 * rs + 7 * (size_t)rs + LB_TP * 3 + 4 + 2 * LB_TP + (sizeof(LbCtrl) + 7) / 8;
  return d * 8 + (size_t)rs * 4 + 16;
}

struct LbBufs {
  DevBuf prob, img_cam, img_qcol, img_tcol, img_q, img_t, img_cq, img_ct, cam_model, cam_col, cam_k, cam_fr, cam_prm, cam_cprm, pt_X,
      pt_cX, pt_var, var_pt, track, img_list, img_obs, cam_list, cam_obs, obs_img, obs_pt, obs_xy, ws_obs, ws_pt, ws_G, res, margins, trace;
};

inline uint64_t lb_bits(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return u;
}

}  // namespace

extern "C" void dsm_default_local_bundle_options(dsm_local_bundle_options* o) {
  o->max_num_iterations = 25;                 // ba_local_max_num_iterations, incremental_mapper_controller.h:98 through .cc:240
  o->max_num_consecutive_invalid_steps = 10;  // dsm_bundle_adjustment_options' value
  o->gradient_tolerance = 10.0;               // incremental_mapper_controller.cc:238
  o->function_tolerance = 0.0;                // :237
  o->parameter_tolerance = 0.0;               // :239
  o->refine_focal_length = 1;                 // :248, incremental_mapper_controller.h:90
  o->refine_principal_point = 0;              // :249, .h:91
  o->refine_extra_params = 1;                 // :250, .h:92
  o->loss_function_type = DSM_LOSS_SOFT_L1;   // :252-253
  o->loss_function_scale = 1.0;               // :251
}

extern "C" int dsm_adjust_local_bundles(dsm_ctx* ctx, uint32_t num_problems, const uint32_t* camera_offsets,
                                        const int32_t* camera_model_ids, double* camera_params, const uint8_t* camera_constant,
                                        const uint32_t* image_offsets, const uint32_t* image_camera, double* image_qvec,
                                        double* image_tvec, const uint8_t* image_constant_pose, const uint8_t* image_constant_tvec,
                                        const uint32_t* point_offsets, const uint64_t* point_ids, double* point_xyz,
                                        const uint8_t* point_constant, const uint32_t* track_offsets, const uint64_t* obs_offsets,
                                        const uint32_t* obs_image, const double* obs_xy, const dsm_local_bundle_options* options,
                                        dsm_local_bundle_result* results_out, double* margins_out, double* trace_out,
                                        dsm_local_bundle_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_adjust_local_bundles", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  const uint32_t B = num_problems;
  dsm_local_bundle_options o;
  if (options)
    o = *options;
  else
    dsm_default_local_bundle_options(&o);
  if (o.max_num_iterations < 0 || o.max_num_consecutive_invalid_steps < 0 || !(o.gradient_tolerance >= 0.0) ||
      !std::isfinite(o.gradient_tolerance) || !(o.function_tolerance >= 0.0) || !std::isfinite(o.function_tolerance) ||
      !(o.parameter_tolerance >= 0.0) || !std::isfinite(o.parameter_tolerance))
    return fail("option out of range");
  if (o.max_num_iterations > (int32_t)DSM_LOCAL_BUNDLE_MAX_ITERATIONS)
    return fail("max_num_iterations above 1000: the loop runs inside one launch");
  if (o.loss_function_type != DSM_LOSS_TRIVIAL && o.loss_function_type != DSM_LOSS_SOFT_L1 && o.loss_function_type != DSM_LOSS_CAUCHY)
    return fail("an unknown loss_function_type");
  if (o.loss_function_type != DSM_LOSS_TRIVIAL && !(o.loss_function_scale > 0.0 && std::isfinite(o.loss_function_scale)))
    return fail("loss_function_scale must be positive for a non-trivial loss");
  if (B && (!camera_offsets || !image_offsets || !point_offsets || !obs_offsets || !results_out)) return fail("NULL argument");
  if (B && (camera_offsets[0] || image_offsets[0] || point_offsets[0] || obs_offsets[0])) return fail("offsets must start at 0");
  for (uint32_t b = 0; b < B; ++b)
    if (camera_offsets[b + 1] < camera_offsets[b] || image_offsets[b + 1] < image_offsets[b] || point_offsets[b + 1] < point_offsets[b] ||
        obs_offsets[b + 1] < obs_offsets[b])
      return fail("offsets must ascend");
  const uint64_t TC = B ? camera_offsets[B] : 0, TI = B ? image_offsets[B] : 0, TP = B ? point_offsets[B] : 0, TO = B ? obs_offsets[B] : 0;
  if ((TC && (!camera_model_ids || !camera_params)) || (TI && (!image_camera || !image_qvec || !image_tvec)) ||
      (TP && (!point_ids || !point_xyz)) || (B && !track_offsets) || (TO && (!obs_image || !obs_xy)))
    return fail("NULL argument");
  if (TO >= 0x80000000ull / LB_ROW) return fail("too many observations in one call");
  // where every camera's parameters start
  std::vector<uint64_t> prm_off(TC + 1, 0);
  for (uint64_t c = 0; c < TC; ++c) {
    if (!cam_model_exists(camera_model_ids[c])) return fail("an unknown camera model");
    prm_off[c + 1] = prm_off[c] + (uint64_t)cam_num_params(camera_model_ids[c]);
  }
  for (uint64_t i = 0; i < prm_off[TC]; ++i)
    if (!std::isfinite(camera_params[i])) return fail("non-finite camera parameters");
  for (uint64_t i = 0; i < TI; ++i) {
    double n2 = 0.0;
    for (int a = 0; a < 4; ++a) {
      if (!std::isfinite(image_qvec[4 * i + a])) return fail("non-finite qvec");
      n2 += image_qvec[4 * i + a] * image_qvec[4 * i + a];
    }
    if (!(n2 > 0.0)) return fail("a zero qvec");
    for (int a = 0; a < 3; ++a)
      if (!std::isfinite(image_tvec[3 * i + a])) return fail("non-finite tvec");
    if (image_constant_tvec && image_constant_tvec[i] > 7) return fail("image_constant_tvec above 7");
  }
  for (uint64_t i = 0; i < 3 * TP; ++i)
    if (!std::isfinite(point_xyz[i])) return fail("non-finite point");
  for (uint64_t i = 0; i < 2 * TO; ++i)
    if (!std::isfinite(obs_xy[i])) return fail("non-finite observation");

  // ---- the canonical order of every problem, and the device arrays
  std::vector<LbProblem> prob(B);
  std::vector<uint32_t> h_img_cam, h_track, h_obs_img, h_obs_pt, h_var_pt, h_img_list, h_img_obs, h_cam_list, h_cam_obs;
  std::vector<int32_t> h_qcol, h_tcol, h_cam_model, h_cam_col, h_cam_k;
  std::vector<uint8_t> h_cam_fr, h_pt_var;
  std::vector<double> h_q, h_t, h_prm, h_X, h_xy;
  // where the device's blocks came from (indices into the caller's batch arrays)
  std::vector<uint64_t> src_img, src_cam, src_pt;
  uint64_t G_total = 0;
  int r_max = 0;
  const bool any_refine = o.refine_focal_length || o.refine_principal_point || o.refine_extra_params;
  for (uint32_t b = 0; b < B; ++b) {
    const uint32_t C = camera_offsets[b + 1] - camera_offsets[b], N = image_offsets[b + 1] - image_offsets[b];
    const uint32_t P = point_offsets[b + 1] - point_offsets[b];
    const uint64_t n = obs_offsets[b + 1] - obs_offsets[b];
    const uint64_t c0 = camera_offsets[b], i0 = image_offsets[b], p0 = point_offsets[b], ob0 = obs_offsets[b];
    const uint32_t* toff = track_offsets + p0 + b;
    if (toff[0] != 0) return fail("track_offsets of a problem must start at 0");
    for (uint32_t p = 0; p < P; ++p)
      if (toff[p + 1] < toff[p]) return fail("track_offsets must ascend");
    if (toff[P] != n) return fail("track_offsets do not end at the problem's observation count");
    for (uint32_t i = 0; i < N; ++i)
      if (image_camera[i0 + i] >= C) return fail("image_camera out of range");
    for (uint64_t k = 0; k < n; ++k)
      if (obs_image[ob0 + k] >= N) return fail("obs_image out of range");
    // points by id
    std::vector<uint32_t> porder(P), prank(P);
    std::iota(porder.begin(), porder.end(), 0u);
    std::sort(porder.begin(), porder.end(), [&](uint32_t x, uint32_t y) { return point_ids[p0 + x] < point_ids[p0 + y]; });
    for (uint32_t r = 0; r < P; ++r) {
      if (r && point_ids[p0 + porder[r]] == point_ids[p0 + porder[r - 1]]) return fail("a repeated point id");
      prank[porder[r]] = r;
    }
    // images by content: flags, pose, camera (model, constancy, parameters), then -- only where all of that ties -- the
    // observations by point rank
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> iobs(N);  // (point rank, observation)
    for (uint32_t p = 0; p < P; ++p)
      for (uint32_t k = toff[p]; k < toff[p + 1]; ++k) iobs[obs_image[ob0 + k]].push_back({prank[p], ob0 + k});
    std::vector<uint32_t> iorder;
    for (uint32_t i = 0; i < N; ++i) {
      if (iobs[i].empty()) continue;  // not in the problem
      iorder.push_back(i);
      std::sort(iobs[i].begin(), iobs[i].end());
      for (size_t k = 1; k < iobs[i].size(); ++k)
        if (iobs[i][k].first == iobs[i][k - 1].first) return fail("one image observes one point twice");
    }
    auto head = [&](uint32_t i, uint64_t* ky) {  // 23 words at most
      const uint64_t cam = c0 + image_camera[i0 + i];
      int n = 0;
      ky[n++] = image_constant_pose && image_constant_pose[i0 + i] ? 1 : 0;
      ky[n++] = image_constant_tvec ? image_constant_tvec[i0 + i] : 0;
      for (int a = 0; a < 4; ++a) ky[n++] = lb_bits(image_qvec[4 * (i0 + i) + a]);
      for (int a = 0; a < 3; ++a) ky[n++] = lb_bits(image_tvec[3 * (i0 + i) + a]);
      ky[n++] = (uint64_t)camera_model_ids[cam];
      ky[n++] = camera_constant && camera_constant[cam] ? 1 : 0;
      for (uint64_t j = prm_off[cam]; j < prm_off[cam + 1]; ++j) ky[n++] = lb_bits(camera_params[j]);
      return n;
    };
    std::stable_sort(iorder.begin(), iorder.end(), [&](uint32_t x, uint32_t y) {
      uint64_t kx[24], ky[24];
      const int nx = head(x, kx), ny = head(y, ky);
      if (!std::equal(kx, kx + nx, ky, ky + ny)) return std::lexicographical_compare(kx, kx + nx, ky, ky + ny);
      const auto &ox = iobs[x], &oy = iobs[y];
      for (size_t k = 0; k < ox.size() && k < oy.size(); ++k) {
        const uint64_t wx[3] = {ox[k].first, lb_bits(obs_xy[2 * ox[k].second]), lb_bits(obs_xy[2 * ox[k].second + 1])};
        const uint64_t wy[3] = {oy[k].first, lb_bits(obs_xy[2 * oy[k].second]), lb_bits(obs_xy[2 * oy[k].second + 1])};
        for (int a = 0; a < 3; ++a)
          if (wx[a] != wy[a]) return wx[a] < wy[a];
      }
      return ox.size() < oy.size();
    });
    std::vector<int32_t> inew(N, -1), cnew(C, -1);
    std::vector<uint32_t> corder;
    for (size_t r = 0; r < iorder.size(); ++r) {
      inew[iorder[r]] = (int32_t)r;
      const uint32_t c = image_camera[i0 + iorder[r]];
      if (cnew[c] < 0) {
        cnew[c] = (int32_t)corder.size();
        corder.push_back(c);
      }
    }
    LbProblem& pb = prob[b];
    pb.n_img = (uint32_t)iorder.size();
    pb.n_cam = (uint32_t)corder.size();
    pb.n_obs = (uint32_t)n;
    pb.o_img = h_img_cam.size();
    pb.o_cam = h_cam_model.size();
    pb.o_pt = h_pt_var.size();
    pb.o_obs = h_obs_img.size();
    pb.o_track = h_track.size();
    // columns: per image qvec 3 and the free tvec components, then per camera its free parameters
    int col = 0;
    for (uint32_t r = 0; r < pb.n_img; ++r) {
      const uint64_t i = i0 + iorder[r];
      const bool cp = image_constant_pose && image_constant_pose[i];
      const uint8_t mk = image_constant_tvec ? image_constant_tvec[i] : 0;
      h_img_cam.push_back((uint32_t)cnew[image_camera[i]]);
      src_img.push_back(i);
      double n2 = 0.0;
      for (int a = 0; a < 4; ++a) n2 += image_qvec[4 * i + a] * image_qvec[4 * i + a];
      const double nn = std::sqrt(n2);
      for (int a = 0; a < 4; ++a) h_q.push_back(image_qvec[4 * i + a] / nn);  // NormalizeQvec (bundle_adjustment.cc:345)
      for (int a = 0; a < 3; ++a) h_t.push_back(image_tvec[3 * i + a]);
      h_qcol.push_back(cp ? -1 : col);
      if (!cp) col += 3;
      for (int a = 0; a < 3; ++a) {
        const bool fr = !cp && !((mk >> a) & 1);
        h_tcol.push_back(fr ? col : -1);
        if (fr) ++col;
      }
    }
    for (uint32_t r = 0; r < pb.n_cam; ++r) {
      const uint64_t c = c0 + corder[r];
      const int model = camera_model_ids[c], np = cam_num_params(model), nfoc = cam_two_focal(model) ? 2 : 1;
      src_cam.push_back(c);
      h_cam_model.push_back(model);
      int k = 0;
      uint8_t fr[12] = {0};
      if (any_refine && !(camera_constant && camera_constant[c]))
        for (int j = 0; j < np; ++j) {
          const bool f = j < nfoc ? o.refine_focal_length : (j < nfoc + 2 ? o.refine_principal_point : o.refine_extra_params);
          if (f) fr[k++] = (uint8_t)j;
        }
      h_cam_col.push_back(k ? col : -1);
      h_cam_k.push_back(k);
      col += k;
      for (int j = 0; j < 12; ++j) {
        h_cam_fr.push_back(fr[j]);
        h_prm.push_back(j < np ? camera_params[prm_off[c] + j] : 0.0);
      }
    }
    if (col > LB_RMAX)
      return dsm_invalid(ctx, "dsm_adjust_local_bundles", "the reduced camera system of problem " + std::to_string(b) + " has " + std::to_string(col) +
                         " columns, above DSM_LOCAL_BUNDLE_MAX_REDUCED_DIM = 128: a problem of that size belongs to dsm_bundle_adjust");
    pb.R = (uint32_t)col;
    r_max = std::max(r_max, col);
    pb.o_G = G_total;
    G_total += (uint64_t)col * (col + 1) / 2;
    // points in rank order (those with an observation), every track by canonical image
    uint32_t np_dev = 0, nvar = 0, at = 0;
    for (uint32_t r = 0; r < P; ++r) {
      const uint32_t p = porder[r];
      if (toff[p + 1] == toff[p]) continue;  // not in the problem
      std::vector<std::pair<int32_t, uint64_t>> el;
      for (uint32_t k = toff[p]; k < toff[p + 1]; ++k) el.push_back({inew[obs_image[ob0 + k]], ob0 + k});
      std::sort(el.begin(), el.end());
      h_track.push_back(at);
      for (const auto& e : el) {
        h_obs_img.push_back((uint32_t)e.first);
        h_obs_pt.push_back(np_dev);
        h_xy.push_back(obs_xy[2 * e.second]);
        h_xy.push_back(obs_xy[2 * e.second + 1]);
        ++at;
      }
      const bool var = !(point_constant && point_constant[p0 + p]);
      h_pt_var.push_back(var);
      nvar += var;
      for (int a = 0; a < 3; ++a) h_X.push_back(point_xyz[3 * (p0 + p) + a]);
      src_pt.push_back(p0 + p);
      ++np_dev;
    }
    h_track.push_back(at);
    pb.n_pt = np_dev;
    pb.n_var_pt = nvar;
    // the variable points in order (padded to the problem's points), and every image's and camera's observations in
    // canonical order: what the F'F sums walk
    const size_t pt_base = h_pt_var.size() - np_dev, ob_base = h_obs_img.size() - at;
    for (uint32_t r = 0; r < np_dev; ++r)
      if (h_pt_var[pt_base + r]) h_var_pt.push_back(r);
    h_var_pt.resize(h_pt_var.size(), 0);
    pb.o_ilist = h_img_list.size();
    pb.o_clist = h_cam_list.size();
    std::vector<uint32_t> icnt(pb.n_img + 1, 0), ccnt(pb.n_cam + 1, 0);
    for (uint32_t k = 0; k < at; ++k) {
      const uint32_t i = h_obs_img[ob_base + k];
      ++icnt[i + 1];
      ++ccnt[h_img_cam[pb.o_img + i] + 1];
    }
    for (uint32_t i = 0; i < pb.n_img; ++i) icnt[i + 1] += icnt[i];
    for (uint32_t c = 0; c < pb.n_cam; ++c) ccnt[c + 1] += ccnt[c];
    h_img_list.insert(h_img_list.end(), icnt.begin(), icnt.end());
    h_cam_list.insert(h_cam_list.end(), ccnt.begin(), ccnt.end());
    h_img_obs.resize(ob_base + at);
    h_cam_obs.resize(ob_base + at);
    for (uint32_t k = 0; k < at; ++k) {  // ascending k: every list keeps the canonical order
      const uint32_t i = h_obs_img[ob_base + k], c = h_img_cam[pb.o_img + i];
      h_img_obs[ob_base + icnt[i]++] = k;
      h_cam_obs[ob_base + ccnt[c]++] = k;
    }
  }
  dsm_local_bundle_report rep{};
  rep.num_problems = B;
  rep.num_points = TP;
  rep.num_observations = TO;
  for (int i = 0; i < LB_MARGINS; ++i) rep.min_margin[i] = INFINITY;
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  if (B == 0) {
    if (report) *report = rep;
    return DSM_OK;
  }
  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  LbBufs d;
  DevEvents<4> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  const size_t nI = h_img_cam.size(), nC = h_cam_model.size(), nP = h_pt_var.size(), nO = h_obs_img.size();
  const size_t trace_rows = (size_t)B * (size_t)(o.max_num_iterations + 1);
  HIPCHK(ctx, dev_upload(d.prob, prob.data(), (size_t)B * sizeof(LbProblem), st));
  HIPCHK(ctx, dev_upload(d.img_cam, h_img_cam.data(), nI * 4, st));
  HIPCHK(ctx, dev_upload(d.img_qcol, h_qcol.data(), nI * 4, st));
  HIPCHK(ctx, dev_upload(d.img_tcol, h_tcol.data(), nI * 12, st));
  HIPCHK(ctx, dev_upload(d.img_q, h_q.data(), nI * 32, st));
  HIPCHK(ctx, dev_upload(d.img_t, h_t.data(), nI * 24, st));
  HIPCHK(ctx, dev_upload(d.cam_model, h_cam_model.data(), nC * 4, st));
  HIPCHK(ctx, dev_upload(d.cam_col, h_cam_col.data(), nC * 4, st));
  HIPCHK(ctx, dev_upload(d.cam_k, h_cam_k.data(), nC * 4, st));
  HIPCHK(ctx, dev_upload(d.cam_fr, h_cam_fr.data(), nC * 12, st));
  HIPCHK(ctx, dev_upload(d.cam_prm, h_prm.data(), nC * 96, st));
  HIPCHK(ctx, dev_upload(d.pt_X, h_X.data(), nP * 24, st));
  HIPCHK(ctx, dev_upload(d.pt_var, h_pt_var.data(), nP, st));
  HIPCHK(ctx, dev_upload(d.var_pt, h_var_pt.data(), nP * 4, st));
  HIPCHK(ctx, dev_upload(d.track, h_track.data(), h_track.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.img_list, h_img_list.data(), h_img_list.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.img_obs, h_img_obs.data(), nO * 4, st));
  HIPCHK(ctx, dev_upload(d.cam_list, h_cam_list.data(), h_cam_list.size() * 4, st));
  HIPCHK(ctx, dev_upload(d.cam_obs, h_cam_obs.data(), nO * 4, st));
  HIPCHK(ctx, dev_upload(d.obs_img, h_obs_img.data(), nO * 4, st));
  HIPCHK(ctx, dev_upload(d.obs_pt, h_obs_pt.data(), nO * 4, st));
  HIPCHK(ctx, dev_upload(d.obs_xy, h_xy.data(), nO * 16, st));
  HIPCHK(ctx, d.img_cq.reserve(std::max<size_t>(nI * 32, 16)));
  HIPCHK(ctx, d.img_ct.reserve(std::max<size_t>(nI * 24, 16)));
  HIPCHK(ctx, d.cam_cprm.reserve(std::max<size_t>(nC * 96, 16)));
  HIPCHK(ctx, d.pt_cX.reserve(std::max<size_t>(nP * 24, 16)));
  HIPCHK(ctx, d.ws_obs.reserve(std::max<size_t>(nO, 1) * LB_ROW * 8));
  HIPCHK(ctx, d.ws_pt.reserve(std::max<size_t>(nP, 1) * LB_PT * 8));
  HIPCHK(ctx, d.ws_G.reserve(std::max<size_t>(G_total, 1) * 8));
  HIPCHK(ctx, d.res.reserve((size_t)B * sizeof(dsm_local_bundle_result)));
  HIPCHK(ctx, d.margins.reserve((size_t)B * LB_MARGINS * 8));
  HIPCHK(ctx, d.trace.reserve(trace_rows * LB_TRACE * 8));
  HIPCHK(ctx, hipMemsetAsync(d.trace.p, 0xFF, trace_rows * LB_TRACE * 8, st));  // all ones: NaN
  LbParams prm;
  prm.B = B;
  prm.loss = o.loss_function_type;
  prm.rs = (r_max + 1) & ~1;
  prm.tr = tr_ceres_defaults();
  prm.tr.max_iterations = o.max_num_iterations;
  prm.tr.max_consecutive_invalid_steps = o.max_num_consecutive_invalid_steps;
  prm.tr.gtol = o.gradient_tolerance;
  prm.tr.ftol = o.function_tolerance;
  prm.tr.ptol = o.parameter_tolerance;
  prm.b = o.loss_function_scale * o.loss_function_scale;  // SoftLOneLoss(a) / CauchyLoss(a): b_(a * a), c_(1 / b_)
  prm.c = 1.0 / prm.b;
  prm.prob = d.prob.as<LbProblem>();
  prm.img_cam = d.img_cam.as<uint32_t>();
  prm.img_qcol = d.img_qcol.as<int32_t>();
  prm.img_tcol = d.img_tcol.as<int32_t>();
  prm.img_q = d.img_q.as<double>();
  prm.img_t = d.img_t.as<double>();
  prm.img_cq = d.img_cq.as<double>();
  prm.img_ct = d.img_ct.as<double>();
  prm.cam_model = d.cam_model.as<int32_t>();
  prm.cam_col = d.cam_col.as<int32_t>();
  prm.cam_k = d.cam_k.as<int32_t>();
  prm.cam_fr = d.cam_fr.as<uint8_t>();
  prm.cam_prm = d.cam_prm.as<double>();
  prm.cam_cprm = d.cam_cprm.as<double>();
  prm.X = d.pt_X.as<double>();
  prm.cX = d.pt_cX.as<double>();
  prm.pt_var = d.pt_var.as<uint8_t>();
  prm.var_pt = d.var_pt.as<uint32_t>();
  prm.track = d.track.as<uint32_t>();
  prm.img_list = d.img_list.as<uint32_t>();
  prm.img_obs = d.img_obs.as<uint32_t>();
  prm.cam_list = d.cam_list.as<uint32_t>();
  prm.cam_obs = d.cam_obs.as<uint32_t>();
  prm.obs_img = d.obs_img.as<uint32_t>();
  prm.obs_pt = d.obs_pt.as<uint32_t>();
  prm.obs_xy = d.obs_xy.as<double>();
  prm.wo = d.ws_obs.as<double>();
  prm.wp = d.ws_pt.as<double>();
  prm.G = d.ws_G.as<double>();
  prm.res = d.res.as<dsm_local_bundle_result>();
  prm.margins = d.margins.as<double>();
  prm.trace = d.trace.as<double>();
  const size_t lds = lb_lds_bytes(prm.rs);
  // S alone is 66 KB at 128 columns: above the 64 KB a kernel gets without asking (a gfx950 workgroup may hold 160 KB)
  HIPCHK(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(k_lb_adjust), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  hipLaunchKernelGGL(k_lb_adjust, dim3(B), dim3(LB_T), lds, st, prm);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  std::vector<double> margins((size_t)B * LB_MARGINS), r_q(nI * 4), r_t(nI * 3), r_prm(nC * 12), r_X(nP * 3);
  HIPCHK(ctx, hipMemcpyAsync(results_out, d.res.p, (size_t)B * sizeof(dsm_local_bundle_result), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(margins.data(), d.margins.p, margins.size() * 8, hipMemcpyDeviceToHost, st));
  if (nI) HIPCHK(ctx, hipMemcpyAsync(r_q.data(), d.img_q.p, nI * 32, hipMemcpyDeviceToHost, st));
  if (nI) HIPCHK(ctx, hipMemcpyAsync(r_t.data(), d.img_t.p, nI * 24, hipMemcpyDeviceToHost, st));
  if (nC) HIPCHK(ctx, hipMemcpyAsync(r_prm.data(), d.cam_prm.p, nC * 96, hipMemcpyDeviceToHost, st));
  if (nP) HIPCHK(ctx, hipMemcpyAsync(r_X.data(), d.pt_X.p, nP * 24, hipMemcpyDeviceToHost, st));
  if (trace_out) HIPCHK(ctx, hipMemcpyAsync(trace_out, d.trace.p, trace_rows * LB_TRACE * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  // back to the caller's order: the variable blocks, and the normalised qvecs of the images with residuals.  A problem with
  // no variable block keeps its input bits.
  for (uint32_t b = 0; b < B; ++b) {
    const LbProblem& pb = prob[b];
    rep.num_iterations += results_out[b].num_iterations;
    for (int i = 0; i < LB_MARGINS; ++i) {
      rep.min_margin[i] = std::min(rep.min_margin[i], margins[(size_t)b * LB_MARGINS + i]);
      if (margins_out) margins_out[(size_t)b * LB_MARGINS + i] = margins[(size_t)b * LB_MARGINS + i];
    }
    if (3ull * pb.n_var_pt + pb.R == 0) continue;
    for (uint32_t r = 0; r < pb.n_img; ++r) {
      const uint64_t i = src_img[pb.o_img + r];
      for (int a = 0; a < 4; ++a) image_qvec[4 * i + a] = r_q[4 * (pb.o_img + r) + a];
      if (h_qcol[pb.o_img + r] >= 0)
        for (int a = 0; a < 3; ++a) image_tvec[3 * i + a] = r_t[3 * (pb.o_img + r) + a];
    }
    for (uint32_t r = 0; r < pb.n_cam; ++r) {
      if (h_cam_col[pb.o_cam + r] < 0) continue;
      const uint64_t c = src_cam[pb.o_cam + r];
      for (uint64_t j = prm_off[c]; j < prm_off[c + 1]; ++j) camera_params[j] = r_prm[12 * (pb.o_cam + r) + (j - prm_off[c])];
    }
    for (uint32_t r = 0; r < pb.n_pt; ++r) {
      if (!h_pt_var[pb.o_pt + r]) continue;
      const uint64_t p = src_pt[pb.o_pt + r];
      for (int a = 0; a < 3; ++a) point_xyz[3 * p + a] = r_X[3 * (pb.o_pt + r) + a];
    }
  }
  HIPCHK(ctx, ev.ms(0, 1, &rep.upload_ms));
  HIPCHK(ctx, ev.ms(1, 2, &rep.solve_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rep.download_ms));
  HIPCHK(ctx, ev.ms(0, 3, &rep.device_ms));
  if (report) *report = rep;
  return DSM_OK;
}
