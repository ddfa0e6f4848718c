// bundle_adjustment.hip -- the global bundle adjustment of the merged reconstruction.
//   DistributedMapperController::AdjustGlobalBundle  src/controllers/distributed_mapper_controller.cpp:836-931
//   BundleAdjuster (ITERATIVE_SCHUR + SCHUR_JACOBI)    src/optim/bundle_adjustment.cc:273-284, 330-456
//   BundleAdjustmentCostFunction                      src/base/cost_functions.h:45-85
// Levenberg-Marquardt with Jacobi scaling, the step rules of trust_region.h; each step solves the Schur complement over the
// variable points with a CG preconditioned by the exact diagonal blocks of S, S applied implicitly from the stored
// per-observation Jacobian blocks.
// Canonical order: points by id, the images with observations by content, their cameras by first use (the host relabels
// both; the rest stays off the device), observations image-major by (image, point rank), each track by (camera, image).  Every sum
// walks a segment of that order (one thread per point over its track, one 64-lane block per image over its observations with
// a fixed LDS tree, one block per camera over its images' partial rows), every scalar is a fixed-order sum of per-block
// partials: no floating-point atomics, the same bytes on every run and for every input order.  Loop control stays on the
// device: one LM iteration is enqueued whole (its CG iterations are no-ops past ctl.cg_stop, the Jacobian update is a no-op
// when the step is not accepted) and the host reads BaCtl once per LM iteration.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
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
#include "block_reduce.h"
#include "ctx.h"
#include "trust_region.h"

namespace {

constexpr int BA_B = 256;   // element-wise kernels and scalar finalisation
constexpr int BA_W = 64;    // segment blocks (one wave)
constexpr int BA_JS = 48;   // doubles per observation: r[2] E[2x3] Fq[2x3] Ft[2x3] Fc[2x12]
constexpr int J_R = 0, J_E = 2, J_Q = 8, J_T = 14, J_C = 20;
constexpr int BA_KMAX = 12;
constexpr int BA_ICAM = 12 + 78;  // per image camera partial row: a k-vector and a packed k x k lower triangle
constexpr double kEta = 0.1;
static_assert(TR_CONVERGENCE == DSM_BA_CONVERGENCE && TR_NO_CONVERGENCE == DSM_BA_NO_CONVERGENCE && TR_FAILURE == DSM_BA_FAILURE,
              "trust_region.h's termination codes are the public ones");

struct BaCtl : TrState {  // the LM loop's state (trust_region.h), then this solver's own
  // the running CG solve
  int cg_stop, cg_fail, cg_iters, pad1;  // pad1: the latch of k_ba_finalize
  double rho, beta, alpha, Q0;
  unsigned long long cg_total;
  double reproj, cand_cost, cand_reproj, mcc;
  double m_cg;
};

struct BaDev {
  uint32_t n_obs, n_pts, n_img, n_cam, nf;
  int max_cg;
  TrOptions tr;
  const uint32_t *o_img, *o_pt, *o_run, *img_off, *trk_off, *trk, *cam_img_off, *cam_imgs, *img_cam, *cam_poff, *cam_foff, *cam_moff;
  const double* o_xy;
  const uint8_t *img_cpose, *img_mask, *pt_var;
  const int *cam_model, *cam_np, *cam_k, *cam_free;
  double *q, *t, *X, *prm, *cq, *ct, *cX, *cprm;
  double *J, *y;
  double *ge, *cne, *se, *De, *Cinv, *ve, *zp, *dy;
  double *gf, *cnf, *sf, *Df, *ddf, *Minv, *b, *x, *r, *z, *p, *qv, *tmp, *icam;
  double *Pc, *Pm, *Pg, *Pe, *Pd, *Pq;
  BaCtl* ctl;
  double* trace;
};

__host__ __device__ inline int tri(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// ---------------------------------------------------------------- small dense algebra
__device__ inline bool inv3_sym(const double* A, double* Ai) {  // packed lower triangle in, full 3 x 3 out
  const double a = A[0], b = A[1], c = A[2], d = A[3], e = A[4], f = A[5];  // [a b d; b c e; d e f]
  const double c00 = c * f - e * e, c01 = d * e - b * f, c02 = b * e - c * d;
  const double c11 = a * f - d * d, c12 = b * d - a * e, c22 = a * c - b * b;
  const double det = a * c00 + b * c01 + d * c02;
  const double id = 1.0 / det;
  Ai[0] = c00 * id; Ai[1] = c01 * id; Ai[2] = c02 * id;
  Ai[3] = c01 * id; Ai[4] = c11 * id; Ai[5] = c12 * id;
  Ai[6] = c02 * id; Ai[7] = c12 * id; Ai[8] = c22 * id;
  return isfinite(id);
}
// k x k SPD (packed lower triangle) -> full inverse through the Cholesky factor; the workspace L holds k * k
__device__ inline void inv_spd(const double* A, int k, double* L, double* out) {
  for (int i = 0; i < k; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[tri(i, j)];
      for (int m = 0; m < j; ++m) s -= L[i * k + m] * L[j * k + m];
      L[i * k + j] = (i == j) ? sqrt(s) : s / L[j * k + j];
    }
  for (int c = 0; c < k; ++c) {  // solve L L^T x = e_c
    double w[BA_KMAX];
    for (int i = 0; i < k; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int m = 0; m < i; ++m) s -= L[i * k + m] * w[m];
      w[i] = s / L[i * k + i];
    }
    for (int i = k - 1; i >= 0; --i) {
      double s = w[i];
      for (int m = i + 1; m < k; ++m) s -= L[m * k + i] * w[m];
      w[i] = s / L[i * k + i];
    }
    for (int i = 0; i < k; ++i) out[i * k + c] = w[i];
  }
}

__device__ inline bool cg_gated(const BaCtl* c, int k) { return c->done || k >= c->cg_stop; }

// ---------------------------------------------------------------- residuals and Jacobians
// mode 0: the state (with Jacobian), always; 1: the candidate (residual only), skipped when done; 2: the state after an
// accepted step (with Jacobian).  Partials: cost and the summed |r| per block.
__global__ void __launch_bounds__(BA_B) k_ba_eval(BaDev d, int mode) {
  __shared__ double sh[BA_B];
  const BaCtl* c = d.ctl;
  if ((mode == 1 && c->done) || (mode == 2 && (c->done || !c->accepted))) return;
  const uint32_t o = blockIdx.x * BA_B + threadIdx.x;
  double cost = 0.0, nrm = 0.0;
  if (o < d.n_obs) {
    const uint32_t i = d.o_img[o], pt = d.o_pt[o], cam = d.img_cam[i];
    const bool cand = mode == 1;
    const double* q = (cand ? d.cq : d.q) + 4 * (size_t)i;
    const double* tv = (cand ? d.ct : d.t) + 3 * (size_t)i;
    const double* X = (cand ? d.cX : d.X) + 3 * (size_t)pt;
    const double* prm = (cand ? d.cprm : d.prm) + d.cam_poff[cam];
    const int model = d.cam_model[cam], np = d.cam_np[cam];
    double w[3];
    ba_rotate(q, X, w);
    const double P0 = w[0] + tv[0], P1 = w[1] + tv[1], P2 = w[2] + tv[2];
    const double u = P0 / P2, v = P1 / P2;
    double r0, r1;
    if (mode == 1) {
      double xx, yy;
      ba_world_to_image<double>(model, prm, u, v, &xx, &yy);
      r0 = xx - d.o_xy[2 * (size_t)o];
      r1 = yy - d.o_xy[2 * (size_t)o + 1];
    } else {
      BaDual xx, yy;
      ba_project_dual(model, np, prm, u, v, &xx, &yy);
      r0 = xx.v - d.o_xy[2 * (size_t)o];
      r1 = yy.v - d.o_xy[2 * (size_t)o + 1];
      double* Jo = d.J + (size_t)BA_JS * o;
      Jo[J_R] = r0;
      Jo[J_R + 1] = r1;
      // dP/dX = R; dP/d(delta) = Dq
      double JP[2][3], Dq[9], R[9];
      ba_pixel_jacobian(xx, yy, P0, P1, P2, w, JP, Dq);
      ba_quat_R(q, R);
      const bool cpose = d.img_cpose[i];
      const uint8_t mask = d.img_mask[i];
      for (int row = 0; row < 2; ++row)
        for (int a = 0; a < 3; ++a) {
          const double e = d.pt_var[pt] ? JP[row][0] * R[a] + JP[row][1] * R[3 + a] + JP[row][2] * R[6 + a] : 0.0;
          const double fq = cpose ? 0.0 : JP[row][0] * Dq[a] + JP[row][1] * Dq[3 + a] + JP[row][2] * Dq[6 + a];
          const double ft = (cpose || ((mask >> a) & 1)) ? 0.0 : JP[row][a];
          Jo[J_E + 3 * row + a] = e;
          Jo[J_Q + 3 * row + a] = fq;
          Jo[J_T + 3 * row + a] = ft;
        }
      const int k = d.cam_k[cam];
      const int* fr = d.cam_free + BA_KMAX * (size_t)cam;
      for (int j = 0; j < BA_KMAX; ++j) {
        Jo[J_C + j] = j < k ? xx.d[2 + fr[j]] : 0.0;
        Jo[J_C + BA_KMAX + j] = j < k ? yy.d[2 + fr[j]] : 0.0;
      }
    }
    const double s2 = r0 * r0 + r1 * r1;
    cost = 0.5 * s2;
    nrm = sqrt(s2);
  }
  const double a = block_sum<BA_B>(cost, sh), b = block_sum<BA_B>(nrm, sh);
  if (threadIdx.x == 0) {
    d.Pc[blockIdx.x] = a;
    d.Pc[gridDim.x + blockIdx.x] = b;
  }
}

// which 0: the initial state (cost, reproj and the initial report values), 1: the candidate
__global__ void __launch_bounds__(BA_B) k_ba_fin_cost(BaDev d, uint32_t nblk, int which) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (which == 1 && c->done) return;
  const double a = sum_partials<BA_B>(d.Pc, nblk, sh), b = sum_partials<BA_B>(d.Pc + nblk, nblk, sh);
  if (threadIdx.x) return;
  if (which == 0) {
    c->cost = a;
    c->reproj = b / (double)d.n_obs;
  } else {
    c->cand_cost = a;
    c->cand_reproj = b / (double)d.n_obs;
  }
}

// ---------------------------------------------------------------- gradient, column norms, scaling
// per point over its track: g_e = E^T r and the squared column norms (unscaled J); the point's part of |x - Plus(x, -g)|
__global__ void __launch_bounds__(BA_B) k_ba_grad_pts(BaDev d, int gate) {
  __shared__ double sh[BA_B];
  if (gate && (d.ctl->done || !d.ctl->accepted)) return;
  const uint32_t p = blockIdx.x * BA_B + threadIdx.x;
  double gm = 0.0;
  if (p < d.n_pts) {
    double g[3] = {0.0, 0.0, 0.0}, cn[3] = {0.0, 0.0, 0.0};
    if (d.pt_var[p])
      for (uint32_t a = d.trk_off[p]; a < d.trk_off[p + 1]; ++a) {
        const double* Jo = d.J + (size_t)BA_JS * d.trk[a];
        for (int j = 0; j < 3; ++j) {
          g[j] += Jo[J_E + j] * Jo[J_R] + Jo[J_E + 3 + j] * Jo[J_R + 1];
          cn[j] += Jo[J_E + j] * Jo[J_E + j] + Jo[J_E + 3 + j] * Jo[J_E + 3 + j];
        }
      }
    for (int j = 0; j < 3; ++j) {
      d.ge[3 * (size_t)p + j] = g[j];
      d.cne[3 * (size_t)p + j] = cn[j];
      const double x = d.X[3 * (size_t)p + j];
      gm = fmax(gm, fabs(x - (x + -g[j])));
    }
  }
  gm = block_max<BA_B>(gm, sh);
  if (threadIdx.x == 0) d.Pg[blockIdx.x] = gm;
}

// one block per image over its observations: g and squared column norms of qvec / tvec, and the camera's part of the image
// into icam[i] (g_c 0..11, squared norms 12..23)
__global__ void __launch_bounds__(BA_W) k_ba_grad_img(BaDev d, int gate, uint32_t pg_base) {
  __shared__ double sh[36 * BA_W];
  if (gate && (d.ctl->done || !d.ctl->accepted)) return;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const int k = d.cam_k[d.img_cam[i]];
  double* a = sh + t;
  for (int v = 0; v < 36; ++v) a[v * BA_W] = 0.0;
  for (uint32_t o = d.img_off[i] + t; o < d.img_off[i + 1]; o += BA_W) {
    const double* Jo = d.J + (size_t)BA_JS * o;
    const double r0 = Jo[J_R], r1 = Jo[J_R + 1];
    for (int j = 0; j < 6; ++j) {  // q 0..2, t 3..5
      const double f0 = Jo[J_Q + (j / 3) * 6 + j % 3], f1 = Jo[J_Q + (j / 3) * 6 + 3 + j % 3];
      a[j * BA_W] += f0 * r0 + f1 * r1;
      a[(6 + j) * BA_W] += f0 * f0 + f1 * f1;
    }
    for (int j = 0; j < k; ++j) {
      const double f0 = Jo[J_C + j], f1 = Jo[J_C + BA_KMAX + j];
      a[(12 + j) * BA_W] += f0 * r0 + f1 * r1;
      a[(24 + j) * BA_W] += f0 * f0 + f1 * f1;
    }
  }
  __syncthreads();
  block_tree<BA_W>(sh, 36);
  if (t) return;
  double gm = 0.0;
  for (int j = 0; j < 6; ++j) {
    d.gf[6 * (size_t)i + j] = sh[j * BA_W];
    d.cnf[6 * (size_t)i + j] = sh[(6 + j) * BA_W];
  }
  for (int j = 0; j < 24; ++j) d.icam[(size_t)BA_ICAM * i + j] = sh[(12 + j) * BA_W];
  if (!d.img_cpose[i] && d.img_off[i + 1] > d.img_off[i]) {
    const double* q = d.q + 4 * (size_t)i;
    const double mg[3] = {-sh[0], -sh[BA_W], -sh[2 * BA_W]};
    double qp[4];
    ba_quat_plus(q, mg, qp);
    for (int j = 0; j < 4; ++j) gm = fmax(gm, fabs(q[j] - qp[j]));
    for (int j = 0; j < 3; ++j) {
      const double x = d.t[3 * (size_t)i + j];
      gm = fmax(gm, fabs(x - (x + -sh[(3 + j) * BA_W])));
    }
  }
  d.Pg[pg_base + i] = gm;
}

// one block per camera over its images' rows (two fixed-order levels: observations -> image, images -> camera)
__global__ void __launch_bounds__(BA_W) k_ba_grad_cam(BaDev d, int gate, uint32_t pg_base) {
  __shared__ double sh[24 * BA_W];
  if (gate && (d.ctl->done || !d.ctl->accepted)) return;
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const int k = d.cam_k[c];
  for (int v = 0; v < 24; ++v) sh[v * BA_W + t] = 0.0;
  for (uint32_t a = d.cam_img_off[c] + t; a < d.cam_img_off[c + 1]; a += BA_W) {
    const double* row = d.icam + (size_t)BA_ICAM * d.cam_imgs[a];
    for (int j = 0; j < k; ++j) {
      sh[j * BA_W + t] += row[j];
      sh[(12 + j) * BA_W + t] += row[12 + j];
    }
  }
  __syncthreads();
  block_tree<BA_W>(sh, 24);
  if (t) return;
  double gm = 0.0;
  const uint32_t fo = d.cam_foff[c];
  const double* prm = d.prm + d.cam_poff[c];
  for (int j = 0; j < k; ++j) {
    d.gf[fo + j] = sh[j * BA_W];
    d.cnf[fo + j] = sh[(12 + j) * BA_W];
    const double x = prm[d.cam_free[BA_KMAX * (size_t)c + j]];
    gm = fmax(gm, fabs(x - (x + -sh[j * BA_W])));
  }
  d.Pg[pg_base + c] = gm;
}

// Jacobi scaling s = 1 / (1 + |column|) (first evaluation only), then the scaled gradient and D = clamp(diag(J^T J))
__global__ void __launch_bounds__(BA_B) k_ba_scale_cols(BaDev d, int first, int gate) {
  if (gate && (d.ctl->done || !d.ctl->accepted)) return;
  const size_t e = (size_t)blockIdx.x * BA_B + threadIdx.x, ne = 3 * (size_t)d.n_pts;
  if (e >= ne + d.nf) return;
  const bool isE = e < ne;
  const size_t j = isE ? e : e - ne;
  double* s = isE ? d.se : d.sf;
  double* g = isE ? d.ge : d.gf;
  const double cn = isE ? d.cne[j] : d.cnf[j];
  if (first) s[j] = 1.0 / (1.0 + sqrt(cn));
  g[j] = s[j] * g[j];
  (isE ? d.De : d.Df)[j] = fmin(fmax(s[j] * s[j] * cn, kLmMinDiag), kLmMaxDiag);
}

__global__ void __launch_bounds__(BA_B) k_ba_scale_J(BaDev d, int gate) {
  if (gate && (d.ctl->done || !d.ctl->accepted)) return;
  const uint32_t o = blockIdx.x * BA_B + threadIdx.x;
  if (o >= d.n_obs) return;
  double* Jo = d.J + (size_t)BA_JS * o;
  const uint32_t i = d.o_img[o], p = d.o_pt[o], cam = d.img_cam[i];
  const int k = d.cam_k[cam];
  for (int row = 0; row < 2; ++row) {
    for (int a = 0; a < 3; ++a) {
      Jo[J_E + 3 * row + a] *= d.se[3 * (size_t)p + a];
      Jo[J_Q + 3 * row + a] *= d.sf[6 * (size_t)i + a];
      Jo[J_T + 3 * row + a] *= d.sf[6 * (size_t)i + 3 + a];
    }
    for (int j = 0; j < k; ++j) Jo[J_C + BA_KMAX * row + j] *= d.sf[d.cam_foff[cam] + j];
  }
}

// ---------------------------------------------------------------- the linear system of one radius
// per point: C = E^T E + D_e / radius, C^-1 and C^-1 g_e
__global__ void __launch_bounds__(BA_B) k_ba_prep_pts(BaDev d) {
  if (d.ctl->done) return;
  const uint32_t p = blockIdx.x * BA_B + threadIdx.x;
  if (p >= d.n_pts) return;
  double* Ci = d.Cinv + 9 * (size_t)p;
  double* v = d.ve + 3 * (size_t)p;
  if (!d.pt_var[p]) {
    for (int j = 0; j < 9; ++j) Ci[j] = 0.0;
    for (int j = 0; j < 3; ++j) v[j] = 0.0;
    return;
  }
  const double radius = d.ctl->radius;
  double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint32_t a = d.trk_off[p]; a < d.trk_off[p + 1]; ++a) {
    const double* E = d.J + (size_t)BA_JS * d.trk[a] + J_E;
    for (int m = 0; m < 3; ++m)
      for (int n = 0; n <= m; ++n) C[tri(m, n)] += E[m] * E[n] + E[3 + m] * E[3 + n];
  }
  for (int m = 0; m < 3; ++m) {
    const double l = sqrt(d.De[3 * (size_t)p + m] / radius);
    C[tri(m, m)] += l * l;
  }
  inv3_sym(C, Ci);
  const double* g = d.ge + 3 * (size_t)p;
  for (int m = 0; m < 3; ++m) v[m] = Ci[3 * m] * g[0] + Ci[3 * m + 1] * g[1] + Ci[3 * m + 2] * g[2];
}

// B = E^T F (3 x 3) for one observation's 2 x 3 blocks; the Schur term B^T C^-1 B (packed) subtracted from P
__device__ inline void schur_sub33(const double* E, const double* F, const double* Ci, double* acc, int stride) {
  double B[9], CB[9];
  for (int m = 0; m < 3; ++m)
    for (int n = 0; n < 3; ++n) B[3 * m + n] = E[m] * F[n] + E[3 + m] * F[3 + n];
  for (int m = 0; m < 3; ++m)
    for (int n = 0; n < 3; ++n) CB[3 * m + n] = Ci[3 * m] * B[n] + Ci[3 * m + 1] * B[3 + n] + Ci[3 * m + 2] * B[6 + n];
  for (int m = 0; m < 3; ++m)
    for (int n = 0; n <= m; ++n) {
      const double ff = F[m] * F[n] + F[3 + m] * F[3 + n];
      const double s = B[m] * CB[n] + B[3 + m] * CB[3 + n] + B[6 + m] * CB[6 + n];
      acc[tri(m, n) * stride] += ff - s;
    }
}

// one block per image: b_q, b_t, the preconditioner blocks of qvec and tvec (inverted), and the camera's part of the image:
// F_c^T E v and F_c^T F_c, minus G^T C^-1 G of every camera run this image heads (G = sum over the run of E^T F_c)
constexpr int PI_RQ = 0, PI_RT = 3, PI_PQ = 6, PI_PT = 12, PI_RC = 18, PI_PC = 30, PI_N = 108;
__global__ void __launch_bounds__(BA_W) k_ba_prep_img(BaDev d) {
  __shared__ double sh[PI_N * BA_W];
  if (d.ctl->done) return;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const uint32_t cam = d.img_cam[i];
  const int k = d.cam_k[cam];
  double* a = sh + t;
  for (int v = 0; v < PI_N; ++v) a[v * BA_W] = 0.0;
  for (uint32_t o = d.img_off[i] + t; o < d.img_off[i + 1]; o += BA_W) {
    const double* Jo = d.J + (size_t)BA_JS * o;
    const uint32_t p = d.o_pt[o];
    const double* E = Jo + J_E;
    const double* Ci = d.Cinv + 9 * (size_t)p;
    const double* v = d.ve + 3 * (size_t)p;
    const double Ev0 = E[0] * v[0] + E[1] * v[1] + E[2] * v[2], Ev1 = E[3] * v[0] + E[4] * v[1] + E[5] * v[2];
    for (int blk = 0; blk < 2; ++blk) {
      const double* F = Jo + (blk ? J_T : J_Q);
      for (int m = 0; m < 3; ++m) a[((blk ? PI_RT : PI_RQ) + m) * BA_W] += F[m] * Ev0 + F[3 + m] * Ev1;
      schur_sub33(E, F, Ci, a + (blk ? PI_PT : PI_PQ) * BA_W, BA_W);
    }
    const double* Fc = Jo + J_C;
    for (int m = 0; m < k; ++m) {
      a[(PI_RC + m) * BA_W] += Fc[m] * Ev0 + Fc[BA_KMAX + m] * Ev1;
      for (int n = 0; n <= m; ++n) a[(PI_PC + tri(m, n)) * BA_W] += Fc[m] * Fc[n] + Fc[BA_KMAX + m] * Fc[BA_KMAX + n];
    }
    const uint32_t run0 = d.o_run[2 * (size_t)o], runn = d.o_run[2 * (size_t)o + 1];
    if (k && runn && d.pt_var[p]) {
      double G[3 * BA_KMAX];  // G[m * k + n] = sum E[:, m] . Fc[:, n]
      for (int j = 0; j < 3 * k; ++j) G[j] = 0.0;
      for (uint32_t s = run0; s < run0 + runn; ++s) {
        const double* Jr = d.J + (size_t)BA_JS * d.trk[s];
        for (int m = 0; m < 3; ++m)
          for (int n = 0; n < k; ++n) G[m * k + n] += Jr[J_E + m] * Jr[J_C + n] + Jr[J_E + 3 + m] * Jr[J_C + BA_KMAX + n];
      }
      for (int m = 0; m < k; ++m) {
        double cg[3];
        for (int u = 0; u < 3; ++u) cg[u] = Ci[3 * u] * G[m] + Ci[3 * u + 1] * G[k + m] + Ci[3 * u + 2] * G[2 * k + m];
        for (int n = 0; n <= m; ++n) a[(PI_PC + tri(m, n)) * BA_W] -= G[n] * cg[0] + G[k + n] * cg[1] + G[2 * k + n] * cg[2];
      }
    }
  }
  __syncthreads();
  block_tree<BA_W>(sh, PI_N);
  if (t) return;
  const double radius = d.ctl->radius;
  for (int blk = 0; blk < 2; ++blk) {
    double P[6];
    for (int j = 0; j < 6; ++j) P[j] = sh[((blk ? PI_PT : PI_PQ) + j) * BA_W];
    for (int m = 0; m < 3; ++m) {
      const size_t col = 6 * (size_t)i + 3 * blk + m;
      const double l = sqrt(d.Df[col] / radius);
      d.ddf[col] = l * l;
      P[tri(m, m)] += l * l;
      d.b[col] = -d.gf[col] + sh[((blk ? PI_RT : PI_RQ) + m) * BA_W];
    }
    inv3_sym(P, d.Minv + 18 * (size_t)i + 9 * blk);
  }
  double* row = d.icam + (size_t)BA_ICAM * i;
  for (int j = 0; j < BA_ICAM; ++j) row[j] = sh[(PI_RC + j) * BA_W];
}

__global__ void __launch_bounds__(BA_W) k_ba_prep_cam(BaDev d) {
  __shared__ double sh[BA_ICAM * BA_W];
  __shared__ double L[BA_KMAX * BA_KMAX];
  if (d.ctl->done) return;
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const int k = d.cam_k[c];
  if (!k) return;
  const int nv = 12 + k * (k + 1) / 2;
  for (int v = 0; v < nv; ++v) sh[v * BA_W + t] = 0.0;
  for (uint32_t a = d.cam_img_off[c] + t; a < d.cam_img_off[c + 1]; a += BA_W) {
    const double* row = d.icam + (size_t)BA_ICAM * d.cam_imgs[a];
    for (int v = 0; v < nv; ++v) sh[v * BA_W + t] += row[v];
  }
  __syncthreads();
  block_tree<BA_W>(sh, nv);
  if (t) return;
  const double radius = d.ctl->radius;
  const uint32_t fo = d.cam_foff[c];
  double P[78];
  for (int j = 0; j < k * (k + 1) / 2; ++j) P[j] = sh[(12 + j) * BA_W];
  for (int m = 0; m < k; ++m) {
    const double l = sqrt(d.Df[fo + m] / radius);
    d.ddf[fo + m] = l * l;
    P[tri(m, m)] += l * l;
    d.b[fo + m] = -d.gf[fo + m] + sh[m * BA_W];
  }
  inv_spd(P, k, L, d.Minv + d.cam_moff[c]);
}

// x = 0, r = b; partials of b.b
__global__ void __launch_bounds__(BA_B) k_ba_cg_init(BaDev d) {
  __shared__ double sh[BA_B];
  if (d.ctl->done) return;
  const uint32_t j = blockIdx.x * BA_B + threadIdx.x;
  double s = 0.0;
  if (j < d.nf) {
    const double bj = d.b[j];
    d.x[j] = 0.0;
    d.r[j] = bj;
    s = bj * bj;
  }
  s = block_sum<BA_B>(s, sh);
  if (threadIdx.x == 0) d.Pq[blockIdx.x] = s;
}
__global__ void __launch_bounds__(BA_B) k_ba_cg_init_fin(BaDev d, uint32_t nblk) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (c->done) return;
  const double bb = sum_partials<BA_B>(d.Pq, nblk, sh);
  if (threadIdx.x) return;
  c->cg_fail = 0;
  c->cg_iters = 0;
  c->rho = 1.0;
  c->Q0 = 0.0;
  c->cg_stop = (d.nf == 0 || sqrt(bb) == 0.0) ? 0 : INT_MAX;  // |b| = 0: the zero step
}

// ---------------------------------------------------------------- one CG iteration (k = 1, 2, ...)
// z = M^-1 r per f block (images' qvec and tvec, then the cameras); partials of r.z
__global__ void __launch_bounds__(BA_B) k_ba_cg_z(BaDev d, int k) {
  __shared__ double sh[BA_B];
  if (cg_gated(d.ctl, k)) return;
  const uint32_t e = blockIdx.x * BA_B + threadIdx.x;
  double s = 0.0;
  if (e < 2 * d.n_img) {
    const size_t o = 3 * (size_t)e;
    const double* M = d.Minv + 9 * (size_t)e;
    for (int m = 0; m < 3; ++m) {
      const double zm = M[3 * m] * d.r[o] + M[3 * m + 1] * d.r[o + 1] + M[3 * m + 2] * d.r[o + 2];
      d.z[o + m] = zm;
      s += d.r[o + m] * zm;
    }
  } else if (e < 2 * d.n_img + d.n_cam) {
    const uint32_t c = e - 2 * d.n_img;
    const int kc = d.cam_k[c];
    const uint32_t fo = d.cam_foff[c];
    const double* M = d.Minv + d.cam_moff[c];
    for (int m = 0; m < kc; ++m) {
      double zm = 0.0;
      for (int n = 0; n < kc; ++n) zm += M[m * kc + n] * d.r[fo + n];
      d.z[fo + m] = zm;
      s += d.r[fo + m] * zm;
    }
  }
  s = block_sum<BA_B>(s, sh);
  if (threadIdx.x == 0) d.Pq[blockIdx.x] = s;
}
__device__ inline bool zero_or_inf(double x) { return x == 0.0 || isinf(x); }
__global__ void __launch_bounds__(BA_B) k_ba_cg_fin_rz(BaDev d, uint32_t nblk, int k) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (cg_gated(c, k)) return;
  const double rho = sum_partials<BA_B>(d.Pq, nblk, sh);
  if (threadIdx.x) return;
  const double last = c->rho;
  c->rho = rho;
  if (zero_or_inf(rho)) {
    c->cg_fail = 1;
  } else if (k > 1) {
    c->beta = rho / last;
    if (zero_or_inf(c->beta)) c->cg_fail = 1;
  }
  if (c->cg_fail) {
    c->cg_stop = k;
    c->cg_iters = k;
  }
}
__global__ void __launch_bounds__(BA_B) k_ba_cg_p(BaDev d, int k) {
  if (cg_gated(d.ctl, k)) return;
  const uint32_t j = blockIdx.x * BA_B + threadIdx.x;
  if (j >= d.nf) return;
  d.p[j] = k == 1 ? d.z[j] : d.z[j] + d.ctl->beta * d.p[j];
}

// S v = (F^T F + D_f) v - F^T E C^-1 E^T F v in four passes.  y_o = F_o v
__global__ void __launch_bounds__(BA_B) k_ba_Fv(BaDev d, const double* __restrict__ v, int k) {
  if (k > 0 && cg_gated(d.ctl, k)) return;
  if (k == 0 && d.ctl->done) return;
  const uint32_t o = blockIdx.x * BA_B + threadIdx.x;
  if (o >= d.n_obs) return;
  const double* Jo = d.J + (size_t)BA_JS * o;
  const uint32_t i = d.o_img[o], cam = d.img_cam[i];
  const int kc = d.cam_k[cam];
  const double* vi = v + 6 * (size_t)i;
  const double* vc = v + d.cam_foff[cam];
  for (int row = 0; row < 2; ++row) {
    double s = 0.0;
    for (int a = 0; a < 3; ++a) s += Jo[J_Q + 3 * row + a] * vi[a] + Jo[J_T + 3 * row + a] * vi[3 + a];
    for (int j = 0; j < kc; ++j) s += Jo[J_C + BA_KMAX * row + j] * vc[j];
    d.y[2 * (size_t)o + row] = s;
  }
}
// z_p = C_p^-1 sum over the track of E^T y
__global__ void __launch_bounds__(BA_B) k_ba_Ey(BaDev d, int k) {
  if (k > 0 && cg_gated(d.ctl, k)) return;
  const uint32_t p = blockIdx.x * BA_B + threadIdx.x;
  if (p >= d.n_pts) return;
  double s[3] = {0.0, 0.0, 0.0};
  if (d.pt_var[p])
    for (uint32_t a = d.trk_off[p]; a < d.trk_off[p + 1]; ++a) {
      const uint32_t o = d.trk[a];
      const double* E = d.J + (size_t)BA_JS * o + J_E;
      const double y0 = d.y[2 * (size_t)o], y1 = d.y[2 * (size_t)o + 1];
      for (int m = 0; m < 3; ++m) s[m] += E[m] * y0 + E[3 + m] * y1;
    }
  const double* Ci = d.Cinv + 9 * (size_t)p;
  for (int m = 0; m < 3; ++m) d.zp[3 * (size_t)p + m] = Ci[3 * m] * s[0] + Ci[3 * m + 1] * s[1] + Ci[3 * m + 2] * s[2];
}
// out_i = D v_i + sum over the image of F^T (y - E z); the camera part of the image into icam[i]; v.out partials per image
__global__ void __launch_bounds__(BA_W) k_ba_Sv_img(BaDev d, const double* __restrict__ v, double* __restrict__ out, int k) {
  __shared__ double sh[18 * BA_W];
  if (cg_gated(d.ctl, k)) return;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const int kc = d.cam_k[d.img_cam[i]];
  double* a = sh + t;
  for (int u = 0; u < 18; ++u) a[u * BA_W] = 0.0;
  for (uint32_t o = d.img_off[i] + t; o < d.img_off[i + 1]; o += BA_W) {
    const double* Jo = d.J + (size_t)BA_JS * o;
    const double* zp = d.zp + 3 * (size_t)d.o_pt[o];
    const double w0 = d.y[2 * (size_t)o] - (Jo[J_E] * zp[0] + Jo[J_E + 1] * zp[1] + Jo[J_E + 2] * zp[2]);
    const double w1 = d.y[2 * (size_t)o + 1] - (Jo[J_E + 3] * zp[0] + Jo[J_E + 4] * zp[1] + Jo[J_E + 5] * zp[2]);
    for (int m = 0; m < 3; ++m) {
      a[m * BA_W] += Jo[J_Q + m] * w0 + Jo[J_Q + 3 + m] * w1;
      a[(3 + m) * BA_W] += Jo[J_T + m] * w0 + Jo[J_T + 3 + m] * w1;
    }
    for (int j = 0; j < kc; ++j) a[(6 + j) * BA_W] += Jo[J_C + j] * w0 + Jo[J_C + BA_KMAX + j] * w1;
  }
  __syncthreads();
  block_tree<BA_W>(sh, 18);
  if (t) return;
  double dot = 0.0;
  for (int m = 0; m < 6; ++m) {
    const size_t col = 6 * (size_t)i + m;
    const double o = d.ddf[col] * v[col] + sh[m * BA_W];
    out[col] = o;
    dot += v[col] * o;
  }
  for (int j = 0; j < kc; ++j) d.icam[(size_t)BA_ICAM * i + j] = sh[(6 + j) * BA_W];
  d.Pd[i] = dot;
}
__global__ void __launch_bounds__(BA_W) k_ba_Sv_cam(BaDev d, const double* __restrict__ v, double* __restrict__ out, int k) {
  __shared__ double sh[BA_KMAX * BA_W];
  if (cg_gated(d.ctl, k)) return;
  const uint32_t c = blockIdx.x, t = threadIdx.x;
  const int kc = d.cam_k[c];
  for (int u = 0; u < kc; ++u) sh[u * BA_W + t] = 0.0;
  for (uint32_t a = d.cam_img_off[c] + t; a < d.cam_img_off[c + 1]; a += BA_W) {
    const double* row = d.icam + (size_t)BA_ICAM * d.cam_imgs[a];
    for (int j = 0; j < kc; ++j) sh[j * BA_W + t] += row[j];
  }
  __syncthreads();
  block_tree<BA_W>(sh, kc);
  if (t) return;
  double dot = 0.0;
  const uint32_t fo = d.cam_foff[c];
  for (int j = 0; j < kc; ++j) {
    const double o = d.ddf[fo + j] * v[fo + j] + sh[j * BA_W];
    out[fo + j] = o;
    dot += v[fo + j] * o;
  }
  d.Pd[d.n_img + c] = dot;
}
__global__ void __launch_bounds__(BA_B) k_ba_cg_fin_pq(BaDev d, int k) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (cg_gated(c, k)) return;
  const double pq = sum_partials<BA_B>(d.Pd, d.n_img + d.n_cam, sh);
  if (threadIdx.x) return;
  if (pq <= 0.0 || isinf(pq) || isnan(pq)) {
    c->cg_fail = 2;
  } else {
    c->alpha = c->rho / pq;
    if (isinf(c->alpha)) c->cg_fail = 1;
  }
  if (c->cg_fail) {
    c->cg_stop = k;
    c->cg_iters = k;
  }
}
// x += alpha p; r -= alpha q (reset = 0) ; partials of x.(b + r)
__global__ void __launch_bounds__(BA_B) k_ba_cg_x(BaDev d, int k, int reset) {
  __shared__ double sh[BA_B];
  if (cg_gated(d.ctl, k)) return;
  const uint32_t j = blockIdx.x * BA_B + threadIdx.x;
  double s = 0.0;
  if (j < d.nf) {
    const double al = d.ctl->alpha;
    const double xj = d.x[j] + al * d.p[j];
    d.x[j] = xj;
    if (!reset) {
      const double rj = d.r[j] - al * d.qv[j];
      d.r[j] = rj;
      s = xj * (d.b[j] + rj);
    }
  }
  s = block_sum<BA_B>(s, sh);
  if (threadIdx.x == 0 && !reset) d.Pq[blockIdx.x] = s;
}
// every residual_reset_period = 10 iterations: r = b - S x
__global__ void __launch_bounds__(BA_B) k_ba_cg_reset(BaDev d, int k) {
  __shared__ double sh[BA_B];
  if (cg_gated(d.ctl, k)) return;
  const uint32_t j = blockIdx.x * BA_B + threadIdx.x;
  double s = 0.0;
  if (j < d.nf) {
    const double rj = d.b[j] - d.tmp[j];
    d.r[j] = rj;
    s = d.x[j] * (d.b[j] + rj);
  }
  s = block_sum<BA_B>(s, sh);
  if (threadIdx.x == 0) d.Pq[blockIdx.x] = s;
}
// Q1 = -x.(b + r); stop when k (Q1 - Q0) / Q1 < eta or at the iteration cap
__global__ void __launch_bounds__(BA_B) k_ba_cg_fin_q(BaDev d, uint32_t nblk, int k) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (cg_gated(c, k)) return;
  const double Q1 = -sum_partials<BA_B>(d.Pq, nblk, sh);
  if (threadIdx.x) return;
  const double zeta = k * (Q1 - c->Q0) / Q1;
  tr_min(&c->m_cg, tr_margin(zeta, kEta));
  if (zeta < kEta || k >= d.max_cg) {
    c->cg_stop = k + 1;
    c->cg_iters = k;
  } else {
    c->Q0 = Q1;
  }
}

// ---------------------------------------------------------------- the step, the candidate and the decision
// back-substitution dy = -C^-1 (g_e + E^T F x) (y holds F x); the candidate point; partials of |delta|^2 and |x|^2
__global__ void __launch_bounds__(BA_B) k_ba_backsub(BaDev d) {
  __shared__ double sh[BA_B];
  if (d.ctl->done) return;
  const uint32_t p = blockIdx.x * BA_B + threadIdx.x;
  double s2 = 0.0, x2 = 0.0;
  if (p < d.n_pts) {
    const double* X = d.X + 3 * (size_t)p;
    double* cX = d.cX + 3 * (size_t)p;
    if (d.pt_var[p]) {
      double s[3] = {d.ge[3 * (size_t)p], d.ge[3 * (size_t)p + 1], d.ge[3 * (size_t)p + 2]};
      for (uint32_t a = d.trk_off[p]; a < d.trk_off[p + 1]; ++a) {
        const uint32_t o = d.trk[a];
        const double* E = d.J + (size_t)BA_JS * o + J_E;
        const double y0 = d.y[2 * (size_t)o], y1 = d.y[2 * (size_t)o + 1];
        for (int m = 0; m < 3; ++m) s[m] += E[m] * y0 + E[3 + m] * y1;
      }
      const double* Ci = d.Cinv + 9 * (size_t)p;
      for (int m = 0; m < 3; ++m) {
        const double dym = -(Ci[3 * m] * s[0] + Ci[3 * m + 1] * s[1] + Ci[3 * m + 2] * s[2]);
        d.dy[3 * (size_t)p + m] = dym;
        const double delta = d.se[3 * (size_t)p + m] * dym;
        cX[m] = X[m] + delta;
        s2 += delta * delta;
        x2 += X[m] * X[m];
      }
    } else {
      for (int m = 0; m < 3; ++m) {
        d.dy[3 * (size_t)p + m] = 0.0;
        cX[m] = X[m];
      }
    }
  }
  const double a = block_sum<BA_B>(s2, sh), b = block_sum<BA_B>(x2, sh);
  if (threadIdx.x == 0) {
    d.Pe[blockIdx.x] = a;
    d.Pe[gridDim.x + blockIdx.x] = b;
  }
}
// the candidate qvec / tvec / camera params: Plus(x, s * step); partials of |delta|^2 and |x|^2 (variable blocks, ambient)
__global__ void __launch_bounds__(BA_B) k_ba_cand_f(BaDev d) {
  __shared__ double sh[BA_B];
  if (d.ctl->done) return;
  const uint32_t e = blockIdx.x * BA_B + threadIdx.x;
  double s2 = 0.0, x2 = 0.0;
  if (e < d.n_img) {
    const double* q = d.q + 4 * (size_t)e;
    const double* tv = d.t + 3 * (size_t)e;
    double* cq = d.cq + 4 * (size_t)e;
    double* ct = d.ct + 3 * (size_t)e;
    if (!d.img_cpose[e] && d.img_off[e + 1] > d.img_off[e]) {
      double dq[3];
      for (int m = 0; m < 3; ++m) {
        dq[m] = d.sf[6 * (size_t)e + m] * d.x[6 * (size_t)e + m];
        s2 += dq[m] * dq[m];
      }
      ba_quat_plus(q, dq, cq);
      for (int m = 0; m < 4; ++m) x2 += q[m] * q[m];
      const uint8_t mask = d.img_mask[e];
      for (int m = 0; m < 3; ++m) {
        x2 += tv[m] * tv[m];
        if ((mask >> m) & 1) {
          ct[m] = tv[m];
        } else {
          const double dl = d.sf[6 * (size_t)e + 3 + m] * d.x[6 * (size_t)e + 3 + m];
          ct[m] = tv[m] + dl;
          s2 += dl * dl;
        }
      }
    } else {
      for (int m = 0; m < 4; ++m) cq[m] = q[m];
      for (int m = 0; m < 3; ++m) ct[m] = tv[m];
    }
  } else if (e < d.n_img + d.n_cam) {
    const uint32_t c = e - d.n_img;
    const int kc = d.cam_k[c], np = d.cam_np[c];
    const double* prm = d.prm + d.cam_poff[c];
    double* cp = d.cprm + d.cam_poff[c];
    for (int j = 0; j < np; ++j) {
      cp[j] = prm[j];
      if (kc) x2 += prm[j] * prm[j];
    }
    for (int j = 0; j < kc; ++j) {
      const int pi = d.cam_free[BA_KMAX * (size_t)c + j];
      const double dl = d.sf[d.cam_foff[c] + j] * d.x[d.cam_foff[c] + j];
      cp[pi] = prm[pi] + dl;
      s2 += dl * dl;
    }
  }
  const double a = block_sum<BA_B>(s2, sh), b = block_sum<BA_B>(x2, sh);
  if (threadIdx.x == 0) {
    d.Pd[blockIdx.x] = a;
    d.Pd[gridDim.x + blockIdx.x] = b;
  }
}
// model_cost_change terms: (J step).(r + J step / 2) per observation
__global__ void __launch_bounds__(BA_B) k_ba_mcc(BaDev d) {
  __shared__ double sh[BA_B];
  if (d.ctl->done) return;
  const uint32_t o = blockIdx.x * BA_B + threadIdx.x;
  double s = 0.0;
  if (o < d.n_obs) {
    const double* Jo = d.J + (size_t)BA_JS * o;
    const double* dy = d.dy + 3 * (size_t)d.o_pt[o];
    for (int row = 0; row < 2; ++row) {
      const double js = d.y[2 * (size_t)o + row] + Jo[J_E + 3 * row] * dy[0] + Jo[J_E + 3 * row + 1] * dy[1] + Jo[J_E + 3 * row + 2] * dy[2];
      s += js * (Jo[J_R + row] + js / 2.0);
    }
  }
  s = block_sum<BA_B>(s, sh);
  if (threadIdx.x == 0) d.Pm[blockIdx.x] = s;
}

// the LM decision of one iteration (TrustRegionMinimizer + LevenbergMarquardtStrategy as DESIGN.md 12 states them)
__global__ void __launch_bounds__(BA_B) k_ba_decide(BaDev d, uint32_t nb_obs, uint32_t nb_pts, uint32_t nb_f) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  if (c->done) return;
  const double mcc = -sum_partials<BA_B>(d.Pm, nb_obs, sh);
  const double s2 = sum_partials<BA_B>(d.Pe, nb_pts, sh) + sum_partials<BA_B>(d.Pd, nb_f, sh);
  const double x2 = sum_partials<BA_B>(d.Pe + nb_pts, nb_pts, sh) + sum_partials<BA_B>(d.Pd + nb_f, nb_f, sh);
  if (threadIdx.x) return;
  c->mcc = mcc;
  c->cg_total += (unsigned long long)c->cg_iters;
  if (tr_decide(c, d.tr, c->cg_fail == 0, c->cand_cost, mcc, s2, x2) == TR_ACCEPTED) c->reproj = c->cand_reproj;
}
__global__ void __launch_bounds__(BA_B) k_ba_commit(BaDev d) {
  if (d.ctl->done || !d.ctl->accepted) return;
  const size_t e = (size_t)blockIdx.x * BA_B + threadIdx.x;
  const size_t nX = 3 * (size_t)d.n_pts, nq = 4 * (size_t)d.n_img, nt = 3 * (size_t)d.n_img;
  if (e < nX) d.X[e] = d.cX[e];
  else if (e < nX + nq) d.q[e - nX] = d.cq[e - nX];
  else if (e < nX + nq + nt) d.t[e - nX - nq] = d.ct[e - nX - nq];
}
__global__ void __launch_bounds__(BA_B) k_ba_commit_prm(BaDev d, uint32_t n_prm) {
  if (d.ctl->done || !d.ctl->accepted) return;
  const uint32_t e = blockIdx.x * BA_B + threadIdx.x;
  if (e < n_prm) d.prm[e] = d.cprm[e];
}
// the gradient max-norm of the state; then the checks that end an iteration: the cap, the gradient (after an accepted step
// or at iteration 0), the radius; one trace row
__global__ void __launch_bounds__(BA_B) k_ba_finalize(BaDev d, uint32_t n_gparts, int first) {
  __shared__ double sh[BA_B];
  BaCtl* c = d.ctl;
  const int latched = c->pad1, done = c->done, accepted = c->accepted;
  __syncthreads();  // every thread has read the flags before thread 0 writes them
  if (latched) return;
  const bool fresh = first || (accepted && !done);
  double gm = 0.0;
  if (fresh) gm = max_partials<BA_B>(d.Pg, n_gparts, sh);
  if (threadIdx.x) return;
  if (fresh) c->gnorm = gm;
  tr_end_iteration(c, d.tr, fresh);
  if (d.trace) {
    double* row = d.trace + DSM_BA_TRACE_COLUMNS * (size_t)c->iter;
    row[0] = c->cost;
    row[1] = c->radius;
    row[2] = first ? NAN : c->last_rho;
    row[3] = first ? 0.0 : (double)c->cg_iters;
    row[4] = first ? 1.0 : (double)c->accepted;
    row[5] = c->gnorm;
  }
  c->pad1 = c->done;  // latched: nothing after the end of the loop changes the control block
}

// ---------------------------------------------------------------- host side
struct BaProblem {
  std::vector<uint32_t> o_img, o_pt, o_run, img_off, trk_off, trk, cam_img_off, cam_imgs, cam_poff, cam_foff, cam_moff;
  std::vector<double> o_xy;
  std::vector<uint8_t> cpose, mask, pt_var;
  std::vector<int> cam_k, cam_free, cam_np;
  uint32_t nf = 0, n_minv = 0;
  uint64_t n_eff = 0;
};

}  // namespace

extern "C" void dsm_default_bundle_adjustment_options(dsm_bundle_adjustment_options* o) {
  if (!o) return;
  *o = dsm_bundle_adjustment_options{};
  o->max_num_iterations = 50;
  o->max_linear_solver_iterations = 100;
  o->gradient_tolerance = 1.0;
  o->function_tolerance = 0.0;
  o->parameter_tolerance = 0.0;
  o->max_num_consecutive_invalid_steps = 10;
  o->refine_focal_length = 1;
  o->refine_principal_point = 0;
  o->refine_extra_params = 1;
}

extern "C" int dsm_bundle_adjust(dsm_ctx* ctx, uint32_t num_cameras, const int32_t* camera_model_ids, double* camera_params,
                                 uint32_t num_images, const uint32_t* image_camera, double* image_qvec, double* image_tvec,
                                 const uint8_t* image_constant_pose, const uint8_t* image_constant_tvec, uint32_t num_points,
                                 const uint64_t* point_ids, double* point_xyz, const uint8_t* point_constant,
                                 const uint32_t* track_offsets, const uint32_t* obs_image, const double* obs_xy,
                                 const dsm_bundle_adjustment_options* options, dsm_bundle_adjustment_report* report, double* trace) {
  const auto t_start = std::chrono::steady_clock::now();
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!track_offsets || (num_cameras && (!camera_model_ids || !camera_params)) ||
      (num_images && (!image_camera || !image_qvec || !image_tvec)) || (num_points && (!point_ids || !point_xyz)))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: NULL argument");
  dsm_bundle_adjustment_options o;
  if (options) o = *options;
  else dsm_default_bundle_adjustment_options(&o);
  auto fin_nonneg = [](double v) { return std::isfinite(v) && v >= 0.0; };
  if (o.max_num_iterations < 0 || o.max_num_iterations > 1000000 || o.max_linear_solver_iterations < 1 ||
      o.max_linear_solver_iterations > 1000000 || !fin_nonneg(o.gradient_tolerance) || !fin_nonneg(o.function_tolerance) ||
      !fin_nonneg(o.parameter_tolerance) || o.max_num_consecutive_invalid_steps < 0)
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: option out of range");
  uint32_t C = num_cameras, N = num_images;  // the caller's counts; below the canonical order, the problem's
  const uint32_t P = num_points;
  if (track_offsets[0] != 0) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: track_offsets must start at 0");
  const uint64_t n_obs64 = track_offsets[P];
  if (n_obs64 >= (1ull << 31) || (n_obs64 && (!obs_image || !obs_xy)))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: bad observation count");
  const uint32_t n_obs = (uint32_t)n_obs64;
  // ---- validation
  BaProblem pb;
  std::vector<uint32_t> poff_in(C + 1, 0);  // the caller's cameras
  for (uint32_t c = 0; c < C; ++c) {
    if (!cam_model_exists(camera_model_ids[c])) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: unknown camera model");
    poff_in[c + 1] = poff_in[c] + cam_num_params(camera_model_ids[c]);
  }
  for (uint32_t j = 0; j < poff_in[C]; ++j)
    if (!std::isfinite(camera_params[j])) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: non-finite camera parameter");
  for (uint32_t i = 0; i < N; ++i) {
    if (image_camera[i] >= C) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: image camera index out of range");
    const double* q = image_qvec + 4 * (size_t)i;
    bool fin = true;
    for (int m = 0; m < 4; ++m) fin = fin && std::isfinite(q[m]);
    for (int m = 0; m < 3; ++m) fin = fin && std::isfinite(image_tvec[3 * (size_t)i + m]);
    if (!fin) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: non-finite qvec or tvec");
    if (q[0] == 0.0 && q[1] == 0.0 && q[2] == 0.0 && q[3] == 0.0) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: zero qvec");
    if (image_constant_tvec && image_constant_tvec[i] > 7) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: constant-tvec mask above 7");
  }
  for (uint32_t p = 0; p < P; ++p) {
    if ((uint64_t)track_offsets[p + 1] < (uint64_t)track_offsets[p] + 2) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: track shorter than 2");
    for (int m = 0; m < 3; ++m)
      if (!std::isfinite(point_xyz[3 * (size_t)p + m])) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: non-finite point");
  }
  for (uint32_t a = 0; a < n_obs; ++a) {
    if (obs_image[a] >= N) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: observation image index out of range");
    if (!std::isfinite(obs_xy[2 * (size_t)a]) || !std::isfinite(obs_xy[2 * (size_t)a + 1]))
      return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: non-finite observation");
  }
  if (n_obs == 0) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: no residuals");
  // ---- canonical order: points by id; observations image-major by (image, point rank) (a counting pass over the points in
  // rank order); tracks by (camera, image) (a counting pass over the observations in camera, image order)
  std::vector<uint32_t> order(P);
  std::iota(order.begin(), order.end(), 0u);
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return point_ids[a] < point_ids[b]; });
  for (uint32_t r = 1; r < P; ++r)
    if (point_ids[order[r]] == point_ids[order[r - 1]]) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: repeated point id");
  // the images with observations by content: flags, pose, the camera's model and parameters, then -- only where all of that
  // ties -- the observations by point rank; the cameras by first use.  Images and cameras without residuals never reach the
  // device, so neither they nor the caller's order of the lists move a sum (as in local_bundle.hip).
  std::vector<uint32_t> iorder, corder;  // canonical index -> the caller's
  {
    std::vector<uint32_t> ioff(N + 1, 0), iobs(n_obs), orank(n_obs);
    for (uint32_t a = 0; a < n_obs; ++a) ++ioff[obs_image[a] + 1];
    for (uint32_t i = 0; i < N; ++i) ioff[i + 1] += ioff[i];
    std::vector<uint32_t> fill(ioff.begin(), ioff.end() - 1);
    for (uint32_t r = 0; r < P; ++r)
      for (uint32_t a = track_offsets[order[r]]; a < track_offsets[order[r] + 1]; ++a) {
        iobs[fill[obs_image[a]]++] = a;
        orank[a] = r;
      }
    auto bits = [](double v) {
      uint64_t u;
      memcpy(&u, &v, sizeof u);
      return u;
    };
    auto head = [&](uint32_t i, uint64_t* ky) {  // 22 words at most
      const uint32_t cam = image_camera[i];
      int n = 0;
      ky[n++] = image_constant_pose && image_constant_pose[i] ? 1 : 0;
      ky[n++] = image_constant_tvec ? image_constant_tvec[i] : 0;
      for (int a = 0; a < 4; ++a) ky[n++] = bits(image_qvec[4 * (size_t)i + a]);
      for (int a = 0; a < 3; ++a) ky[n++] = bits(image_tvec[3 * (size_t)i + a]);
      ky[n++] = (uint64_t)camera_model_ids[cam];
      for (uint32_t j = poff_in[cam]; j < poff_in[cam + 1]; ++j) ky[n++] = bits(camera_params[j]);
      return n;
    };
    for (uint32_t i = 0; i < N; ++i)
      if (ioff[i + 1] > ioff[i]) iorder.push_back(i);
    std::stable_sort(iorder.begin(), iorder.end(), [&](uint32_t x, uint32_t y) {
      uint64_t kx[24], ky[24];
      const int nx = head(x, kx), ny = head(y, ky);
      if (!std::equal(kx, kx + nx, ky, ky + ny)) return std::lexicographical_compare(kx, kx + nx, ky, ky + ny);
      const uint32_t lx = ioff[x + 1] - ioff[x], ly = ioff[y + 1] - ioff[y];
      for (uint32_t k = 0; k < lx && k < ly; ++k) {
        const uint32_t ax = iobs[ioff[x] + k], ay = iobs[ioff[y] + k];
        const uint64_t wx[3] = {orank[ax], bits(obs_xy[2 * (size_t)ax]), bits(obs_xy[2 * (size_t)ax + 1])};
        const uint64_t wy[3] = {orank[ay], bits(obs_xy[2 * (size_t)ay]), bits(obs_xy[2 * (size_t)ay + 1])};
        for (int a = 0; a < 3; ++a)
          if (wx[a] != wy[a]) return wx[a] < wy[a];
      }
      return lx < ly;
    });
  }
  std::vector<uint32_t> c_icam(iorder.size()), c_oimg(n_obs), poff(1, 0);
  std::vector<int32_t> c_model;
  std::vector<double> c_qvec(4 * iorder.size()), c_tvec(3 * iorder.size()), c_prm;
  std::vector<uint8_t> c_cpose(iorder.size()), c_mask(iorder.size());
  {
    std::vector<uint32_t> inew(N, 0), cnew(C, UINT32_MAX);
    for (uint32_t r = 0; r < iorder.size(); ++r) {
      const uint32_t i = iorder[r], c = image_camera[i];
      inew[i] = r;
      if (cnew[c] == UINT32_MAX) {
        cnew[c] = (uint32_t)corder.size();
        corder.push_back(c);
        c_model.push_back(camera_model_ids[c]);
        c_prm.insert(c_prm.end(), camera_params + poff_in[c], camera_params + poff_in[c + 1]);
        poff.push_back((uint32_t)c_prm.size());
      }
      c_icam[r] = cnew[c];
      std::copy(image_qvec + 4 * (size_t)i, image_qvec + 4 * (size_t)i + 4, c_qvec.begin() + 4 * (size_t)r);
      std::copy(image_tvec + 3 * (size_t)i, image_tvec + 3 * (size_t)i + 3, c_tvec.begin() + 3 * (size_t)r);
      c_cpose[r] = image_constant_pose && image_constant_pose[i];
      c_mask[r] = image_constant_tvec ? image_constant_tvec[i] : 0;
    }
    for (uint32_t a = 0; a < n_obs; ++a) c_oimg[a] = inew[obs_image[a]];
  }
  // from here on the problem in canonical order; the caller's arrays are written once, at the end
  double *const out_params = camera_params, *const out_qvec = image_qvec, *const out_tvec = image_tvec;
  N = (uint32_t)iorder.size();
  C = (uint32_t)corder.size();
  image_camera = c_icam.data();
  obs_image = c_oimg.data();
  camera_model_ids = c_model.data();
  camera_params = c_prm.data();
  image_qvec = c_qvec.data();
  image_tvec = c_tvec.data();
  image_constant_pose = c_cpose.data();
  image_constant_tvec = c_mask.data();
  const uint32_t n_prm = poff[C];
  pb.cam_np.resize(C);
  for (uint32_t c = 0; c < C; ++c) pb.cam_np[c] = (int)(poff[c + 1] - poff[c]);
  pb.img_off.assign(N + 1, 0);
  for (uint32_t a = 0; a < n_obs; ++a) ++pb.img_off[obs_image[a] + 1];
  for (uint32_t i = 0; i < N; ++i) pb.img_off[i + 1] += pb.img_off[i];
  pb.o_img.resize(n_obs);
  pb.o_pt.resize(n_obs);
  pb.o_xy.resize(2 * (size_t)n_obs);
  {
    std::vector<uint32_t> fill(pb.img_off.begin(), pb.img_off.end() - 1);
    for (uint32_t r = 0; r < P; ++r) {
      const uint32_t p = order[r];
      for (uint32_t a = track_offsets[p]; a < track_offsets[p + 1]; ++a) {
        const uint32_t o = fill[obs_image[a]]++;
        pb.o_img[o] = obs_image[a];
        pb.o_pt[o] = r;
        pb.o_xy[2 * (size_t)o] = obs_xy[2 * (size_t)a];
        pb.o_xy[2 * (size_t)o + 1] = obs_xy[2 * (size_t)a + 1];
      }
    }
  }
  for (uint32_t i = 0; i < N; ++i)
    for (uint32_t o = pb.img_off[i] + 1; o < pb.img_off[i + 1]; ++o)
      if (pb.o_pt[o] == pb.o_pt[o - 1]) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_bundle_adjust: an image observes a point twice");
  // cameras in the problem, their images, free parameters and f-layout
  pb.cam_img_off.assign(C + 1, 0);
  for (uint32_t i = 0; i < N; ++i)
    if (pb.img_off[i + 1] > pb.img_off[i]) ++pb.cam_img_off[image_camera[i] + 1];
  for (uint32_t c = 0; c < C; ++c) pb.cam_img_off[c + 1] += pb.cam_img_off[c];
  pb.cam_imgs.resize(pb.cam_img_off[C]);
  {
    std::vector<uint32_t> fill(pb.cam_img_off.begin(), pb.cam_img_off.end() - 1);
    for (uint32_t i = 0; i < N; ++i)
      if (pb.img_off[i + 1] > pb.img_off[i]) pb.cam_imgs[fill[image_camera[i]]++] = i;
  }
  pb.cam_k.assign(C, 0);
  pb.cam_free.assign((size_t)BA_KMAX * C, 0);
  pb.cam_foff.resize(C);
  pb.cam_moff.resize(C);
  pb.cpose.resize(N);
  pb.mask.resize(N);
  pb.nf = 6 * N;
  pb.n_minv = 18 * N;
  const bool any_refine = o.refine_focal_length || o.refine_principal_point || o.refine_extra_params;
  for (uint32_t c = 0; c < C; ++c) {
    pb.cam_foff[c] = pb.nf;
    pb.cam_moff[c] = pb.n_minv;
    if (pb.cam_img_off[c + 1] == pb.cam_img_off[c] || !any_refine) continue;
    const int m = camera_model_ids[c], np = pb.cam_np[c];
    const int nfoc = cam_two_focal(m) ? 2 : 1;
    int k = 0;
    for (int j = 0; j < np; ++j) {
      const bool keep = j < nfoc ? o.refine_focal_length : (j < nfoc + 2 ? o.refine_principal_point : o.refine_extra_params);
      if (keep) pb.cam_free[(size_t)BA_KMAX * c + k++] = j;
    }
    pb.cam_k[c] = k;
    pb.nf += k;
    pb.n_minv += k * k;
    pb.n_eff += k;
  }
  for (uint32_t i = 0; i < N; ++i) {
    pb.cpose[i] = image_constant_pose && image_constant_pose[i];
    pb.mask[i] = image_constant_tvec ? image_constant_tvec[i] : 0;
    if (pb.img_off[i + 1] > pb.img_off[i] && !pb.cpose[i]) pb.n_eff += 3 + 3 - __builtin_popcount(pb.mask[i]);
  }
  pb.pt_var.resize(P);
  for (uint32_t r = 0; r < P; ++r) {
    pb.pt_var[r] = !(point_constant && point_constant[order[r]]);
    if (pb.pt_var[r]) pb.n_eff += 3;
  }
  // tracks by (camera, image): walk cameras, their images, the images' observations; camera runs inside each track
  pb.trk_off.assign(P + 1, 0);
  for (uint32_t o = 0; o < n_obs; ++o) ++pb.trk_off[pb.o_pt[o] + 1];
  for (uint32_t r = 0; r < P; ++r) pb.trk_off[r + 1] += pb.trk_off[r];
  pb.trk.resize(n_obs);
  {
    std::vector<uint32_t> fill(pb.trk_off.begin(), pb.trk_off.end() - 1);
    for (uint32_t c = 0; c < C; ++c)
      for (uint32_t a = pb.cam_img_off[c]; a < pb.cam_img_off[c + 1]; ++a) {
        const uint32_t i = pb.cam_imgs[a];
        for (uint32_t o = pb.img_off[i]; o < pb.img_off[i + 1]; ++o) pb.trk[fill[pb.o_pt[o]]++] = o;
      }
  }
  pb.o_run.assign(2 * (size_t)n_obs, 0);
  for (uint32_t r = 0; r < P; ++r)
    for (uint32_t a = pb.trk_off[r]; a < pb.trk_off[r + 1];) {
      const uint32_t cam = image_camera[pb.o_img[pb.trk[a]]];
      uint32_t b = a + 1;
      while (b < pb.trk_off[r + 1] && image_camera[pb.o_img[pb.trk[b]]] == cam) ++b;
      pb.o_run[2 * (size_t)pb.trk[a]] = a;
      pb.o_run[2 * (size_t)pb.trk[a] + 1] = b - a;
      a = b;
    }
  // state: qvecs of the images in the problem normalised (AddImageToProblem), points in rank order
  std::vector<double> q(image_qvec, image_qvec + 4 * (size_t)N), X(3 * (size_t)P);
  for (uint32_t i = 0; i < N; ++i) {
    if (pb.img_off[i + 1] == pb.img_off[i]) continue;
    double* qi = q.data() + 4 * (size_t)i;
    const double n = std::sqrt(qi[0] * qi[0] + qi[1] * qi[1] + qi[2] * qi[2] + qi[3] * qi[3]);
    for (int m = 0; m < 4; ++m) qi[m] /= n;
  }
  for (uint32_t r = 0; r < P; ++r)
    for (int m = 0; m < 3; ++m) X[3 * (size_t)r + m] = point_xyz[3 * (size_t)order[r] + m];
  std::vector<int> cam_model(camera_model_ids, camera_model_ids + C);
  pb.cam_poff.assign(poff.begin(), poff.end());

  // ---- device
  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  const uint32_t nb_obs = (n_obs + BA_B - 1) / BA_B, nb_pts = std::max<uint32_t>(1, (P + BA_B - 1) / BA_B);
  const uint32_t nf = pb.nf, nb_f = std::max<uint32_t>(1, (nf + BA_B - 1) / BA_B);
  const uint32_t nb_blk = std::max<uint32_t>(1, (2 * N + C + BA_B - 1) / BA_B), nb_ent = std::max<uint32_t>(1, (N + C + BA_B - 1) / BA_B);
  const uint32_t nb_cols = (uint32_t)((3 * (size_t)P + nf + BA_B - 1) / BA_B);
  const uint32_t nb_commit = (uint32_t)((3 * (size_t)P + 7 * (size_t)N + BA_B - 1) / BA_B);
  const uint32_t n_gparts = nb_pts + N + C;
  const size_t nfa = (size_t)nf + 1;
  const uint32_t nb_fpart = std::max(nb_f, std::max(nb_blk, nb_ent));
  std::vector<uint32_t> img_cam(image_camera, image_camera + N);  // an upload's source: declared before the buffers, it outlives them
  DevBuf b_oimg, b_opt, b_orun, b_imgoff, b_trkoff, b_trk, b_camimgoff, b_camimgs, b_imgcam, b_campoff, b_camfoff, b_cammoff, b_oxy,
      b_cpose, b_mask, b_ptvar, b_cammodel, b_camnp, b_camk, b_camfree, b_q, b_t, b_X, b_prm, b_cq, b_ct, b_cX, b_cprm, b_J, b_y,
      b_ge, b_cne, b_se, b_De, b_Cinv, b_ve, b_zp, b_dy, b_gf, b_cnf, b_sf, b_Df, b_ddf, b_Minv, b_b, b_x, b_r, b_z, b_p, b_qv,
      b_tmp, b_icam, b_Pc, b_Pm, b_Pg, b_Pe, b_Pd, b_Pq, b_ctl, b_trace;
  DevEvents<6> ev;  // jacobian(first): 0-1; per LM iteration: 2 CG 3 candidate 4 Jacobian 5
  int rc = DSM_OK;
  auto alloc = [&](DevBuf& b, size_t bytes) { HIPTRY(b.reserve(std::max<size_t>(bytes, 8))); };
  HIPTRY(dev_upload(b_oimg, pb.o_img.data(), 4 * (size_t)n_obs, st));
  HIPTRY(dev_upload(b_opt, pb.o_pt.data(), 4 * (size_t)n_obs, st));
  HIPTRY(dev_upload(b_orun, pb.o_run.data(), 8 * (size_t)n_obs, st));
  HIPTRY(dev_upload(b_imgoff, pb.img_off.data(), 4 * ((size_t)N + 1), st));
  HIPTRY(dev_upload(b_trkoff, pb.trk_off.data(), 4 * ((size_t)P + 1), st));
  HIPTRY(dev_upload(b_trk, pb.trk.data(), 4 * (size_t)n_obs, st));
  HIPTRY(dev_upload(b_camimgoff, pb.cam_img_off.data(), 4 * ((size_t)C + 1), st));
  HIPTRY(dev_upload(b_camimgs, pb.cam_imgs.data(), 4 * pb.cam_imgs.size(), st));
  HIPTRY(dev_upload(b_imgcam, img_cam.data(), 4 * (size_t)N, st));
  HIPTRY(dev_upload(b_campoff, pb.cam_poff.data(), 4 * ((size_t)C + 1), st));
  HIPTRY(dev_upload(b_camfoff, pb.cam_foff.data(), 4 * (size_t)C, st));
  HIPTRY(dev_upload(b_cammoff, pb.cam_moff.data(), 4 * (size_t)C, st));
  HIPTRY(dev_upload(b_oxy, pb.o_xy.data(), 16 * (size_t)n_obs, st));
  HIPTRY(dev_upload(b_cpose, pb.cpose.data(), N, st));
  HIPTRY(dev_upload(b_mask, pb.mask.data(), N, st));
  HIPTRY(dev_upload(b_ptvar, pb.pt_var.data(), P, st));
  HIPTRY(dev_upload(b_cammodel, cam_model.data(), 4 * (size_t)C, st));
  HIPTRY(dev_upload(b_camnp, pb.cam_np.data(), 4 * (size_t)C, st));
  HIPTRY(dev_upload(b_camk, pb.cam_k.data(), 4 * (size_t)C, st));
  HIPTRY(dev_upload(b_camfree, pb.cam_free.data(), 4 * pb.cam_free.size(), st));
  HIPTRY(dev_upload(b_q, q.data(), 32 * (size_t)N, st));
  HIPTRY(dev_upload(b_t, image_tvec, 24 * (size_t)N, st));
  HIPTRY(dev_upload(b_X, X.data(), 24 * (size_t)P, st));
  HIPTRY(dev_upload(b_prm, camera_params, 8 * (size_t)n_prm, st));
  alloc(b_cq, 32 * (size_t)N);
  alloc(b_ct, 24 * (size_t)N);
  alloc(b_cX, 24 * (size_t)P);
  alloc(b_cprm, 8 * (size_t)n_prm);
  alloc(b_J, 8 * (size_t)BA_JS * n_obs);
  alloc(b_y, 16 * (size_t)n_obs);
  for (DevBuf* b : {&b_ge, &b_cne, &b_se, &b_De, &b_ve, &b_zp, &b_dy}) alloc(*b, 24 * (size_t)P);
  alloc(b_Cinv, 72 * (size_t)P);
  for (DevBuf* b : {&b_gf, &b_cnf, &b_sf, &b_Df, &b_ddf, &b_b, &b_x, &b_r, &b_z, &b_p, &b_qv, &b_tmp}) alloc(*b, 8 * nfa);
  alloc(b_Minv, 8 * ((size_t)pb.n_minv + 1));
  alloc(b_icam, 8 * (size_t)BA_ICAM * N);
  alloc(b_Pc, 16 * (size_t)nb_obs);
  alloc(b_Pm, 8 * (size_t)std::max(nb_obs, nb_fpart));
  alloc(b_Pg, 8 * (size_t)n_gparts);
  alloc(b_Pe, 16 * (size_t)nb_pts);
  alloc(b_Pd, 8 * std::max<size_t>((size_t)N + C, 2 * (size_t)nb_fpart));
  alloc(b_Pq, 8 * (size_t)nb_fpart);
  alloc(b_ctl, sizeof(BaCtl));
  const int max_iter = o.max_num_iterations;
  if (trace) alloc(b_trace, 8 * (size_t)DSM_BA_TRACE_COLUMNS * ((size_t)max_iter + 1));
  HIPTRY(ev.create());
  BaCtl init{};
  tr_init(&init, kTrInitialRadius);
  init.m_cg = INFINITY;
  HIPTRY(dev_upload(b_ctl, &init, sizeof(BaCtl), st));

  BaDev d{};
  d.n_obs = n_obs; d.n_pts = P; d.n_img = N; d.n_cam = C; d.nf = nf;
  d.max_cg = o.max_linear_solver_iterations;
  d.tr = tr_ceres_defaults();
  d.tr.max_iterations = max_iter; d.tr.max_consecutive_invalid_steps = o.max_num_consecutive_invalid_steps;
  d.tr.gtol = o.gradient_tolerance; d.tr.ftol = o.function_tolerance; d.tr.ptol = o.parameter_tolerance;
  d.o_img = b_oimg.as<uint32_t>(); d.o_pt = b_opt.as<uint32_t>(); d.o_run = b_orun.as<uint32_t>(); d.img_off = b_imgoff.as<uint32_t>();
  d.trk_off = b_trkoff.as<uint32_t>(); d.trk = b_trk.as<uint32_t>(); d.cam_img_off = b_camimgoff.as<uint32_t>();
  d.cam_imgs = b_camimgs.as<uint32_t>(); d.img_cam = b_imgcam.as<uint32_t>(); d.cam_poff = b_campoff.as<uint32_t>();
  d.cam_foff = b_camfoff.as<uint32_t>(); d.cam_moff = b_cammoff.as<uint32_t>(); d.o_xy = b_oxy.as<double>();
  d.img_cpose = b_cpose.as<uint8_t>(); d.img_mask = b_mask.as<uint8_t>(); d.pt_var = b_ptvar.as<uint8_t>();
  d.cam_model = b_cammodel.as<int>(); d.cam_np = b_camnp.as<int>(); d.cam_k = b_camk.as<int>(); d.cam_free = b_camfree.as<int>();
  d.q = b_q.as<double>(); d.t = b_t.as<double>(); d.X = b_X.as<double>(); d.prm = b_prm.as<double>();
  d.cq = b_cq.as<double>(); d.ct = b_ct.as<double>(); d.cX = b_cX.as<double>(); d.cprm = b_cprm.as<double>();
  d.J = b_J.as<double>(); d.y = b_y.as<double>();
  d.ge = b_ge.as<double>(); d.cne = b_cne.as<double>(); d.se = b_se.as<double>(); d.De = b_De.as<double>(); d.Cinv = b_Cinv.as<double>();
  d.ve = b_ve.as<double>(); d.zp = b_zp.as<double>(); d.dy = b_dy.as<double>();
  d.gf = b_gf.as<double>(); d.cnf = b_cnf.as<double>(); d.sf = b_sf.as<double>(); d.Df = b_Df.as<double>(); d.ddf = b_ddf.as<double>();
  d.Minv = b_Minv.as<double>(); d.b = b_b.as<double>(); d.x = b_x.as<double>(); d.r = b_r.as<double>(); d.z = b_z.as<double>();
  d.p = b_p.as<double>(); d.qv = b_qv.as<double>(); d.tmp = b_tmp.as<double>(); d.icam = b_icam.as<double>();
  d.Pc = b_Pc.as<double>(); d.Pm = b_Pm.as<double>(); d.Pg = b_Pg.as<double>(); d.Pe = b_Pe.as<double>(); d.Pd = b_Pd.as<double>();
  d.Pq = b_Pq.as<double>(); d.ctl = b_ctl.as<BaCtl>(); d.trace = trace ? b_trace.as<double>() : nullptr;
  const double setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();

  const dim3 B(BA_B), W(BA_W);
  // the Jacobian pipeline: evaluation, gradient and column norms, scaling (gate: only after an accepted step)
  auto jacobian = [&](int first) {
    const int gate = first ? 0 : 1;
    hipLaunchKernelGGL(k_ba_eval, dim3(nb_obs), B, 0, st, d, first ? 0 : 2);
    if (first) hipLaunchKernelGGL(k_ba_fin_cost, dim3(1), B, 0, st, d, nb_obs, 0);
    hipLaunchKernelGGL(k_ba_grad_pts, dim3(nb_pts), B, 0, st, d, gate);
    if (N) hipLaunchKernelGGL(k_ba_grad_img, dim3(N), W, 0, st, d, gate, nb_pts);
    if (C) hipLaunchKernelGGL(k_ba_grad_cam, dim3(C), W, 0, st, d, gate, nb_pts + N);
    hipLaunchKernelGGL(k_ba_scale_cols, dim3(nb_cols), B, 0, st, d, first, gate);
    hipLaunchKernelGGL(k_ba_scale_J, dim3(nb_obs), B, 0, st, d, gate);
    hipLaunchKernelGGL(k_ba_finalize, dim3(1), B, 0, st, d, n_gparts, first);
  };
  auto Sv = [&](const double* v, double* out, int k) {
    hipLaunchKernelGGL(k_ba_Fv, dim3(nb_obs), B, 0, st, d, v, k);
    hipLaunchKernelGGL(k_ba_Ey, dim3(nb_pts), B, 0, st, d, k);
    hipLaunchKernelGGL(k_ba_Sv_img, dim3(N), W, 0, st, d, v, out, k);
    if (C) hipLaunchKernelGGL(k_ba_Sv_cam, dim3(C), W, 0, st, d, v, out, k);
  };
  float ms_jac = 0.f, ms_cg = 0.f, ms_cand = 0.f, ms_total = 0.f;
  BaCtl h{};
  if (rc == DSM_OK) {
    HIPTRY(hipEventRecord(ev[0], st));
    jacobian(1);
    HIPTRY(hipGetLastError());  // a launch that failed to start
    HIPTRY(hipEventRecord(ev[1], st));
    HIPTRY(hipMemcpyAsync(&h, d.ctl, sizeof(BaCtl), hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    if (rc == DSM_OK) {
      double ms = 0;
      HIPTRY(ev.ms(0, 1, &ms));
      ms_jac += ms;
      ms_total += ms;
      if (!std::isfinite(h.cost)) {  // the initial evaluation failed
        h.term = DSM_BA_FAILURE;
        h.done = 1;
      }
    }
  }
  const double initial_cost = h.cost, initial_reproj = h.reproj;
  while (rc == DSM_OK && !h.done) {
    HIPTRY(hipEventRecord(ev[2], st));
    hipLaunchKernelGGL(k_ba_prep_pts, dim3(nb_pts), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_prep_img, dim3(N), W, 0, st, d);
    if (C) hipLaunchKernelGGL(k_ba_prep_cam, dim3(C), W, 0, st, d);
    hipLaunchKernelGGL(k_ba_cg_init, dim3(nb_f), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_cg_init_fin, dim3(1), B, 0, st, d, nb_f);
    if (nf)
      for (int k = 1; k <= o.max_linear_solver_iterations; ++k) {
        hipLaunchKernelGGL(k_ba_cg_z, dim3(nb_blk), B, 0, st, d, k);
        hipLaunchKernelGGL(k_ba_cg_fin_rz, dim3(1), B, 0, st, d, nb_blk, k);
        hipLaunchKernelGGL(k_ba_cg_p, dim3(nb_f), B, 0, st, d, k);
        Sv(d.p, d.qv, k);
        hipLaunchKernelGGL(k_ba_cg_fin_pq, dim3(1), B, 0, st, d, k);
        const int reset = k % 10 == 0;
        hipLaunchKernelGGL(k_ba_cg_x, dim3(nb_f), B, 0, st, d, k, reset);
        if (reset) {
          Sv(d.x, d.tmp, k);
          hipLaunchKernelGGL(k_ba_cg_reset, dim3(nb_f), B, 0, st, d, k);
        }
        hipLaunchKernelGGL(k_ba_cg_fin_q, dim3(1), B, 0, st, d, nb_f, k);
      }
    HIPTRY(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k_ba_Fv, dim3(nb_obs), B, 0, st, d, (const double*)d.x, 0);
    hipLaunchKernelGGL(k_ba_backsub, dim3(nb_pts), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_cand_f, dim3(nb_ent), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_mcc, dim3(nb_obs), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_eval, dim3(nb_obs), B, 0, st, d, 1);
    hipLaunchKernelGGL(k_ba_fin_cost, dim3(1), B, 0, st, d, nb_obs, 1);
    hipLaunchKernelGGL(k_ba_decide, dim3(1), B, 0, st, d, nb_obs, nb_pts, nb_ent);
    hipLaunchKernelGGL(k_ba_commit, dim3(nb_commit), B, 0, st, d);
    hipLaunchKernelGGL(k_ba_commit_prm, dim3((n_prm + BA_B - 1) / BA_B + 1), B, 0, st, d, n_prm);
    HIPTRY(hipEventRecord(ev[4], st));
    jacobian(0);
    HIPTRY(hipGetLastError());
    HIPTRY(hipEventRecord(ev[5], st));
    HIPTRY(hipMemcpyAsync(&h, d.ctl, sizeof(BaCtl), hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    if (rc != DSM_OK) break;
    double a = 0, b2 = 0, c2 = 0;
    HIPTRY(ev.ms(2, 3, &a));
    HIPTRY(ev.ms(3, 4, &b2));
    HIPTRY(ev.ms(4, 5, &c2));
    ms_cg += a;
    ms_cand += b2;
    ms_jac += c2;
    ms_total += a + b2 + c2;
  }
  if (rc == DSM_OK) {
    std::vector<double> Xo(3 * (size_t)P), qo(4 * (size_t)N), to(3 * (size_t)N), po(n_prm);
    HIPTRY(hipMemcpyAsync(Xo.data(), d.X, 24 * (size_t)P, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(qo.data(), d.q, 32 * (size_t)N, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(to.data(), d.t, 24 * (size_t)N, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(po.data(), d.prm, 8 * (size_t)n_prm, hipMemcpyDeviceToHost, st));
    std::vector<double> tr;
    if (trace) {
      tr.resize((size_t)DSM_BA_TRACE_COLUMNS * (h.iter + 1));
      HIPTRY(hipMemcpyAsync(tr.data(), d.trace, 8 * tr.size(), hipMemcpyDeviceToHost, st));
    }
    HIPTRY(hipStreamSynchronize(st));
    if (rc == DSM_OK) {
      for (uint32_t r = 0; r < P; ++r)
        for (int m = 0; m < 3; ++m) point_xyz[3 * (size_t)order[r] + m] = Xo[3 * (size_t)r + m];
      for (uint32_t i = 0; i < N; ++i) {  // images and cameras outside the problem keep their bits
        for (int m = 0; m < 4; ++m) out_qvec[4 * (size_t)iorder[i] + m] = qo[4 * (size_t)i + m];
        for (int m = 0; m < 3; ++m) out_tvec[3 * (size_t)iorder[i] + m] = to[3 * (size_t)i + m];
      }
      for (uint32_t c = 0; c < C; ++c) std::copy(po.begin() + poff[c], po.begin() + poff[c + 1], out_params + poff_in[corder[c]]);
      if (trace) std::copy(tr.begin(), tr.end(), trace);
      if (report) {
        dsm_bundle_adjustment_report rep{};
        rep.termination = h.term;
        rep.num_iterations = h.iter;
        rep.num_successful_steps = h.n_succ;
        rep.num_invalid_steps = h.n_invalid_total;
        rep.num_residuals = 2 * (uint64_t)n_obs;
        rep.num_effective_parameters = pb.n_eff;
        rep.total_cg_iterations = h.cg_total;
        rep.initial_cost = initial_cost;
        rep.final_cost = h.cost;
        rep.initial_mean_reprojection_error = initial_reproj;
        rep.final_mean_reprojection_error = h.reproj;
        // the shared state starts its margins at infinity; this report's largest value is DBL_MAX
        rep.min_rho_margin = std::min(h.m_accept, DBL_MAX);
        rep.min_cg_margin = std::min(h.m_cg, DBL_MAX);
        rep.min_gradient_margin = std::min(h.m_grad, DBL_MAX);
        rep.setup_ms = setup_ms;
        rep.jacobian_ms = ms_jac;
        rep.cg_ms = ms_cg;
        rep.candidate_ms = ms_cand;
        rep.total_ms = ms_total;
        *report = rep;
      }
    }
  }
  return rc;
}
