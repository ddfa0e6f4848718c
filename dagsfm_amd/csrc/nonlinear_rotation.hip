// nonlinear_rotation.hip -- the NONLINEAR global rotation estimator on the device.
//   DistributedMapperController::GlobalRotationAveraging   src/controllers/distributed_mapper_controller.cpp:945-1008 (:969-986)
//   NonlinearRotationEstimator::EstimateRotations          src/rotation_estimation/nonlinear_rotation_estimator.cpp:82-131
//   PairwiseRotationError                                  src/rotation_estimation/pairwise_rotation_error.h:98-128
// One residual block per edge of the first component: r = RotationMatrixToAngleAxis(R(a_j) R(a_i)^T R(a_12)^T), differentiated
// by forward-mode dual numbers through ceres' conversions (rotation_ceres.h), under ceres::SoftLOneLoss and ceres' corrector.
// The minimizer is ceres' Levenberg-Marquardt as DESIGN.md 12 states it (Jacobi scaling, D = clamp(diag J^T J), the step
// rules and their order: trust_region.h), without a Schur complement: (J^T J + D / radius) step = -g is solved by a
// conjugate gradient preconditioned by the exact 3 x 3 diagonal blocks, x0 = 0, to a relative residual of cg_tolerance
// (1e-14).
//
// Layout.  Vectors over images are [N][3]; an edge record is NL_EDGE doubles: the corrected residual r[3], the corrected
// Jacobian blocks with respect to image 1 and image 2 (3 x 3 row-major each, unscaled), rho(s).  There are two edge buffers:
// the candidate of every step is linearised where its cost is evaluated, into the buffer that is not current, and an
// accepted step only flips ctl.cur.  Every sum over edges is a gather over the image's CSR row (sorted by neighbour), the
// operator recomputes J_e p per row entry instead of reading a per-edge product (one launch less per CG iteration), and every
// scalar is per-block partials summed by one fixed tree (block_reduce.h): no floating-point atomics, the same bytes from run
// to run and for every order of the input list.
//
// Loop control stays on the device.  One LM iteration is enqueued whole: the preconditioner and CG start, a budget of CG
// iterations of two launches each that are no-ops past ctl.cg_stop, the step, the candidate, one thread's decision, and the
// commit with the new gradient (no-ops unless accepted).  The host reads the control block once per LM iteration; only a
// solve that outlasts the budget is continued (the tail kernels are no-ops while the solve runs), so the budget changes the
// number of no-op launches and never a result.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "block_reduce.h"
#include "ctx.h"
#include "graph_edges.h"
#include "rotation_ceres.h"
#include "rotation_graph.h"
#include "trust_region.h"

namespace {

constexpr int NL_EDGE = 22;               // r[3], J1[9], J2[9], rho(s)
constexpr int NL_LINEAR_SOLVER_FAILED = 3;  // internal, beside TR_*: a CG solve ended above cg_max_residual

// device-side loop state; every field has one writer per launch (thread 0 of block 0).  No kernel reads a value that is
// written in the same launch, with one exception: cg_stop, which k_nl_cg_ap(k) and k_nl_step(k) may set to k while other
// blocks of that launch read it at their entry (nl_block_read).  Such a block sees INT_MAX or k; with INT_MAX it repeats the
// stop test on the same partials and ends the same way, with k it returns at once: both are the ended solve, and nothing else
// depends on which one it saw.
struct NlCtl : TrState {  // accepted: the last step was accepted (or this is iteration 0), so the gradient is fresh
  int cur;        // the edge buffer that holds the linearisation of the accepted state
  int cg_stop;    // CG iterations k >= cg_stop are no-ops (INT_MAX while the solve runs)
  int cg_done;    // the solve of this LM iteration has ended: the tail may run
  int cg_last;    // its iterations
  int pending;    // a decision was taken and its trace row is not written yet
  double initial_cost;
  double rz[2];   // r.z of CG iteration k at [k & 1]
  double bb;      // ||b||^2 of the running solve
  double last_resid, cg_worst;
  unsigned long long cg_total;
};

struct NlOpt {
  double loss_b;  // robust_loss_width^2
  double min_diag, max_diag, cg_tol, cg_max_resid;
  int cg_max;
  TrOptions tr;
};

// the entry test of every kernel of the loop; the running loop is the path that falls through
#define nl_ended(ctl) __builtin_expect((ctl)->done, 0)

// a control word that thread 0 of block 0 may write later in the same launch, read once per block: every thread of a block
// takes the same path to the barriers that follow
__device__ inline int nl_block_read(const int* word) {
  __shared__ int w;
  if (threadIdx.x == 0) w = *(const volatile int*)word;
  __syncthreads();
  return w;
}

// ---------------------------------------------------------------- the residual block
// PairwiseRotationError::operator() over dual numbers seeded on the two orientations, ceres::SoftLOneLoss(a) with b = a^2
// (rho = 2 b (sqrt(1 + s / b) - 1), rho' = max(DBL_MIN, 1 / sqrt(1 + s / b)), rho'' = -rho' / (2 b (1 + s / b)) < 0) and ceres'
// Corrector, which for rho'' <= 0 scales the residual and the Jacobian by sqrt(rho').  rec: an edge record.
__device__ inline void nl_edge_eval(const double* a1, const double* a2, const double* a12, double loss_b, double* rec, double* rho3) {
  typedef RotDual<6> T;
  T w1[3], w2[3], M1[9], M2[9], L[9], E[9], q[4], aa[3];
  for (int c = 0; c < 3; ++c) {
    w1[c] = rd_const<6>(a1[c]);
    w1[c].d[c] = 1.0;
    w2[c] = rd_const<6>(a2[c]);
    w2[c].d[3 + c] = 1.0;
  }
  double M12[9];
  ceres_angle_axis_to_rotation(w1, M1);
  ceres_angle_axis_to_rotation(w2, M2);
  ceres_angle_axis_to_rotation(a12, M12);
  for (int i = 0; i < 3; ++i)  // loop = R2 R1^T
    for (int j = 0; j < 3; ++j) L[i * 3 + j] = M2[i * 3] * M1[j * 3] + M2[i * 3 + 1] * M1[j * 3 + 1] + M2[i * 3 + 2] * M1[j * 3 + 2];
  for (int i = 0; i < 3; ++i)  // err = loop R12^T
    for (int j = 0; j < 3; ++j) E[i * 3 + j] = L[i * 3] * M12[j * 3] + L[i * 3 + 1] * M12[j * 3 + 1] + L[i * 3 + 2] * M12[j * 3 + 2];
  ceres_rotation_to_quaternion(E, q);
  ceres_quaternion_to_angle_axis(q, aa);
  const double s = aa[0].v * aa[0].v + aa[1].v * aa[1].v + aa[2].v * aa[2].v;
  const double sum = 1.0 + s / loss_b;
  const double tmp = sqrt(sum);
  const double rho0 = 2.0 * loss_b * (tmp - 1.0);
  const double rho1 = fmax(DBL_MIN, 1.0 / tmp);
  const double rho2 = -(rho1 / loss_b) / (2.0 * sum);
  const double scale = sqrt(rho1);  // Corrector: sq_norm == 0 or rho'' <= 0 -> residual_scaling = sqrt(rho'), alpha_sq_norm = 0
  for (int r = 0; r < 3; ++r) {
    rec[r] = scale * aa[r].v;
    for (int c = 0; c < 3; ++c) {
      rec[3 + r * 3 + c] = scale * aa[r].d[c];
      rec[12 + r * 3 + c] = scale * aa[r].d[3 + c];
    }
  }
  rec[21] = rho0;
  if (rho3) {
    rho3[0] = rho0;
    rho3[1] = rho1;
    rho3[2] = rho2;
  }
}

__global__ void __launch_bounds__(RA_BLOCK) k_nl_debug(uint32_t n, const double* __restrict__ a1, const double* __restrict__ a2,
                                                       const double* __restrict__ a12, double loss_b, double* __restrict__ res,
                                                       double* __restrict__ jac, double* __restrict__ rho) {
  const uint32_t e = blockIdx.x * RA_BLOCK + threadIdx.x;
  if (e >= n) return;
  double rec[NL_EDGE], rho3[3];
  nl_edge_eval(a1 + 3 * (size_t)e, a2 + 3 * (size_t)e, a12 + 3 * (size_t)e, loss_b, rec, rho3);
  for (int c = 0; c < 3; ++c) {
    res[3 * (size_t)e + c] = rec[c];
    rho[3 * (size_t)e + c] = rho3[c];
  }
  for (int c = 0; c < 18; ++c) jac[18 * (size_t)e + c] = rec[3 + c];
}

// ---------------------------------------------------------------- per-edge kernel
// mode 0: the start (the candidate is R itself, into the current buffer).  mode 1: the candidate R + s x of the finished
// solve, into the other buffer, and the model cost change -(J step).(r + J step / 2) of the current linearisation.
// Partials: the candidate's cost 1/2 rho(s), the model cost change.
__global__ void __launch_bounds__(RA_BLOCK) k_nl_edges(uint32_t M, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej,
                                                       const double* __restrict__ r12, const double* __restrict__ R,
                                                       const double* __restrict__ x, const double* __restrict__ sc, double loss_b,
                                                       const NlCtl* ctl, int mode, double* __restrict__ E0, double* __restrict__ E1,
                                                       double* __restrict__ P) {
  if (mode && (nl_ended(ctl) || !ctl->cg_done)) return;
  __shared__ double sh[2 * RA_BLOCK];
  const int cur = ctl->cur;
  const double* Ecur = cur ? E1 : E0;
  double* Eout = mode ? (cur ? E0 : E1) : (cur ? E1 : E0);
  const uint32_t e = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (e < M) {
    const size_t i3 = 3 * (size_t)ei[e], j3 = 3 * (size_t)ej[e];
    double c1[3], c2[3];
    for (int c = 0; c < 3; ++c) {
      c1[c] = R[i3 + c];
      c2[c] = R[j3 + c];
    }
    if (mode) {
      const double* rec = Ecur + (size_t)NL_EDGE * e;
      double d1[3], d2[3];
      for (int c = 0; c < 3; ++c) {
        d1[c] = sc[i3 + c] * x[i3 + c];
        d2[c] = sc[j3 + c] * x[j3 + c];
        c1[c] += d1[c];
        c2[c] += d2[c];
      }
      double m = 0.0;
      for (int r = 0; r < 3; ++r) {
        const double js = (rec[3 + r * 3] * d1[0] + rec[3 + r * 3 + 1] * d1[1] + rec[3 + r * 3 + 2] * d1[2]) +
                          (rec[12 + r * 3] * d2[0] + rec[12 + r * 3 + 1] * d2[1] + rec[12 + r * 3 + 2] * d2[2]);
        m += js * (rec[r] + js / 2.0);
      }
      acc[1] = -m;
    }
    double rec[NL_EDGE];
    nl_edge_eval(c1, c2, r12 + 3 * (size_t)e, loss_b, rec, nullptr);
    double* out = Eout + (size_t)NL_EDGE * e;
    for (int c = 0; c < NL_EDGE; ++c) out[c] = rec[c];
    acc[0] = 0.5 * rec[21];
  }
  write_partials<RA_BLOCK, 2>(acc, sh, P);
}

// ---------------------------------------------------------------- per-image kernels (gathers over the CSR row)
// CSR: image v has entries p in [off[v], off[v + 1]) sorted by neighbour nb[p]; ce[p] = 2 * edge + (v is the edge's image 2)

// Commit and linearise.  mode 0: the start (also the Jacobi scaling s = 1 / (1 + |column|), kept for the whole run).  mode 1:
// a no-op unless the step was accepted; R += s x, then from the (now current) edge buffer: the column norms, D = clamp(s^2
// |column|^2), the scaled gradient, the scaled diagonal block of J^T J.  Partials: the max-norm of the unscaled gradient.
__global__ void __launch_bounds__(RA_BLOCK) k_nl_linearize(uint32_t N, const uint32_t* __restrict__ off, const uint32_t* __restrict__ ce,
                                                           const double* __restrict__ E0, const double* __restrict__ E1,
                                                           const double* __restrict__ x, double* __restrict__ R, double* __restrict__ sc,
                                                           double* __restrict__ D, double* __restrict__ gs, double* __restrict__ B,
                                                           const NlCtl* ctl, int mode, NlOpt o, double* __restrict__ Pg) {
  if (nl_ended(ctl) || (mode && (!ctl->pending || !ctl->accepted))) return;
  __shared__ double sh[RA_BLOCK];
  const double* E = ctl->cur ? E1 : E0;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double gmax = 0.0;
  if (v < N) {
    const size_t v3 = 3 * (size_t)v;
    if (mode)
      for (int c = 0; c < 3; ++c) R[v3 + c] += sc[v3 + c] * x[v3 + c];
    double cn[3] = {0, 0, 0}, g[3] = {0, 0, 0}, b[6] = {0, 0, 0, 0, 0, 0};  // b: 00 01 02 11 12 22
    for (uint32_t p = off[v]; p < off[v + 1]; ++p) {
      const double* rec = E + (size_t)NL_EDGE * (ce[p] >> 1);
      const double* J = rec + 3 + 9 * (ce[p] & 1);
      for (int c = 0; c < 3; ++c) {
        cn[c] += (J[c] * J[c] + J[3 + c] * J[3 + c]) + J[6 + c] * J[6 + c];
        g[c] += (J[c] * rec[0] + J[3 + c] * rec[1]) + J[6 + c] * rec[2];
      }
      b[0] += (J[0] * J[0] + J[3] * J[3]) + J[6] * J[6];
      b[1] += (J[0] * J[1] + J[3] * J[4]) + J[6] * J[7];
      b[2] += (J[0] * J[2] + J[3] * J[5]) + J[6] * J[8];
      b[3] += (J[1] * J[1] + J[4] * J[4]) + J[7] * J[7];
      b[4] += (J[1] * J[2] + J[4] * J[5]) + J[7] * J[8];
      b[5] += (J[2] * J[2] + J[5] * J[5]) + J[8] * J[8];
    }
    double s[3];
    for (int c = 0; c < 3; ++c) {
      if (mode == 0) sc[v3 + c] = 1.0 / (1.0 + sqrt(cn[c]));
      s[c] = sc[v3 + c];
      D[v3 + c] = fmin(fmax(s[c] * s[c] * cn[c], o.min_diag), o.max_diag);
      gs[v3 + c] = s[c] * g[c];
      gmax = fmax(gmax, fabs(g[c]));
    }
    double* Bv = B + 6 * (size_t)v;
    Bv[0] = s[0] * s[0] * b[0];
    Bv[1] = s[0] * s[1] * b[1];
    Bv[2] = s[0] * s[2] * b[2];
    Bv[3] = s[1] * s[1] * b[3];
    Bv[4] = s[1] * s[2] * b[4];
    Bv[5] = s[2] * s[2] * b[5];
  }
  const double m = block_max<RA_BLOCK>(gmax, sh);
  if (threadIdx.x == 0) Pg[blockIdx.x] = m;
}

// z = Minv r for the symmetric 3 x 3 inverse Minv (00 01 02 11 12 22)
__device__ inline void nl_apply_minv(const double* Mi, const double* r, double* z) {
  z[0] = (Mi[0] * r[0] + Mi[1] * r[1]) + Mi[2] * r[2];
  z[1] = (Mi[1] * r[0] + Mi[3] * r[1]) + Mi[4] * r[2];
  z[2] = (Mi[2] * r[0] + Mi[4] * r[1]) + Mi[5] * r[2];
}

// CG start of one LM iteration: lm = (sqrt(D / radius))^2, the preconditioner (B + diag lm)^-1, b = -gs, x = 0, r = b, z = Minv r.
// Partials: r.z, r.r into the parity-0 buffer.
__global__ void __launch_bounds__(RA_BLOCK) k_nl_cg_init(uint32_t N, const double* __restrict__ D, const double* __restrict__ gs,
                                                         const double* __restrict__ B, double* __restrict__ lm, double* __restrict__ Minv,
                                                         double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                         NlCtl* ctl, double* __restrict__ Pz) {
  if (nl_ended(ctl)) return;
  __shared__ double sh[2 * RA_BLOCK];
  const double radius = ctl->radius;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (v < N) {
    const size_t v3 = 3 * (size_t)v;
    double l[3], rv[3], zv[3];
    for (int c = 0; c < 3; ++c) {
      const double t = sqrt(D[v3 + c] / radius);
      l[c] = t * t;
      lm[v3 + c] = l[c];
      rv[c] = -gs[v3 + c];
    }
    const double* Bv = B + 6 * (size_t)v;
    const double a00 = Bv[0] + l[0], a01 = Bv[1], a02 = Bv[2], a11 = Bv[3] + l[1], a12 = Bv[4], a22 = Bv[5] + l[2];
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    double* Mi = Minv + 6 * (size_t)v;
    Mi[0] = c00 / det;
    Mi[1] = c01 / det;
    Mi[2] = c02 / det;
    Mi[3] = (a00 * a22 - a02 * a02) / det;
    Mi[4] = (a01 * a02 - a00 * a12) / det;
    Mi[5] = (a00 * a11 - a01 * a01) / det;
    nl_apply_minv(Mi, rv, zv);
    for (int c = 0; c < 3; ++c) {
      x[v3 + c] = 0.0;
      r[v3 + c] = rv[c];
      z[v3 + c] = zv[c];
      acc[0] += rv[c] * zv[c];
      acc[1] += rv[c] * rv[c];
    }
  }
  write_partials<RA_BLOCK, 2>(acc, sh, Pz);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    ctl->cg_stop = INT_MAX;
    ctl->cg_done = 0;
  }
}

// whether the solve has ended before iteration k, from the partials of (r.z, r.r) that iteration k - 1 (or the start) left;
// every block computes the same answer from the same bytes.  A non-finite residual ends the solve (and fails the call).
__device__ inline bool nl_cg_ended(const double* __restrict__ Pz, int nb, int k, const NlCtl* ctl, double tol, int cg_max, double* sh,
                                   double* rz, double* bb, double* rel) {
  double s[2];
  sum_partials<RA_BLOCK, 2>(Pz, nb, s, sh);
  *rz = s[0];
  *bb = k == 0 ? s[1] : ctl->bb;
  *rel = *bb > 0.0 ? sqrt(s[1] / *bb) : 0.0;
  return !(*rel > tol) || k >= cg_max;
}
__device__ inline void nl_cg_record_end(NlCtl* ctl, int k, double rel) {
  if (ctl->cg_stop != INT_MAX) return;
  ctl->cg_stop = k;
  ctl->cg_last = k;
  ctl->cg_total += (unsigned long long)k;
  ctl->last_resid = rel;
  ctl->cg_worst = rel > ctl->cg_worst || !(rel == rel) ? rel : ctl->cg_worst;
}

// CG iteration k, part 1: the stop test, beta = rz_k / rz_{k-1}, p_k = z + beta p_{k-1} (written for this image, recomputed
// for its neighbours: the same bytes), q = (Js^T Js + lm) p_k with J_e p recomputed per row entry.  Partials: p.q
__global__ void __launch_bounds__(RA_BLOCK) k_nl_cg_ap(uint32_t N, int nbv, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nb,
                                                       const uint32_t* __restrict__ ce, const double* __restrict__ E0,
                                                       const double* __restrict__ E1, const double* __restrict__ sc,
                                                       const double* __restrict__ lm, const double* __restrict__ z,
                                                       const double* __restrict__ pold, double* __restrict__ pnew, double* __restrict__ q,
                                                       NlCtl* ctl, int k, double tol, int cg_max, const double* __restrict__ Pz,
                                                       double* __restrict__ Pq) {
  if (nl_ended(ctl) || k >= nl_block_read(&ctl->cg_stop)) return;
  __shared__ double sh[2 * RA_BLOCK];
  double rz, bb, rel;
  const bool ended = nl_cg_ended(Pz, nbv, k, ctl, tol, cg_max, sh, &rz, &bb, &rel);
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (ended) {
    if (writer) nl_cg_record_end(ctl, k, rel);
    return;
  }
  const double beta = k == 0 ? 0.0 : rz / ctl->rz[(k - 1) & 1];
  if (writer) {
    ctl->rz[k & 1] = rz;
    if (k == 0) ctl->bb = bb;
  }
  const double* E = ctl->cur ? E1 : E0;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[1] = {0.0};
  if (v < N) {
    const size_t v3 = 3 * (size_t)v;
    double pv[3], spv[3], a[3] = {0, 0, 0};
    for (int c = 0; c < 3; ++c) {
      pv[c] = k == 0 ? z[v3 + c] : z[v3 + c] + beta * pold[v3 + c];
      pnew[v3 + c] = pv[c];
      spv[c] = sc[v3 + c] * pv[c];
    }
    for (uint32_t p = off[v]; p < off[v + 1]; ++p) {
      const size_t u3 = 3 * (size_t)nb[p];
      const int side = ce[p] & 1;
      const double* rec = E + (size_t)NL_EDGE * (ce[p] >> 1);
      const double* Jv = rec + 3 + 9 * side;
      const double* Ju = rec + 3 + 9 * (1 - side);
      double spu[3], t[3];
      for (int c = 0; c < 3; ++c) spu[c] = sc[u3 + c] * (k == 0 ? z[u3 + c] : z[u3 + c] + beta * pold[u3 + c]);
      for (int r = 0; r < 3; ++r)
        t[r] = ((Jv[r * 3] * spv[0] + Jv[r * 3 + 1] * spv[1]) + Jv[r * 3 + 2] * spv[2]) +
               ((Ju[r * 3] * spu[0] + Ju[r * 3 + 1] * spu[1]) + Ju[r * 3 + 2] * spu[2]);
      for (int c = 0; c < 3; ++c) a[c] += (Jv[c] * t[0] + Jv[3 + c] * t[1]) + Jv[6 + c] * t[2];
    }
    for (int c = 0; c < 3; ++c) {
      const double qc = sc[v3 + c] * a[c] + lm[v3 + c] * pv[c];
      q[v3 + c] = qc;
      acc[0] += pv[c] * qc;
    }
  }
  write_partials<RA_BLOCK, 1>(acc, sh, Pq);
}

// CG iteration k, part 2: alpha = rz_k / p.q (every block sums the same partials), x += alpha p, r -= alpha q, z = Minv r.
// Partials: r.z, r.r for iteration k + 1
__global__ void __launch_bounds__(RA_BLOCK) k_nl_cg_xr(uint32_t N, int nbv, const double* __restrict__ Pq, const double* __restrict__ Minv,
                                                       const double* __restrict__ p, const double* __restrict__ q, double* __restrict__ x,
                                                       double* __restrict__ r, double* __restrict__ z, const NlCtl* ctl, int k,
                                                       double* __restrict__ Pz) {
  if (nl_ended(ctl) || k >= ctl->cg_stop) return;
  __shared__ double sh[2 * RA_BLOCK];
  double pq[1];
  sum_partials<RA_BLOCK, 1>(Pq, nbv, pq, sh);
  const double alpha = ctl->rz[k & 1] / pq[0];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (v < N) {
    const size_t v3 = 3 * (size_t)v;
    double rv[3], zv[3];
    for (int c = 0; c < 3; ++c) {
      x[v3 + c] += alpha * p[v3 + c];
      rv[c] = r[v3 + c] - alpha * q[v3 + c];
      r[v3 + c] = rv[c];
    }
    nl_apply_minv(Minv + 6 * (size_t)v, rv, zv);
    for (int c = 0; c < 3; ++c) {
      z[v3 + c] = zv[c];
      acc[0] += rv[c] * zv[c];
      acc[1] += rv[c] * rv[c];
    }
  }
  write_partials<RA_BLOCK, 2>(acc, sh, Pz);
}

// The end of the enqueued CG iterations (k_end is the first one not enqueued): the stop test once more, then, if the solve has
// ended, the partials of |s x|^2 and |R|^2 (the parameter tolerance).  While the solve still runs this is a no-op and the
// host enqueues more iterations.
__global__ void __launch_bounds__(RA_BLOCK) k_nl_step(uint32_t N, int nbv, const double* __restrict__ R, const double* __restrict__ x,
                                                      const double* __restrict__ sc, NlCtl* ctl, int k_end, double tol, int cg_max,
                                                      const double* __restrict__ Pz, double* __restrict__ Pv) {
  if (nl_ended(ctl)) return;
  __shared__ double sh[2 * RA_BLOCK];
  const bool writer = blockIdx.x == 0 && threadIdx.x == 0;
  if (k_end < nl_block_read(&ctl->cg_stop)) {  // else an earlier iteration has ended the solve
    double rz, bb, rel;
    if (!nl_cg_ended(Pz, nbv, k_end, ctl, tol, cg_max, sh, &rz, &bb, &rel)) return;
    if (writer) nl_cg_record_end(ctl, k_end, rel);
  }
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[2] = {0.0, 0.0};
  if (v < N)
    for (int c = 0; c < 3; ++c) {
      const size_t i = 3 * (size_t)v + c;
      const double d = sc[i] * x[i];
      acc[0] += d * d;
      acc[1] += R[i] * R[i];
    }
  write_partials<RA_BLOCK, 2>(acc, sh, Pv);
  if (writer) ctl->cg_done = 1;
}

// ---------------------------------------------------------------- one thread's decisions (trust_region.h)
__global__ void __launch_bounds__(RA_BLOCK) k_nl_decide(int nbe, const double* __restrict__ Pe, int nbv, const double* __restrict__ Pv,
                                                        NlCtl* ctl, int mode, NlOpt o, double initial_radius) {
  if (mode && (nl_ended(ctl) || !ctl->cg_done || ctl->pending)) return;
  __shared__ double sh[2 * RA_BLOCK];
  double e2[2], v2[2] = {0.0, 0.0};
  sum_partials<RA_BLOCK, 2>(Pe, nbe, e2, sh);
  if (mode) sum_partials<RA_BLOCK, 2>(Pv, nbv, v2, sh);
  if (threadIdx.x != 0) return;
  if (mode == 0) {
    ctl->cost = ctl->initial_cost = e2[0];
    ctl->radius = initial_radius;
    ctl->accepted = 1;
    ctl->pending = 1;
    if (!isfinite(e2[0])) tr_finish(ctl, TR_FAILURE);
    return;
  }
  ctl->cg_done = 0;
  if (!(ctl->last_resid <= o.cg_max_resid)) {
    tr_finish(ctl, NL_LINEAR_SOLVER_FAILED);
    return;
  }
  ctl->pending = 1;
  // e2: the candidate's cost and model_cost_change; v2: |delta|^2 and |x|^2.  An accepted candidate is already linearised.
  if (tr_decide(ctl, o.tr, true, e2[0], e2[1], v2[0], v2[1]) == TR_ACCEPTED) ctl->cur ^= 1;
}

// after every iteration (and at iteration 0): the gradient max-norm when fresh, the checks that end an iteration, the trace row
__global__ void __launch_bounds__(RA_BLOCK) k_nl_post(int nbv, const double* __restrict__ Pg, NlCtl* ctl, NlOpt o, double* __restrict__ trace) {
  if (!ctl->pending) return;
  __shared__ double sh[RA_BLOCK];
  const double gm = max_partials<RA_BLOCK>(Pg, (uint32_t)nbv, sh);
  if (threadIdx.x != 0) return;
  const bool fresh = ctl->accepted && !ctl->done;
  if (fresh) ctl->gnorm = gm;
  tr_end_iteration(ctl, o.tr, fresh);
  if (trace) {
    double* row = trace + (size_t)DSM_NLR_TRACE_COLUMNS * ctl->iter;
    row[0] = ctl->cost;
    row[1] = ctl->radius;
    row[2] = ctl->last_rho;
    row[3] = ctl->iter ? (double)ctl->cg_last : 0.0;
    row[4] = (double)ctl->accepted;
    row[5] = ctl->gnorm;
  }
  ctl->pending = 0;
}

}  // namespace

extern "C" void dsm_default_nonlinear_rotation_options(dsm_nonlinear_rotation_options* o) {
  if (!o) return;
  *o = dsm_nonlinear_rotation_options{};
  o->robust_loss_width = 0.1;
  o->max_num_iterations = 200;
  o->max_num_consecutive_invalid_steps = 5;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_cg_iterations = 0;
  o->cg_tolerance = 1e-14;
  o->cg_max_residual = 1e-9;
  o->max_relative_rotation_difference_degrees = 5.0;
}

extern "C" int dsm_debug_pairwise_rotation_error(dsm_ctx* ctx, uint32_t n, const double* rotation1, const double* rotation2,
                                                 const double* relative_rotation, double loss_width, double* residuals,
                                                 double* jacobians, double* rho) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (n && (!rotation1 || !rotation2 || !relative_rotation || !residuals || !jacobians || !rho))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_debug_pairwise_rotation_error: NULL argument");
  if (!(loss_width > 0.0) || !std::isfinite(loss_width))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_debug_pairwise_rotation_error: loss_width must be positive");
  if (n == 0) return DSM_OK;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf in, out;
  const size_t n3 = 3 * (size_t)n;
  HIPCHK(ctx, in.reserve(3 * n3 * 8));
  HIPCHK(ctx, out.reserve(8 * n3 * 8));
  double* di = in.as<double>();
  double* d_o = out.as<double>();
  HIPCHK(ctx, hipMemcpyAsync(di, rotation1, n3 * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(di + n3, rotation2, n3 * 8, hipMemcpyHostToDevice, st));
  HIPCHK(ctx, hipMemcpyAsync(di + 2 * n3, relative_rotation, n3 * 8, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_nl_debug, dim3((n + RA_BLOCK - 1) / RA_BLOCK), dim3(RA_BLOCK), 0, st, n, (const double*)di, (const double*)(di + n3),
                     (const double*)(di + 2 * n3), loss_width * loss_width, d_o, d_o + 2 * n3, d_o + n3);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipMemcpyAsync(residuals, d_o, n3 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(rho, d_o + n3, n3 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(jacobians, d_o + 2 * n3, 6 * n3 * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  return DSM_OK;
}

extern "C" int dsm_view_graph_rotation_averaging_nonlinear(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs,
                                                           const uint8_t* use, uint32_t n_initial, const uint32_t* initial_image_ids,
                                                           const double* initial_orientations,
                                                           const dsm_nonlinear_rotation_options* options, uint32_t* image_ids_out,
                                                           double* orientations_out, uint8_t* image_in_final_cc, uint32_t* n_images_out,
                                                           uint8_t* edge_state, double* relative_rotations_out,
                                                           dsm_nonlinear_rotation_report* report, double* trace) {
  static const char* const kWho = "dsm_view_graph_rotation_averaging_nonlinear";
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!n_images_out || (n_pairs && (!pairs || !qvecs || !image_ids_out || !orientations_out || !image_in_final_cc || !edge_state ||
                                    !relative_rotations_out)) ||
      (n_initial && (!initial_image_ids || !initial_orientations)))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging_nonlinear: NULL argument");
  if (n_pairs > (UINT32_MAX >> 2)) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging_nonlinear: too many pairs");
  dsm_nonlinear_rotation_options o;
  if (options)
    o = *options;
  else
    dsm_default_nonlinear_rotation_options(&o);
  if (!(o.robust_loss_width > 0.0) || !std::isfinite(o.robust_loss_width) || o.max_num_iterations < 0 ||
      o.max_num_iterations > (1 << 20) || o.max_num_consecutive_invalid_steps < 1 || !(o.function_tolerance >= 0.0) ||
      !(o.gradient_tolerance >= 0.0) || !(o.parameter_tolerance >= 0.0) || !(o.initial_trust_region_radius > 0.0) ||
      !std::isfinite(o.initial_trust_region_radius) || !(o.max_trust_region_radius >= o.initial_trust_region_radius) ||
      !(o.min_relative_decrease >= 0.0) || !(o.min_lm_diagonal > 0.0) || !(o.max_lm_diagonal >= o.min_lm_diagonal) ||
      o.max_num_cg_iterations < 0 || !(o.cg_tolerance > 0.0) || !(o.cg_max_residual > 0.0) ||
      !(o.max_relative_rotation_difference_degrees >= 0.0))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging_nonlinear: option out of range");
  for (uint32_t k = 0; k < n_initial; ++k) {
    if (k && initial_image_ids[k] <= initial_image_ids[k - 1])
      return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging_nonlinear: initial_image_ids must ascend strictly");
    for (int c = 0; c < 3; ++c)
      if (!std::isfinite(initial_orientations[3 * (size_t)k + c]))
        return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging_nonlinear: non-finite initial orientation");
  }
  dsm_nonlinear_rotation_report rep{};
  rep.termination = DSM_BA_NO_CONVERGENCE;
  *n_images_out = 0;
  if (report) *report = rep;
  // step 1 (rotation_graph.h)
  RaGraph g;
  if (const int grc = ra_build_graph(ctx, kWho, n_pairs, pairs, qvecs, use, edge_state, relative_rotations_out, g)) return grc;
  if (g.M == 0) return DSM_OK;
  const uint32_t N = g.N, M = g.M;
  rep.num_components = g.num_components;
  rep.num_images = N;
  rep.num_edges = M;
  const size_t n3 = 3 * (size_t)N, m3 = 3 * (size_t)M;
  std::vector<double> Rh(n3, 0.0), relh(m3);
  if (n_initial) {
    for (uint32_t v = 0; v < N; ++v) {
      const uint32_t* it = std::lower_bound(initial_image_ids, initial_image_ids + n_initial, g.cimg[v]);
      if (it == initial_image_ids + n_initial || *it != g.cimg[v]) {
        for (uint32_t e = 0; e < n_pairs; ++e) edge_state[e] = 0;
        return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT,
                        "dsm_view_graph_rotation_averaging_nonlinear: an image of the first component has no initial orientation");
      }
      for (int c = 0; c < 3; ++c) Rh[3 * (size_t)v + c] = initial_orientations[3 * (size_t)(it - initial_image_ids) + c];
    }
  }

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  const int nbv = (int)((N + RA_BLOCK - 1) / RA_BLOCK), nbe = (int)((M + RA_BLOCK - 1) / RA_BLOCK);
  DevBuf d_ei, d_ej, d_off, d_nb, d_ce, d_r12, d_R, d_x, d_r, d_z, d_p0, d_p1, d_q, d_sc, d_D, d_gs, d_lm, d_B, d_Minv, d_E0, d_E1, d_Pe,
      d_Pv, d_Pg, d_Pq, d_Pz0, d_Pz1, d_ctl, d_state, d_rel, d_trace;
  DevEvent ev0, ev1;
  int rc = DSM_OK;
  const size_t trace_n = ((size_t)o.max_num_iterations + 1) * DSM_NLR_TRACE_COLUMNS;
  HIPTRY(d_ei.reserve((size_t)M * 4));
  HIPTRY(d_ej.reserve((size_t)M * 4));
  HIPTRY(d_off.reserve(((size_t)N + 1) * 4));
  HIPTRY(d_nb.reserve((size_t)M * 8));
  HIPTRY(d_ce.reserve((size_t)M * 8));
  HIPTRY(d_r12.reserve(m3 * 8));
  for (DevBuf* b : {&d_R, &d_x, &d_r, &d_z, &d_p0, &d_p1, &d_q, &d_sc, &d_D, &d_gs, &d_lm}) HIPTRY(b->reserve(n3 * 8));
  for (DevBuf* b : {&d_B, &d_Minv}) HIPTRY(b->reserve(6 * (size_t)N * 8));
  for (DevBuf* b : {&d_E0, &d_E1}) HIPTRY(b->reserve((size_t)NL_EDGE * M * 8));
  HIPTRY(d_Pe.reserve((size_t)nbe * 2 * 8));
  for (DevBuf* b : {&d_Pv, &d_Pg, &d_Pq, &d_Pz0, &d_Pz1}) HIPTRY(b->reserve((size_t)nbv * 2 * 8));
  HIPTRY(d_ctl.reserve(sizeof(NlCtl)));
  HIPTRY(d_state.reserve(M));
  HIPTRY(d_rel.reserve(m3 * 8));
  HIPTRY(d_trace.reserve(trace_n * 8));
  HIPTRY(hipEventCreate(&ev0.e));
  HIPTRY(hipEventCreate(&ev1.e));
  NlCtl h{};
  tr_init(&h, 0.0);  // k_nl_decide(mode 0) sets the radius
  if (rc == DSM_OK) {
    HIPTRY(hipEventRecord(ev0, st));
    HIPTRY(hipMemcpyAsync(d_ei.p, g.ei.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ej.p, g.ej.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_off.p, g.off.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_nb.p, g.nb.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ce.p, g.cev.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_r12.p, g.r12.data(), m3 * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_R.p, Rh.data(), n3 * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ctl.p, &h, sizeof(NlCtl), hipMemcpyHostToDevice, st));
    for (DevBuf* b : {&d_x, &d_p0, &d_p1, &d_sc}) HIPTRY(hipMemsetAsync(b->p, 0, n3 * 8, st));
    HIPTRY(hipMemsetAsync(d_Pg.p, 0, (size_t)nbv * 8, st));
    HIPTRY(hipMemsetAsync(d_trace.p, 0, trace_n * 8, st));
  }
  NlCtl* ctl = d_ctl.as<NlCtl>();
  const uint32_t *ei_ = d_ei.as<uint32_t>(), *ej_ = d_ej.as<uint32_t>(), *off_ = d_off.as<uint32_t>(), *nb_ = d_nb.as<uint32_t>(),
                 *ce_ = d_ce.as<uint32_t>();
  double *R_ = d_R.as<double>(), *x_ = d_x.as<double>(), *r_ = d_r.as<double>(), *z_ = d_z.as<double>(), *q_ = d_q.as<double>(),
         *sc_ = d_sc.as<double>(), *D_ = d_D.as<double>(), *gs_ = d_gs.as<double>(), *lm_ = d_lm.as<double>(), *B_ = d_B.as<double>(),
         *Mi_ = d_Minv.as<double>(), *E0_ = d_E0.as<double>(), *E1_ = d_E1.as<double>(), *Pe_ = d_Pe.as<double>(), *Pv_ = d_Pv.as<double>(),
         *Pg_ = d_Pg.as<double>(), *Pq_ = d_Pq.as<double>(), *tr_ = d_trace.as<double>();
  double* p_[2] = {d_p0.as<double>(), d_p1.as<double>()};
  double* Pz_[2] = {d_Pz0.as<double>(), d_Pz1.as<double>()};
  NlOpt k{};
  k.loss_b = o.robust_loss_width * o.robust_loss_width;
  k.tr.ftol = o.function_tolerance;
  k.tr.gtol = o.gradient_tolerance;
  k.tr.ptol = o.parameter_tolerance;
  k.tr.max_radius = o.max_trust_region_radius;
  k.tr.min_radius = kTrMinRadius;
  k.tr.min_relative_decrease = o.min_relative_decrease;
  k.min_diag = o.min_lm_diagonal;
  k.max_diag = o.max_lm_diagonal;
  k.cg_tol = o.cg_tolerance;
  k.cg_max_resid = o.cg_max_residual;
  k.tr.max_iterations = o.max_num_iterations;
  k.tr.max_consecutive_invalid_steps = o.max_num_consecutive_invalid_steps;
  k.cg_max = o.max_num_cg_iterations > 0 ? o.max_num_cg_iterations : (int)std::max<uint32_t>(1000u, 20u * N);
  const dim3 gv(nbv), ge(nbe), one(1), bs(RA_BLOCK);
  auto read_ctl = [&]() {
    HIPTRY(hipGetLastError());
    HIPTRY(hipMemcpyAsync(&h, d_ctl.p, sizeof(NlCtl), hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
  };
  // the tail of an LM iteration (mode 1) or the start (mode 0): candidate, decision, commit + linearisation, termination tests
  auto tail = [&](int mode) {
    hipLaunchKernelGGL(k_nl_edges, ge, bs, 0, st, M, ei_, ej_, (const double*)d_r12.as<double>(), (const double*)R_, (const double*)x_,
                       (const double*)sc_, k.loss_b, (const NlCtl*)ctl, mode, E0_, E1_, Pe_);
    hipLaunchKernelGGL(k_nl_decide, one, bs, 0, st, nbe, (const double*)Pe_, nbv, (const double*)Pv_, ctl, mode, k,
                       o.initial_trust_region_radius);
    hipLaunchKernelGGL(k_nl_linearize, gv, bs, 0, st, N, off_, ce_, (const double*)E0_, (const double*)E1_, (const double*)x_, R_, sc_, D_,
                       gs_, B_, (const NlCtl*)ctl, mode, k, Pg_);
    hipLaunchKernelGGL(k_nl_post, one, bs, 0, st, nbv, (const double*)Pg_, ctl, k, tr_);
  };
  if (rc == DSM_OK) {
    tail(0);
    read_ctl();
  }
  int budget = std::min(k.cg_max, 48);
  uint64_t launches = 4;
  while (rc == DSM_OK && !h.done) {
    hipLaunchKernelGGL(k_nl_cg_init, gv, bs, 0, st, N, (const double*)D_, (const double*)gs_, (const double*)B_, lm_, Mi_, x_, r_, z_, ctl,
                       Pz_[0]);
    ++launches;
    for (int k0 = 0; rc == DSM_OK;) {
      const int k1 = std::min(k.cg_max, k0 + budget);
      for (int it = k0; it < k1; ++it) {
        hipLaunchKernelGGL(k_nl_cg_ap, gv, bs, 0, st, N, nbv, off_, nb_, ce_, (const double*)E0_, (const double*)E1_, (const double*)sc_,
                           (const double*)lm_, (const double*)z_, (const double*)p_[it & 1], p_[(it + 1) & 1], q_, ctl, it, k.cg_tol,
                           k.cg_max, (const double*)Pz_[it & 1], Pq_);
        hipLaunchKernelGGL(k_nl_cg_xr, gv, bs, 0, st, N, nbv, (const double*)Pq_, (const double*)Mi_, (const double*)p_[(it + 1) & 1],
                           (const double*)q_, x_, r_, z_, (const NlCtl*)ctl, it, Pz_[(it + 1) & 1]);
      }
      hipLaunchKernelGGL(k_nl_step, gv, bs, 0, st, N, nbv, (const double*)R_, (const double*)x_, (const double*)sc_, ctl, k1, k.cg_tol, k.cg_max,
                         (const double*)Pz_[k1 & 1], Pv_);
      tail(1);
      launches += 2 * (uint64_t)(k1 - k0) + 5;
      read_ctl();
      if (h.done || h.cg_stop != INT_MAX || k1 >= k.cg_max) break;  // the solve ended inside the budget: the tail has run
      k0 = k1;
    }
    budget = std::min(k.cg_max, std::max(16, h.cg_last + h.cg_last / 4 + 8));
  }
  if (rc == DSM_OK && h.term == NL_LINEAR_SOLVER_FAILED) {
    ctx->err = std::string(kWho) + ": a conjugate-gradient solve ended at a relative residual of " + std::to_string(h.last_resid);
    rc = DSM_ERR_NOT_CONVERGED;
  }
  std::vector<uint8_t> st8(M);
  if (rc == DSM_OK) {
    // step 3 (rotation_graph.h)
    const double thr = o.max_relative_rotation_difference_degrees * kRaDegToRad;
    hipLaunchKernelGGL(k_ra_filter, ge, bs, 0, st, M, ei_, ej_, (const double*)d_r12.as<double>(), (const double*)R_, thr * thr,
                       d_state.as<uint8_t>(), d_rel.as<double>());
    HIPTRY(hipGetLastError());
    HIPTRY(hipEventRecord(ev1, st));
    HIPTRY(hipMemcpyAsync(Rh.data(), d_R.p, n3 * 8, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(st8.data(), d_state.p, M, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(relh.data(), d_rel.p, m3 * 8, hipMemcpyDeviceToHost, st));
    if (trace && h.iter >= 0)
      HIPTRY(hipMemcpyAsync(trace, d_trace.p, ((size_t)h.iter + 1) * DSM_NLR_TRACE_COLUMNS * 8, hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    HIPTRY(dev_events_ms(ev0, ev1, &rep.device_ms));
  }
  if (rc != DSM_OK) (void)hipStreamSynchronize(st);
  rep.termination = h.term == NL_LINEAR_SOLVER_FAILED || !h.done ? DSM_BA_FAILURE : h.term;
  rep.num_iterations = (uint32_t)h.iter;
  rep.num_successful_steps = (uint32_t)h.n_succ;
  rep.num_rejected_steps = (uint32_t)h.n_rej;
  rep.num_invalid_steps = (uint32_t)h.n_invalid_total;
  rep.total_cg_iterations = h.cg_total;
  rep.num_kernel_launches = launches;
  rep.initial_cost = h.initial_cost;
  rep.final_cost = h.cost;
  rep.final_trust_region_radius = h.radius;
  rep.max_cg_relative_residual = h.cg_worst;
  rep.min_rho_margin = h.m_accept;
  rep.min_gradient_margin = h.m_grad;
  rep.min_function_margin = h.m_func;
  if (rc == DSM_OK) {
    ra_write_outputs(g, st8, relh, Rh, image_ids_out, orientations_out, image_in_final_cc, n_images_out, edge_state, relative_rotations_out,
                     &rep.num_filtered_edges, &rep.num_final_images);
  } else {
    for (uint32_t e = 0; e < n_pairs; ++e) edge_state[e] = 0;
  }
  if (report) *report = rep;
  return rc;
}
