// rotation_averaging.hip -- global rotation averaging of the filtered view graph ("Global rotation averaging").
//   DistributedMapperController::GlobalRotationAveraging  src/controllers/distributed_mapper_controller.cpp:945-1008
//   RobustRotationEstimator (ROBUST_L1L2)                  src/rotation_estimation/robust_rotation_estimator.cpp:84-318
//   L1Solver (ADMM)                                        src/solver/l1_solver.h
//   FilterViewPairsFromOrientation                         src/sfm/filter_view_pairs_from_orientation.cpp:22-90
//   ImageGraph::ExtractLargestCC                           src/graph/image_graph.cpp:8-50
// Every edge's three weights are equal, so A^T W A = L_w (x) I3 with L_w the weighted graph Laplacian grounded at the
// constant image: every solve of the reference (CHOLMOD) is here ONE scalar SPD system with three right-hand sides, solved by a
// Jacobi-preconditioned conjugate gradient warm-started from the previous solve.  Vectors over images are [N][3] (image 0,
// the smallest id, is the constant one and stays 0); vectors over edges are [M][3].  The host builds the component and a CSR
// over images whose entries are sorted by neighbour; every operator that sums over edges is a gather over that CSR row (no
// floating-point atomics), every reduction is per-block partials (a fixed LDS tree) summed by one fixed tree, so the result
// is the same bytes from run to run and for every order of the input list.  Loop control stays on the device: a kernel of CG
// iteration k (ADMM iteration t) is a no-op once k >= ctl.cg_stop (t >= ctl.admm_stop); the host enqueues iterations in
// batches, reads the flags between batches, and the batch size changes only the number of no-op launches.
#include <hip/hip_runtime.h>
#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "block_reduce.h"
#include "ctx.h"
#include "graph_edges.h"
#include "rotation_ceres.h"
#include "rotation_graph.h"

namespace {

// device-side loop state; every field has one writer per launch and no reader in that launch
struct RaCtl {
  int cg_stop;          // CG iterations k >= cg_stop are no-ops (INT_MAX while the solve runs)
  int admm_stop;        // ADMM iterations t >= admm_stop are no-ops
  int step_stop;        // 1: the L1 / IRLS loop has converged (written by k_ra_step_check)
  int admm_iters;       // ADMM iterations of the current Solve
  double rz[2][3];      // r.z of the running CG solve, double-buffered by iteration parity
  int active[2][3];     // column still iterating, double-buffered by iteration parity
  double bb[3];         // ||b_c||^2 of the running solve
  int cold[3];          // the warm start was worse than zero: the column restarts from x = 0
  unsigned long long cg_total;
  double cg_worst;      // largest final relative residual of all solves
  double last_resid;    // final relative residual of the last solve
  double last_step;     // average step of the last L1 / IRLS iteration
  double admm_r, admm_s, admm_pe, admm_de;  // the last ADMM stopping values
};

__device__ inline bool gated(const RaCtl* c, int admm_t) { return admm_t >= 0 && admm_t >= c->admm_stop; }

// ---------------------------------------------------------------- per-edge kernels
// residuals (robust_rotation_estimator.cpp:290-307): b_e = MultiplyRotations(-R_j, MultiplyRotations(R12_e, R_i)), and the
// IRLS weight w_e = sigma / (|b_e|^2 + sigma^2)^2 (:235-241); partials of ||b||^2
__global__ void __launch_bounds__(RA_BLOCK) k_ra_residuals(uint32_t M, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej,
                                                           const double* __restrict__ r12, const double* __restrict__ R, double sigma,
                                                           double* __restrict__ b, double* __restrict__ w, double* __restrict__ P) {
  __shared__ double sh[RA_BLOCK];
  const uint32_t e = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[1] = {0.0};
  if (e < M) {
    const double* Ri = R + 3 * (size_t)ei[e];
    const double* Rj = R + 3 * (size_t)ej[e];
    double inner[3], mRj[3] = {-Rj[0], -Rj[1], -Rj[2]}, res[3];
    mul_rot(r12 + 3 * (size_t)e, Ri, inner);
    mul_rot(mRj, inner, res);
    const double e2 = res[0] * res[0] + res[1] * res[1] + res[2] * res[2];
    const double tmp = e2 + sigma * sigma;
    w[e] = sigma / (tmp * tmp);
    for (int c = 0; c < 3; ++c) b[3 * (size_t)e + c] = res[c];
    acc[0] = res[0] * res[0] + res[1] * res[1] + res[2] * res[2];
  }
  write_partials<RA_BLOCK, 1>(acc, sh, P);
}

// ADMM after the x update (l1_solver.h Solve): Ax, ax_hat, z (shrinkage), u; partials of ||Ax - z - b||^2, ||Ax||^2, ||z||^2
__global__ void __launch_bounds__(RA_BLOCK) k_ra_admm_edges(uint32_t M, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej,
                                                            const double* __restrict__ x, const double* __restrict__ b,
                                                            double* __restrict__ z, double* __restrict__ zold, double* __restrict__ u,
                                                            double alpha, double rho, RaCtl* ctl, int t, double* __restrict__ P) {
  if (gated(ctl, t)) return;
  __shared__ double sh[3 * RA_BLOCK];
  const uint32_t e = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[3] = {0.0, 0.0, 0.0};
  if (e < M) {
    const double kappa = 1.0 / rho;
    const double* xi = x + 3 * (size_t)ei[e];
    const double* xj = x + 3 * (size_t)ej[e];
    for (int c = 0; c < 3; ++c) {
      const size_t k = 3 * (size_t)e + c;
      const double ax = xj[c] - xi[c];
      const double zo = z[k], bk = b[k];
      double ah = alpha * ax;
      ah += (1.0 - alpha) * (zo + bk);
      const double v = ah - bk + u[k];
      const double zn = fmax(0.0, v - kappa) - fmax(0.0, -v - kappa);
      u[k] += ah - zn - bk;
      zold[k] = zo;
      z[k] = zn;
      const double r = ax - zn - bk;
      acc[0] += r * r;
      acc[1] += ax * ax;
      acc[2] += zn * zn;
    }
  }
  write_partials<RA_BLOCK, 3>(acc, sh, P);
}

// ---------------------------------------------------------------- per-image kernels (gathers over the CSR row)
// CSR: image v has entries p in [off[v], off[v + 1]) sorted by neighbour nb[p]; ce[p] = 2 * edge + (v is the edge's image 2),
// i.e. the sign of A's block: -I for image 1, +I for image 2.

// right-hand side: mode 0 (ADMM, l1_solver.h) rhs = A^T (b + z - u);  mode 1 (IRLS) rhs = A^T W b
__global__ void __launch_bounds__(RA_BLOCK) k_ra_rhs(uint32_t N, const uint32_t* __restrict__ off, const uint32_t* __restrict__ ce,
                                                     int mode, const double* __restrict__ b, const double* __restrict__ z,
                                                     const double* __restrict__ u, const double* __restrict__ w, double* __restrict__ rhs,
                                                     const RaCtl* ctl, int t) {
  if (gated(ctl, t)) return;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  if (v >= N) return;
  double s[3] = {0.0, 0.0, 0.0};
  if (v > 0) {
    for (uint32_t p = off[v]; p < off[v + 1]; ++p) {
      const uint32_t e = ce[p] >> 1;
      const double sg = (ce[p] & 1) ? 1.0 : -1.0;
      for (int c = 0; c < 3; ++c) {
        const size_t k = 3 * (size_t)e + c;
        const double val = mode == 0 ? (b[k] + z[k]) - u[k] : w[e] * b[k];
        s[c] += sg * val;
      }
    }
  }
  for (int c = 0; c < 3; ++c) rhs[3 * (size_t)v + c] = s[c];
}

// (L_w y)_v = d_v y_v - sum_u w_e y_u over the row (image 0 is grounded: y_0 = 0 and row 0 is 0)
__device__ inline void lap_row(uint32_t v, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nb,
                               const uint32_t* __restrict__ ce, const double* __restrict__ w, const double* __restrict__ y, double d,
                               double* out) {
  double s[3] = {0.0, 0.0, 0.0};
  for (uint32_t p = off[v]; p < off[v + 1]; ++p) {
    const double we = w[ce[p] >> 1];
    const double* yu = y + 3 * (size_t)nb[p];
    for (int c = 0; c < 3; ++c) s[c] += we * yu[c];
  }
  for (int c = 0; c < 3; ++c) out[c] = d * y[3 * (size_t)v + c] - s[c];
}

// CG start, part 1: weighted degrees d, r = rhs - L x (warm start); partials of ||r_c||^2, ||rhs_c||^2
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_init(uint32_t N, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nb,
                                                         const uint32_t* __restrict__ ce, const double* __restrict__ w,
                                                         const double* __restrict__ rhs, const double* __restrict__ x,
                                                         double* __restrict__ d, double* __restrict__ r, const RaCtl* ctl, int t,
                                                         double* __restrict__ P) {
  if (gated(ctl, t)) return;
  __shared__ double sh[6 * RA_BLOCK];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  if (v < N && v > 0) {
    double dv = 0.0;
    for (uint32_t p = off[v]; p < off[v + 1]; ++p) dv += w[ce[p] >> 1];
    d[v] = dv;
    double lx[3];
    lap_row(v, off, nb, ce, w, x, dv, lx);
    for (int c = 0; c < 3; ++c) {
      const double bc = rhs[3 * (size_t)v + c];
      const double rc = bc - lx[c];
      r[3 * (size_t)v + c] = rc;
      acc[c] = rc * rc;
      acc[3 + c] = bc * bc;
    }
  } else if (v == 0) {
    d[0] = 1.0;
    for (int c = 0; c < 3; ++c) r[c] = 0.0;
  }
  write_partials<RA_BLOCK, 6>(acc, sh, P);
}

// CG start, part 2 (one block): a column whose warm start is worse than zero (||r|| > ||b||) restarts cold
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_init_fin(int nb, const double* __restrict__ P, RaCtl* ctl, int t) {
  if (gated(ctl, t)) return;
  __shared__ double sh[6 * RA_BLOCK];
  double s[6];
  sum_partials<RA_BLOCK, 6>(P, nb, s, sh);
  if (threadIdx.x == 0)
    for (int c = 0; c < 3; ++c) {
      ctl->bb[c] = s[3 + c];
      ctl->cold[c] = s[c] > s[3 + c];
    }
}

// CG start, part 3: z = r / d, p = z (cold columns: x = 0, r = rhs); partials of r.z, r.r
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_init2(uint32_t N, const double* __restrict__ rhs, const double* __restrict__ d,
                                                          double* __restrict__ x, double* __restrict__ r, double* __restrict__ zp,
                                                          double* __restrict__ p, const RaCtl* ctl, int t, double* __restrict__ P) {
  if (gated(ctl, t)) return;
  __shared__ double sh[6 * RA_BLOCK];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  if (v < N) {
    for (int c = 0; c < 3; ++c) {
      const size_t k = 3 * (size_t)v + c;
      if (ctl->cold[c]) {
        x[k] = 0.0;
        r[k] = v > 0 ? rhs[k] : 0.0;
      }
      const double zz = v > 0 ? r[k] / d[v] : 0.0;
      zp[k] = zz;
      p[k] = zz;
      acc[c] = r[k] * zz;
      acc[3 + c] = r[k] * r[k];
    }
  }
  write_partials<RA_BLOCK, 6>(acc, sh, P);
}

// the state of the solve after r.z / r.r are known (one writer: thread 0 of the calling block)
__device__ inline void cg_decide(RaCtl* ctl, const double (&s)[6], int slot, int k_done, int cg_max, double tol) {
  double worst = 0.0;
  int any = 0;
  for (int c = 0; c < 3; ++c) {
    ctl->rz[slot][c] = s[c];
    const double rel = ctl->bb[c] > 0.0 ? sqrt(s[3 + c] / ctl->bb[c]) : 0.0;
    const int act = ctl->bb[c] > 0.0 && rel > tol;
    ctl->active[slot][c] = act;
    any |= act;
    worst = fmax(worst, rel);
  }
  if (!any || k_done >= cg_max) {
    ctl->cg_stop = k_done;
    ctl->cg_total += (unsigned long long)k_done;
    ctl->last_resid = worst;
    ctl->cg_worst = fmax(ctl->cg_worst, worst);
  } else {
    ctl->cg_stop = INT_MAX;
  }
}

// CG start, part 4 (one block): rz, active columns, stop at 0 iterations when nothing is left to do
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_init_fin2(int nb, const double* __restrict__ P, RaCtl* ctl, int t, int cg_max,
                                                              double tol) {
  if (gated(ctl, t)) return;
  __shared__ double sh[6 * RA_BLOCK];
  double s[6];
  sum_partials<RA_BLOCK, 6>(P, nb, s, sh);
  if (threadIdx.x == 0) cg_decide(ctl, s, 0, 0, cg_max, tol);
}

// CG iteration k, part 1: q = L p; partials of p.q
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_lp(uint32_t N, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nb,
                                                       const uint32_t* __restrict__ ce, const double* __restrict__ w,
                                                       const double* __restrict__ d, const double* __restrict__ p, double* __restrict__ q,
                                                       const RaCtl* ctl, int t, int k, double* __restrict__ P) {
  if (gated(ctl, t) || k >= ctl->cg_stop) return;
  __shared__ double sh[3 * RA_BLOCK];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[3] = {0, 0, 0};
  if (v < N) {
    double lq[3] = {0.0, 0.0, 0.0};
    if (v > 0) lap_row(v, off, nb, ce, w, p, d[v], lq);
    for (int c = 0; c < 3; ++c) {
      q[3 * (size_t)v + c] = lq[c];
      acc[c] = p[3 * (size_t)v + c] * lq[c];
    }
  }
  write_partials<RA_BLOCK, 3>(acc, sh, P);
}

// CG iteration k, part 2: alpha = rz / pq (every block sums the same partials); x += alpha p, r -= alpha q, z = r / d;
// partials of r.z, r.r
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_update(uint32_t N, int nb, const double* __restrict__ Ppq, const double* __restrict__ d,
                                                           double* __restrict__ x, double* __restrict__ r, double* __restrict__ zp,
                                                           const double* __restrict__ p, const double* __restrict__ q, const RaCtl* ctl,
                                                           int t, int k, double* __restrict__ P) {
  if (gated(ctl, t) || k >= ctl->cg_stop) return;
  __shared__ double sh[6 * RA_BLOCK];
  double pq[3];
  sum_partials<RA_BLOCK, 3>(Ppq, nb, pq, sh);
  double alpha[3];
  for (int c = 0; c < 3; ++c) alpha[c] = ctl->active[k & 1][c] ? ctl->rz[k & 1][c] / pq[c] : 0.0;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[6] = {0, 0, 0, 0, 0, 0};
  if (v < N && v > 0) {
    for (int c = 0; c < 3; ++c) {
      const size_t i = 3 * (size_t)v + c;
      x[i] += alpha[c] * p[i];
      const double rc = r[i] - alpha[c] * q[i];
      r[i] = rc;
      const double zz = rc / d[v];
      zp[i] = zz;
      acc[c] = rc * zz;
      acc[3 + c] = rc * rc;
    }
  }
  write_partials<RA_BLOCK, 6>(acc, sh, P);
}

// CG iteration k, part 3: beta = rz_new / rz (every block sums the same partials), p = z + beta p; thread 0 of block 0 writes
// the state of iteration k + 1 into the other parity slot
__global__ void __launch_bounds__(RA_BLOCK) k_ra_cg_dir(uint32_t N, int nb, const double* __restrict__ Prz, const double* __restrict__ zp,
                                                        double* __restrict__ p, RaCtl* ctl, int t, int k, int cg_max, double tol) {
  if (gated(ctl, t) || k >= ctl->cg_stop) return;
  __shared__ double sh[6 * RA_BLOCK];
  double s[6];
  sum_partials<RA_BLOCK, 6>(Prz, nb, s, sh);
  double beta[3];
  for (int c = 0; c < 3; ++c) beta[c] = ctl->active[k & 1][c] ? s[c] / ctl->rz[k & 1][c] : 0.0;
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  if (v < N)
    for (int c = 0; c < 3; ++c) {
      const size_t i = 3 * (size_t)v + c;
      if (ctl->active[k & 1][c]) p[i] = zp[i] + beta[c] * p[i];
    }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    // a column that stopped is no longer updated: its r.z and r.r are still those it stopped at, and it stays stopped
    cg_decide(ctl, s, (k + 1) & 1, k + 1, cg_max, tol);
  }
}

// ADMM convergence terms over images: ||rho A^T (z - z_old)||^2, ||rho A^T u||^2
__global__ void __launch_bounds__(RA_BLOCK) k_ra_admm_verts(uint32_t N, const uint32_t* __restrict__ off, const uint32_t* __restrict__ ce,
                                                            const double* __restrict__ z, const double* __restrict__ zold,
                                                            const double* __restrict__ u, double rho, const RaCtl* ctl, int t,
                                                            double* __restrict__ P) {
  if (gated(ctl, t)) return;
  __shared__ double sh[2 * RA_BLOCK];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[2] = {0, 0};
  if (v < N && v > 0) {
    double sv[3] = {0, 0, 0}, av[3] = {0, 0, 0};
    for (uint32_t p = off[v]; p < off[v + 1]; ++p) {
      const uint32_t e = ce[p] >> 1;
      const double sg = (ce[p] & 1) ? 1.0 : -1.0;
      for (int c = 0; c < 3; ++c) {
        const size_t k = 3 * (size_t)e + c;
        sv[c] += sg * (z[k] - zold[k]);
        av[c] += sg * u[k];
      }
    }
    for (int c = 0; c < 3; ++c) {
      const double a = -rho * sv[c], bq = rho * av[c];
      acc[0] += a * a;
      acc[1] += bq * bq;
    }
  }
  write_partials<RA_BLOCK, 2>(acc, sh, P);
}

// ADMM stop (one block): r_norm < primal_eps && s_norm < dual_eps (l1_solver.h)
__global__ void __launch_bounds__(RA_BLOCK) k_ra_admm_check(int nbe, const double* __restrict__ Pe, const double* __restrict__ Pb, int nbv,
                                                            const double* __restrict__ Pv, double primal_abs, double dual_abs, double rel_tol,
                                                            RaCtl* ctl, int t) {
  if (gated(ctl, t)) return;
  __shared__ double sh[3 * RA_BLOCK];
  double e3[3], b1[1], v2[2];
  sum_partials<RA_BLOCK, 3>(Pe, nbe, e3, sh);
  sum_partials<RA_BLOCK, 1>(Pb, nbe, b1, sh);
  sum_partials<RA_BLOCK, 2>(Pv, nbv, v2, sh);
  if (threadIdx.x == 0) {
    const double r_norm = sqrt(e3[0]), s_norm = sqrt(v2[0]);
    const double max_norm = fmax(fmax(sqrt(e3[1]), sqrt(e3[2])), sqrt(b1[0]));
    const double pe = primal_abs + rel_tol * max_norm;
    const double de = dual_abs + rel_tol * sqrt(v2[1]);
    ctl->admm_iters = t + 1;
    ctl->admm_r = r_norm;
    ctl->admm_s = s_norm;
    ctl->admm_pe = pe;
    ctl->admm_de = de;
    if (r_norm < pe && s_norm < de) ctl->admm_stop = t + 1;
  }
}

// UpdateGlobalRotations (:270-285): R_v = MultiplyRotations(R_v, x_v) for v > 0; partials of |x_v| (ComputeAverageStepSize)
__global__ void __launch_bounds__(RA_BLOCK) k_ra_rotate(uint32_t N, const double* __restrict__ x, double* __restrict__ R,
                                                        double* __restrict__ P) {
  __shared__ double sh[RA_BLOCK];
  const uint32_t v = blockIdx.x * RA_BLOCK + threadIdx.x;
  double acc[1] = {0.0};
  if (v < N && v > 0) {
    const double* xv = x + 3 * (size_t)v;
    double out[3];
    mul_rot(R + 3 * (size_t)v, xv, out);
    for (int c = 0; c < 3; ++c) R[3 * (size_t)v + c] = out[c];
    acc[0] = sqrt(xv[0] * xv[0] + xv[1] * xv[1] + xv[2] * xv[2]);
  }
  write_partials<RA_BLOCK, 1>(acc, sh, P);
}

// average step over N - 1 images; L1 stops on <= threshold, IRLS on < threshold (:207, :258)
__global__ void __launch_bounds__(RA_BLOCK) k_ra_step_check(int nbv, const double* __restrict__ P, uint32_t n_var, double thr, int irls,
                                                            RaCtl* ctl) {
  __shared__ double sh[RA_BLOCK];
  double s[1];
  sum_partials<RA_BLOCK, 1>(P, nbv, s, sh);
  if (threadIdx.x == 0) {
    const double avg = s[0] / (double)n_var;
    ctl->last_step = avg;
    ctl->step_stop = irls ? (avg < thr) : (avg <= thr);
  }
}

__global__ void k_ra_fill(double* __restrict__ a, size_t n, double v) {
  const size_t i = (size_t)blockIdx.x * RA_BLOCK + threadIdx.x;
  if (i < n) a[i] = v;
}

}  // namespace

extern "C" void dsm_default_rotation_averaging_options(dsm_rotation_averaging_options* o) {
  if (!o) return;
  *o = dsm_rotation_averaging_options{};
  o->max_num_l1_iterations = 5;
  o->max_num_irls_iterations = 100;
  o->l1_step_convergence_threshold = 0.001;
  o->irls_step_convergence_threshold = 0.001;
  o->irls_loss_parameter_sigma = 5.0 * kRaDegToRad;
  o->admm_initial_max_iterations = 5;
  o->max_num_cg_iterations = 0;
  o->cg_batch_iterations = 0;
  o->admm_rho = 1.0;
  o->admm_alpha = 1.0;
  o->admm_absolute_tolerance = 1e-4;
  o->admm_relative_tolerance = 1e-2;
  o->max_relative_rotation_difference_degrees = 5.0;
  o->cg_tolerance = 1e-12;
  o->cg_max_residual = 1e-9;
}

extern "C" int dsm_view_graph_rotation_averaging(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs,
                                                 const uint8_t* use, const dsm_rotation_averaging_options* options,
                                                 uint32_t* image_ids_out, double* orientations_out, uint8_t* image_in_final_cc,
                                                 uint32_t* n_images_out, uint8_t* edge_state, double* relative_rotations_out,
                                                 dsm_rotation_averaging_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!n_images_out || (n_pairs && (!pairs || !qvecs || !image_ids_out || !orientations_out || !image_in_final_cc || !edge_state ||
                                    !relative_rotations_out)))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging: NULL argument");
  if (n_pairs > (UINT32_MAX >> 2)) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging: too many pairs");
  dsm_rotation_averaging_options o;
  if (options)
    o = *options;
  else
    dsm_default_rotation_averaging_options(&o);
  if (o.max_num_l1_iterations < 0 || o.max_num_l1_iterations > DSM_RA_MAX_L1_ITERATIONS || o.max_num_irls_iterations < 0 ||
      o.admm_initial_max_iterations < 0 || o.admm_initial_max_iterations > (1 << 20) || o.max_num_cg_iterations < 0 ||
      o.cg_batch_iterations < 0 || !(o.admm_rho > 0.0) || !(o.irls_loss_parameter_sigma > 0.0) ||
      !(o.max_relative_rotation_difference_degrees >= 0.0) || !(o.cg_tolerance > 0.0) || !(o.cg_max_residual > 0.0) ||
      !std::isfinite(o.admm_alpha) || !std::isfinite(o.admm_absolute_tolerance) || !std::isfinite(o.admm_relative_tolerance) ||
      !std::isfinite(o.l1_step_convergence_threshold) || !std::isfinite(o.irls_step_convergence_threshold))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_rotation_averaging: option out of range");
  dsm_rotation_averaging_report rep{};
  *n_images_out = 0;
  if (report) *report = rep;
  // step 1 (rotation_graph.h): the checks on every used edge, the unique edges, the first component and its CSR
  RaGraph g;
  if (const int grc = ra_build_graph(ctx, "dsm_view_graph_rotation_averaging", n_pairs, pairs, qvecs, use, edge_state, relative_rotations_out, g))
    return grc;
  if (g.M == 0) return DSM_OK;
  const uint32_t N = g.N, M = g.M;
  const std::vector<uint32_t>&ei = g.ei, &ej = g.ej, &off = g.off, &nb = g.nb, &cev = g.cev;
  const std::vector<double>& r12 = g.r12;
  rep.num_components = g.num_components;
  rep.num_images = N;
  rep.num_edges = M;

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  const int nbv = (int)((N + RA_BLOCK - 1) / RA_BLOCK), nbe = (int)((M + RA_BLOCK - 1) / RA_BLOCK);
  const size_t n3 = 3 * (size_t)N, m3 = 3 * (size_t)M;
  DevBuf d_ei, d_ej, d_off, d_nb, d_ce, d_r12, d_R, d_x, d_rhs, d_r, d_zp, d_p, d_q, d_d, d_b, d_w, d_one, d_z, d_zold, d_u, d_P1, d_P2,
      d_P3, d_P4, d_ctl, d_state, d_rel;
  DevEvent ev0, ev1;
  int rc = DSM_OK;
  const size_t np = (size_t)std::max(nbv, nbe);
  HIPTRY(d_ei.reserve((size_t)M * 4));
  HIPTRY(d_ej.reserve((size_t)M * 4));
  HIPTRY(d_off.reserve(((size_t)N + 1) * 4));
  HIPTRY(d_nb.reserve((size_t)M * 8));
  HIPTRY(d_ce.reserve((size_t)M * 8));
  HIPTRY(d_r12.reserve(m3 * 8));
  for (DevBuf* b : {&d_R, &d_x, &d_rhs, &d_r, &d_zp, &d_p, &d_q}) HIPTRY(b->reserve(n3 * 8));
  HIPTRY(d_d.reserve((size_t)N * 8));
  for (DevBuf* b : {&d_b, &d_z, &d_zold, &d_u, &d_rel}) HIPTRY(b->reserve(m3 * 8));
  HIPTRY(d_w.reserve((size_t)M * 8));
  HIPTRY(d_one.reserve((size_t)M * 8));
  for (DevBuf* b : {&d_P1, &d_P2, &d_P3, &d_P4}) HIPTRY(b->reserve(np * 6 * 8));
  HIPTRY(d_ctl.reserve(sizeof(RaCtl)));
  HIPTRY(d_state.reserve(M));
  HIPTRY(hipEventCreate(&ev0.e));
  HIPTRY(hipEventCreate(&ev1.e));
  RaCtl h{}, init{};
  init.cg_stop = 0;
  init.admm_stop = INT_MAX;
  static const int kAdmmReset[3] = {INT_MAX, 0, 0};  // admm_stop, step_stop, admm_iters at the start of an L1 iteration
  std::vector<uint8_t> st8(M);
  std::vector<double> Rh(n3), relh(m3);
  if (rc == DSM_OK) {
    HIPTRY(hipEventRecord(ev0, st));
    HIPTRY(hipMemcpyAsync(d_ei.p, ei.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ej.p, ej.data(), (size_t)M * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_off.p, off.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_nb.p, nb.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ce.p, cev.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_r12.p, r12.data(), m3 * 8, hipMemcpyHostToDevice, st));
    HIPTRY(hipMemcpyAsync(d_ctl.p, &init, sizeof(RaCtl), hipMemcpyHostToDevice, st));
    for (DevBuf* b : {&d_R, &d_x, &d_rhs, &d_r, &d_zp, &d_p, &d_q}) HIPTRY(hipMemsetAsync(b->p, 0, n3 * 8, st));
    HIPTRY(hipMemsetAsync(d_d.p, 0, (size_t)N * 8, st));
  }
  RaCtl* ctl = d_ctl.as<RaCtl>();
  const uint32_t* off_ = d_off.as<uint32_t>();
  const uint32_t* nb_ = d_nb.as<uint32_t>();
  const uint32_t* ce_ = d_ce.as<uint32_t>();
  const int cg_max = o.max_num_cg_iterations > 0 ? o.max_num_cg_iterations : (int)std::max<uint32_t>(1000u, 20u * N);
  const int batch = o.cg_batch_iterations > 0 ? o.cg_batch_iterations : 16;
  const double sigma = o.irls_loss_parameter_sigma;
  auto read_ctl = [&]() {
    HIPTRY(hipMemcpyAsync(&h, d_ctl.p, sizeof(RaCtl), hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
  };
  auto residuals = [&]() {
    hipLaunchKernelGGL(k_ra_residuals, dim3(nbe), dim3(RA_BLOCK), 0, st, M, d_ei.as<uint32_t>(), d_ej.as<uint32_t>(), d_r12.as<double>(),
                       d_R.as<double>(), sigma, d_b.as<double>(), d_w.as<double>(), d_P4.as<double>());
  };
  // one CG solve of L_w x = rhs (weights w), gated by ADMM iteration t (-1: not gated); returns false on a read failure
  auto solve = [&](const double* w, int t) {
    hipLaunchKernelGGL(k_ra_cg_init, dim3(nbv), dim3(RA_BLOCK), 0, st, N, off_, nb_, ce_, w, d_rhs.as<double>(), d_x.as<double>(),
                       d_d.as<double>(), d_r.as<double>(), (const RaCtl*)ctl, t, d_P1.as<double>());
    hipLaunchKernelGGL(k_ra_cg_init_fin, dim3(1), dim3(RA_BLOCK), 0, st, nbv, (const double*)d_P1.as<double>(), ctl, t);
    hipLaunchKernelGGL(k_ra_cg_init2, dim3(nbv), dim3(RA_BLOCK), 0, st, N, (const double*)d_rhs.as<double>(), (const double*)d_d.as<double>(),
                       d_x.as<double>(), d_r.as<double>(), d_zp.as<double>(), d_p.as<double>(), (const RaCtl*)ctl, t, d_P2.as<double>());
    hipLaunchKernelGGL(k_ra_cg_init_fin2, dim3(1), dim3(RA_BLOCK), 0, st, nbv, (const double*)d_P2.as<double>(), ctl, t, cg_max,
                       o.cg_tolerance);
    for (int k0 = 0; rc == DSM_OK; k0 += batch) {
      for (int k = k0; k < k0 + batch && k < cg_max; ++k) {
        hipLaunchKernelGGL(k_ra_cg_lp, dim3(nbv), dim3(RA_BLOCK), 0, st, N, off_, nb_, ce_, w, (const double*)d_d.as<double>(),
                           (const double*)d_p.as<double>(), d_q.as<double>(), (const RaCtl*)ctl, t, k, d_P1.as<double>());
        hipLaunchKernelGGL(k_ra_cg_update, dim3(nbv), dim3(RA_BLOCK), 0, st, N, nbv, (const double*)d_P1.as<double>(),
                           (const double*)d_d.as<double>(), d_x.as<double>(), d_r.as<double>(), d_zp.as<double>(),
                           (const double*)d_p.as<double>(), (const double*)d_q.as<double>(), (const RaCtl*)ctl, t, k, d_P2.as<double>());
        hipLaunchKernelGGL(k_ra_cg_dir, dim3(nbv), dim3(RA_BLOCK), 0, st, N, nbv, (const double*)d_P2.as<double>(),
                           (const double*)d_zp.as<double>(), d_p.as<double>(), ctl, t, k, cg_max, o.cg_tolerance);
      }
      HIPTRY(hipGetLastError());
      read_ctl();
      if (t >= 0 && t >= h.admm_stop) break;
      if (h.cg_stop <= k0 + batch || k0 + batch >= cg_max) break;
    }
    if (rc == DSM_OK && h.cg_worst > o.cg_max_residual) {
      ctx->err = "dsm_view_graph_rotation_averaging: a conjugate-gradient solve ended at a relative residual of " +
                 std::to_string(h.cg_worst);
      rc = DSM_ERR_NOT_CONVERGED;
    }
  };
  auto rotate_and_check = [&](double thr, int irls) {
    hipLaunchKernelGGL(k_ra_rotate, dim3(nbv), dim3(RA_BLOCK), 0, st, N, (const double*)d_x.as<double>(), d_R.as<double>(), d_P3.as<double>());
    residuals();
    hipLaunchKernelGGL(k_ra_step_check, dim3(1), dim3(RA_BLOCK), 0, st, nbv, (const double*)d_P3.as<double>(), N - 1, thr, irls, ctl);
    HIPTRY(hipGetLastError());
    read_ctl();
  };
  if (rc == DSM_OK) {
    hipLaunchKernelGGL(k_ra_fill, dim3((M + RA_BLOCK - 1) / RA_BLOCK), dim3(RA_BLOCK), 0, st, d_one.as<double>(), (size_t)M, 1.0);
    residuals();
  }
  // L1 regression (SolveL1Regression, :196-223): ADMM Solve with a cap that doubles per outer iteration
  int admm_cap = o.admm_initial_max_iterations;
  const double primal_abs = sqrt((double)m3) * o.admm_absolute_tolerance, dual_abs = sqrt(3.0 * (N - 1)) * o.admm_absolute_tolerance;
  for (int it = 0; rc == DSM_OK && it < o.max_num_l1_iterations; ++it) {
    HIPTRY(hipMemsetAsync(d_z.p, 0, m3 * 8, st));
    HIPTRY(hipMemsetAsync(d_u.p, 0, m3 * 8, st));
    HIPTRY(hipMemcpyAsync(&ctl->admm_stop, kAdmmReset, sizeof(kAdmmReset), hipMemcpyHostToDevice, st));
    for (int t = 0; rc == DSM_OK && t < admm_cap; ++t) {
      hipLaunchKernelGGL(k_ra_rhs, dim3(nbv), dim3(RA_BLOCK), 0, st, N, off_, ce_, 0, (const double*)d_b.as<double>(),
                         (const double*)d_z.as<double>(), (const double*)d_u.as<double>(), (const double*)d_w.as<double>(),
                         d_rhs.as<double>(), (const RaCtl*)ctl, t);
      solve(d_one.as<double>(), t);
      if (rc != DSM_OK || t >= h.admm_stop) break;
      hipLaunchKernelGGL(k_ra_admm_edges, dim3(nbe), dim3(RA_BLOCK), 0, st, M, d_ei.as<uint32_t>(), d_ej.as<uint32_t>(),
                         (const double*)d_x.as<double>(), (const double*)d_b.as<double>(), d_z.as<double>(), d_zold.as<double>(),
                         d_u.as<double>(), o.admm_alpha, o.admm_rho, ctl, t, d_P1.as<double>());
      hipLaunchKernelGGL(k_ra_admm_verts, dim3(nbv), dim3(RA_BLOCK), 0, st, N, off_, ce_, (const double*)d_z.as<double>(),
                         (const double*)d_zold.as<double>(), (const double*)d_u.as<double>(), o.admm_rho, (const RaCtl*)ctl, t,
                         d_P2.as<double>());
      hipLaunchKernelGGL(k_ra_admm_check, dim3(1), dim3(RA_BLOCK), 0, st, nbe, (const double*)d_P1.as<double>(),
                         (const double*)d_P4.as<double>(), nbv, (const double*)d_P2.as<double>(), primal_abs, dual_abs,
                         o.admm_relative_tolerance, ctl, t);
      HIPTRY(hipGetLastError());
    }
    if (rc != DSM_OK) break;
    read_ctl();
    rep.admm_iterations[it] = (uint32_t)h.admm_iters;
    rep.num_l1_iterations = it + 1;
    rotate_and_check(o.l1_step_convergence_threshold, 0);
    rep.last_l1_step = h.last_step;
    if (h.step_stop) break;
    admm_cap *= 2;
  }
  // IRLS (SolveIRLS, :225-268)
  for (int it = 0; rc == DSM_OK && it < o.max_num_irls_iterations; ++it) {
    hipLaunchKernelGGL(k_ra_rhs, dim3(nbv), dim3(RA_BLOCK), 0, st, N, off_, ce_, 1, (const double*)d_b.as<double>(),
                       (const double*)d_z.as<double>(), (const double*)d_u.as<double>(), (const double*)d_w.as<double>(),
                       d_rhs.as<double>(), (const RaCtl*)ctl, -1);
    solve(d_w.as<double>(), -1);
    if (rc != DSM_OK) break;
    rep.num_irls_iterations = it + 1;
    rotate_and_check(o.irls_step_convergence_threshold, 1);
    rep.last_irls_step = h.last_step;
    if (h.step_stop) break;
  }
  if (rc == DSM_OK) {
    const double thr = o.max_relative_rotation_difference_degrees * kRaDegToRad;
    hipLaunchKernelGGL(k_ra_filter, dim3(nbe), dim3(RA_BLOCK), 0, st, M, d_ei.as<uint32_t>(), d_ej.as<uint32_t>(), d_r12.as<double>(),
                       (const double*)d_R.as<double>(), thr * thr, d_state.as<uint8_t>(), d_rel.as<double>());
    HIPTRY(hipGetLastError());
    HIPTRY(hipEventRecord(ev1, st));
    HIPTRY(hipMemcpyAsync(Rh.data(), d_R.p, n3 * 8, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(st8.data(), d_state.p, M, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(relh.data(), d_rel.p, m3 * 8, hipMemcpyDeviceToHost, st));
    HIPTRY(hipMemcpyAsync(&h, d_ctl.p, sizeof(RaCtl), hipMemcpyDeviceToHost, st));
    HIPTRY(hipStreamSynchronize(st));
    HIPTRY(dev_events_ms(ev0, ev1, &rep.device_ms));
  }
  if (rc != DSM_OK) (void)hipStreamSynchronize(st);
  rep.total_cg_iterations = h.cg_total;
  rep.max_cg_relative_residual = h.cg_worst;
  if (rc == DSM_OK) {
    ra_write_outputs(g, st8, relh, Rh, image_ids_out, orientations_out, image_in_final_cc, n_images_out, edge_state, relative_rotations_out,
                     &rep.num_filtered_edges, &rep.num_final_images);
  } else {
    for (uint32_t e = 0; e < n_pairs; ++e) edge_state[e] = 0;
  }
  if (report) *report = rep;
  return rc;
}
