// pose_refinement.hip -- batched absolute pose refinement: RefineAbsolutePose (src/estimators/pose.cc:198-311) as
// IncrementalMapper::RegisterNextImage calls it (src/sfm/incremental_mapper.cc:498-535), for a batch of independent problems
// (DESIGN.md 15).  BundleAdjustmentCostFunction with the 3D point constant under ceres::CauchyLoss, qvec through
// QuaternionParameterization, tvec free, the camera's focal / extra parameters free by the problem's flags; the trust-region
// rulings of DESIGN.md 12 (trust_region.h), the damped normal equations solved by an unpivoted Cholesky.
//
// One kernel, k_pr_refine: a one-wave workgroup per problem runs the whole Levenberg-Marquardt loop.  Per evaluation the 64 lanes
// walk the problem's points (lane l takes points l, l + 64, ...): residual and Jacobian through ba_project.h's dual numbers, the
// loss-corrected rows to the problem's workspace (SoA), then J'J row by row and J'r as fixed-order tree sums (the lane's in-order
// partial sums, then the xor butterfly 32 .. 1).  Lane 0 scales, factors, solves, decides and applies Plus.  No host round trips,
// no floating-point atomics; a result depends on the problem and the options alone.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "ba_project.h"
#include "ctx.h"
#include "trust_region.h"
#include "wave_reduce.h"

namespace {

constexpr int PR_P = 16;               // free tangent dimensions at most: qvec 3, tvec 3, camera 10 (FULL_OPENCV / THIN_PRISM_FISHEYE)
constexpr int PR_ROW = 2 * PR_P + 2;   // workspace doubles per point: the two corrected Jacobian rows, the corrected residual
constexpr int PR_MARGINS = DSM_POSE_REFINEMENT_MARGINS;

struct PrParams {
  uint32_t B;
  TrOptions tr;  // ceres' defaults but for gradient_tolerance and max_num_iterations
  double b, c;   // CauchyLoss: b = scale^2, c = 1 / b
  const dsm_camera* cams;
  const uint64_t* offsets;
  const double* xy;
  const double* X;
  const uint8_t* mask;
  const double* q_in;
  const double* t_in;
  const uint8_t* flags;
  double* ws;  // [offsets[B]][PR_ROW], SoA inside a problem
  dsm_pose_refinement_result* res;
  double* margins;  // [B][PR_MARGINS]
  uint8_t* steps;   // [B][tr.max_iterations]
};

struct PrState {
  double q[4], t[3], prm[12];
};

struct PrShared : TrState {
  TrOptions opt;  // the kernel's, beside the state: lane 0's device functions take one pointer
  PrState x, cand;
  double A[PR_P * PR_P];  // J'J of the corrected Jacobian (upper triangle from the sums, mirrored), then scaled in place
  double L[PR_P * PR_P];
  double g[PR_P], gs[PR_P], s[PR_P], D[PR_P], step[PR_P], delta[PR_P];
  double cand_cost, mcc, s2;
  double m_pivot;  // the smallest Cholesky pivot relative to its diagonal entry
  int fr[PR_P];    // the free camera parameter indices
  int model, np, k, P, cam_var, valid;
};

struct PrView {
  const double* xy;
  const double* X;
  const uint8_t* mask;
  double* ws;
  int N;
  double b, c;
};

// one copy each of the projection's dual instantiation and of Plus in this file's code (the library's size cap)
__device__ __noinline__ void pr_project(int model, int np, const double* prm, double u, double v, BaDual* x, BaDual* y) {
  ba_project_dual(model, np, prm, u, v, x, y);
}
__device__ __noinline__ void pr_quat_plus(const double* x, const double* d, double* out) { ba_quat_plus(x, d, out); }

// The cost 1/2 sum rho(|r|^2) of state st over the inlier points (every lane returns it); with jac the corrected rows go to the
// workspace.  Corrector (ceres/internal/corrector.cc): CauchyLoss has rho'' < 0, so the first branch holds for every residual:
// residual and Jacobian rows are both scaled by sqrt(rho').
__device__ __noinline__ double pr_eval(const PrView& v, const PrShared* sm, const PrState* st, int lane, bool jac) {
  double q[4], t[3], prm[12];
  for (int i = 0; i < 4; ++i) q[i] = st->q[i];
  for (int i = 0; i < 3; ++i) t[i] = st->t[i];
  for (int i = 0; i < 12; ++i) prm[i] = st->prm[i];
  const int model = sm->model, np = sm->np, k = sm->k;
  double acc = 0.0;
  for (int i = lane; i < v.N; i += 64) {
    if (!v.mask[i]) continue;  // adds +0.0
    double w[3];
    ba_rotate(q, v.X + 3 * (size_t)i, w);
    const double P0 = w[0] + t[0], P1 = w[1] + t[1], P2 = w[2] + t[2];
    const double pu = P0 / P2, pv = P1 / P2;
    BaDual xx, yy;
    pr_project(model, np, prm, pu, pv, &xx, &yy);
    const double r0 = xx.v - v.xy[2 * (size_t)i], r1 = yy.v - v.xy[2 * (size_t)i + 1];
    const double s = r0 * r0 + r1 * r1;
    const double sum = 1.0 + s * v.c;  // CauchyLoss::Evaluate
    const double inv = 1.0 / sum;
    acc += 0.5 * (v.b * log(sum));
    if (!jac) continue;
    const double sq = sqrt(fmax(DBL_MIN, inv));
    double JP[2][3], Dq[9];
    ba_pixel_jacobian(xx, yy, P0, P1, P2, w, JP, Dq);
    double* row = v.ws + i;
    const size_t N = (size_t)v.N;
    for (int r = 0; r < 2; ++r) {
      const BaDual& dd = r ? yy : xx;
      for (int a = 0; a < 3; ++a) {
        row[(size_t)(r * PR_P + a) * N] = sq * (JP[r][0] * Dq[a] + JP[r][1] * Dq[3 + a] + JP[r][2] * Dq[6 + a]);
        row[(size_t)(r * PR_P + 3 + a) * N] = sq * JP[r][a];
      }
      for (int j = 0; j < PR_P - 6; ++j) {
        double dj = 0.0;
        if (j < k) dj = dd.d[2 + sm->fr[j]];
        row[(size_t)(r * PR_P + 6 + j) * N] = sq * dj;
      }
    }
    row[(size_t)(2 * PR_P) * N] = sq * r0;
    row[(size_t)(2 * PR_P + 1) * N] = sq * r1;
  }
  return wave_sum(acc);
}

// J'J (row a: entries a .. P - 1) and J'r from the workspace rows, one row of the triangle per pass
__device__ __noinline__ void pr_normal(const PrView& v, PrShared* sm, int lane) {
  const int P = sm->P;
  const size_t N = (size_t)v.N;
  for (int a = 0; a < P; ++a) {
    double acc[PR_P + 1];
#pragma unroll
    for (int b = 0; b <= PR_P; ++b) acc[b] = 0.0;
    for (int i = lane; i < v.N; i += 64) {
      if (!v.mask[i]) continue;
      const double* row = v.ws + i;
      const double j0 = row[(size_t)a * N], j1 = row[(size_t)(PR_P + a) * N];
#pragma unroll
      for (int b = 0; b < PR_P; ++b)
        if (b >= a && b < P) acc[b] += j0 * row[(size_t)b * N] + j1 * row[(size_t)(PR_P + b) * N];
      acc[PR_P] += j0 * row[(size_t)(2 * PR_P) * N] + j1 * row[(size_t)(2 * PR_P + 1) * N];
    }
#pragma unroll
    for (int b = 0; b <= PR_P; ++b) acc[b] = wave_sum(acc[b]);
    if (lane == 0) {
#pragma unroll
      for (int b = 0; b < PR_P; ++b)
        if (b >= a && b < P) sm->A[a * PR_P + b] = sm->A[b * PR_P + a] = acc[b];
      sm->g[a] = acc[PR_P];
    }
  }
}

// lane 0, after an evaluation: Jacobi scaling (from the first Jacobian), the scaled system, D, the gradient max-norm
__device__ __noinline__ void pr_scale(PrShared* sm, bool first) {
  const int P = sm->P;
  double cn[PR_P];
  for (int j = 0; j < P; ++j) {
    cn[j] = sm->A[j * PR_P + j];
    if (first) sm->s[j] = 1.0 / (1.0 + sqrt(cn[j]));
  }
  for (int a = 0; a < P; ++a) {
    for (int b = 0; b < P; ++b) sm->A[a * PR_P + b] = (sm->s[a] * sm->A[a * PR_P + b]) * sm->s[b];
    sm->gs[a] = sm->s[a] * sm->g[a];
    sm->D[a] = fmin(fmax((sm->s[a] * sm->s[a]) * cn[a], kLmMinDiag), kLmMaxDiag);
  }
  // |x - Plus(x, -g)|inf over the variable blocks, g unscaled
  double ng[3] = {-sm->g[0], -sm->g[1], -sm->g[2]}, qp[4], m = 0.0;
  pr_quat_plus(sm->x.q, ng, qp);
  for (int i = 0; i < 4; ++i) m = fmax(m, fabs(sm->x.q[i] - qp[i]));
  for (int i = 0; i < 3; ++i) m = fmax(m, fabs(sm->x.t[i] - (sm->x.t[i] - sm->g[3 + i])));
  for (int j = 0; j < sm->k; ++j) {
    const double p = sm->x.prm[sm->fr[j]];
    m = fmax(m, fabs(p - (p - sm->g[6 + j])));
  }
  sm->gnorm = m;
}

// lane 0: (A + diag(sqrt(D / radius)^2)) step = -gs by an unpivoted Cholesky, model_cost_change, the candidate.  A pivot that is
// not positive and finite makes the step invalid.
__device__ __noinline__ void pr_step(PrShared* sm) {
  const int P = sm->P;
  double* L = sm->L;
  bool ok = true;
  for (int i = 0; i < P && ok; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = sm->A[i * PR_P + j];
      if (i == j) {
        const double l = sqrt(sm->D[i] / sm->radius);
        s += l * l;
      }
      const double diag = s;
      for (int m = 0; m < j; ++m) s -= L[i * PR_P + m] * L[j * PR_P + m];
      if (i == j) {
        tr_min(&sm->m_pivot, isfinite(s) && diag > 0.0 ? fabs(s) / diag : 0.0);
        if (!(s > 0.0) || !isfinite(s)) {
          ok = false;
          break;
        }
        L[i * PR_P + i] = sqrt(s);
      } else {
        L[i * PR_P + j] = s / L[j * PR_P + j];
      }
    }
  sm->valid = 0;
  sm->mcc = sm->s2 = 0.0;
  if (!ok) return;
  double w[PR_P];
  for (int i = 0; i < P; ++i) {
    double s = -sm->gs[i];
    for (int m = 0; m < i; ++m) s -= L[i * PR_P + m] * w[m];
    w[i] = s / L[i * PR_P + i];
  }
  for (int i = P - 1; i >= 0; --i) {
    double s = w[i];
    for (int m = i + 1; m < P; ++m) s -= L[m * PR_P + i] * w[m];
    w[i] = s / L[i * PR_P + i];
  }
  // model_cost_change = -(J step)'(r + J step / 2) = -step'(gs + A step / 2)
  double mcc = 0.0, s2 = 0.0;
  for (int i = 0; i < P; ++i) {
    double as = 0.0;
    for (int j = 0; j < P; ++j) as += sm->A[i * PR_P + j] * w[j];
    mcc += w[i] * (sm->gs[i] + as / 2.0);
    sm->step[i] = w[i];
    sm->delta[i] = sm->s[i] * w[i];
    s2 += sm->delta[i] * sm->delta[i];
  }
  sm->mcc = -mcc;
  sm->s2 = s2;
  sm->cand = sm->x;
  pr_quat_plus(sm->x.q, sm->delta, sm->cand.q);
  for (int i = 0; i < 3; ++i) sm->cand.t[i] = sm->x.t[i] + sm->delta[3 + i];
  for (int j = 0; j < sm->k; ++j) sm->cand.prm[sm->fr[j]] = sm->x.prm[sm->fr[j]] + sm->delta[6 + j];
  sm->valid = tr_step_usable(sm->mcc, s2);
}

// lane 0: the decision of one iteration (trust_region.h); returns the step's code
__device__ __noinline__ int pr_decide(PrShared* sm) {
  double x2 = 0.0;
  for (int i = 0; i < 4; ++i) x2 += sm->x.q[i] * sm->x.q[i];
  for (int i = 0; i < 3; ++i) x2 += sm->x.t[i] * sm->x.t[i];
  if (sm->cam_var)
    for (int i = 0; i < sm->np; ++i) x2 += sm->x.prm[i] * sm->x.prm[i];
  const int code = tr_decide(sm, sm->opt, sm->valid != 0, sm->cand_cost, sm->mcc, sm->s2, x2);
  if (code == TR_ACCEPTED) sm->x = sm->cand;
  return code;
}

__global__ void __launch_bounds__(64) k_pr_refine(PrParams p) {
  __shared__ PrShared sm;
  const int lane = threadIdx.x;
  const uint32_t b = blockIdx.x;
  if (b >= p.B) return;
  const dsm_camera cam = p.cams[b];
  PrView v;
  const uint64_t off = p.offsets[b];
  v.N = (int)(p.offsets[b + 1] - off);
  v.xy = p.xy + 2 * off;
  v.X = p.X + 3 * off;
  v.mask = p.mask + off;
  v.ws = p.ws + (size_t)PR_ROW * off;
  v.b = p.b;
  v.c = p.c;
  int n_in = 0;
  for (int i = lane; i < v.N; i += 64) n_in += v.mask[i] != 0;
  n_in = wave_sum(n_in);
  dsm_pose_refinement_result* out = &p.res[b];
  if (lane == 0) {
    tr_init(&sm, kTrInitialRadius);
    sm.opt = p.tr;
    sm.m_pivot = INFINITY;
    sm.model = cam.model_id;
    sm.np = cam_num_params(cam.model_id);
    const int nfoc = cam_two_focal(cam.model_id) ? 2 : 1;
    int k = 0;
    for (int j = 0; j < sm.np; ++j) {  // the principal point is always constant (pose.cc:255-261)
      const bool free_j = j < nfoc ? (p.flags[b] & 1) : (j >= nfoc + 2 && (p.flags[b] & 2));
      if (free_j) sm.fr[k++] = j;
    }
    sm.k = k;
    sm.P = 6 + k;
    sm.cam_var = k > 0;
    for (int i = 0; i < 4; ++i) sm.x.q[i] = p.q_in[4 * (size_t)b + i];
    for (int i = 0; i < 3; ++i) sm.x.t[i] = p.t_in[3 * (size_t)b + i];
    for (int i = 0; i < 12; ++i) sm.x.prm[i] = i < sm.np ? cam.params[i] : 0.0;
    if (n_in > 0) {  // NormalizeQuaternion (pose.cc:246); an empty problem leaves qvec as it came
      const double n = sqrt(sm.x.q[0] * sm.x.q[0] + sm.x.q[1] * sm.x.q[1] + sm.x.q[2] * sm.x.q[2] + sm.x.q[3] * sm.x.q[3]);
      if (n > 0.0) {
        for (int i = 0; i < 4; ++i) sm.x.q[i] /= n;
      } else {  // NormalizeQuaternion's identity for a zero quaternion
        sm.x.q[0] = 1.0;
        sm.x.q[1] = sm.x.q[2] = sm.x.q[3] = 0.0;
      }
    }
  }
  __syncthreads();
  double initial_cost = 0.0;
  if (n_in > 0) {
    const double c0 = pr_eval(v, &sm, &sm.x, lane, true);
    initial_cost = c0;
    __syncthreads();
    pr_normal(v, &sm, lane);
    if (lane == 0) {
      sm.cost = c0;
      if (!isfinite(c0)) {
        tr_finish(&sm, TR_FAILURE);
      } else {
        pr_scale(&sm, true);
        tr_end_iteration(&sm, sm.opt, true);
      }
    }
    __syncthreads();
    while (!sm.done) {  // at most max_iterations rounds: tr_decide counts every one, tr_end_iteration stops at the cap
      if (lane == 0) pr_step(&sm);
      __syncthreads();
      const double cc = sm.valid ? pr_eval(v, &sm, &sm.cand, lane, false) : INFINITY;
      if (lane == 0) {
        sm.cand_cost = cc;
        const int code = pr_decide(&sm);
        if (p.steps) p.steps[(size_t)b * p.tr.max_iterations + (sm.iter - 1)] = (uint8_t)code;
      }
      __syncthreads();
      const bool fresh = sm.accepted && !sm.done;
      if (fresh) {
        (void)pr_eval(v, &sm, &sm.x, lane, true);
        __syncthreads();
        pr_normal(v, &sm, lane);
        if (lane == 0) pr_scale(&sm, false);
      }
      if (lane == 0) tr_end_iteration(&sm, sm.opt, fresh);
      __syncthreads();
    }
  }
  if (lane == 0) {
    out->success = sm.term != DSM_BA_FAILURE;  // Solver::Summary::IsSolutionUsable
    out->termination = sm.term;
    out->num_iterations = (uint32_t)sm.iter;
    out->num_successful_steps = (uint32_t)sm.n_succ;
    out->num_invalid_steps = (uint32_t)sm.n_invalid_total;
    out->num_residual_blocks = (uint32_t)n_in;
    out->initial_cost = initial_cost;
    out->final_cost = sm.cost;
    for (int i = 0; i < 4; ++i) out->qvec[i] = sm.x.q[i];
    for (int i = 0; i < 3; ++i) out->tvec[i] = sm.x.t[i];
    for (int i = 0; i < 12; ++i) out->camera_params[i] = i < sm.np ? sm.x.prm[i] : cam.params[i];
    const double mg[PR_MARGINS] = {sm.m_accept, sm.m_grad, sm.m_func, sm.m_param, sm.m_pivot};
    for (int i = 0; i < PR_MARGINS; ++i) p.margins[(size_t)b * PR_MARGINS + i] = mg[i];
  }
}

bool pr_options_ok(const dsm_pose_refinement_options& o) {
  // AbsolutePoseRefinementOptions::Check (pose.h:99-103); non-finite values fail
  return o.gradient_tolerance >= 0.0 && std::isfinite(o.gradient_tolerance) && o.max_num_iterations >= 0 &&
         o.loss_function_scale >= 0.0 && std::isfinite(o.loss_function_scale);
}

struct PrBufs {
  DevBuf cams, offsets, xy, X, mask, q, t, flags, ws, res, margins, steps;
};

}  // namespace

extern "C" void dsm_default_pose_refinement_options(dsm_pose_refinement_options* o) {
  o->gradient_tolerance = 1.0;   // pose.h:82
  o->loss_function_scale = 1.0;  // pose.h:88
  o->max_num_iterations = 100;   // pose.h:85
  o->reserved = 0;
}

extern "C" int dsm_refine_absolute_poses(dsm_ctx* ctx, uint32_t num_problems, const dsm_camera* cameras, const uint64_t* offsets,
                                         const double* points2D, const double* points3D, const uint8_t* inlier_mask,
                                         const double* qvecs_in, const double* tvecs_in, const uint8_t* refine_flags,
                                         const dsm_pose_refinement_options* options, dsm_pose_refinement_result* results_out,
                                         double* margins_out, uint8_t* steps_out, dsm_pose_refinement_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_refine_absolute_poses", msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  const uint32_t B = num_problems;
  if (!offsets || (B && (!cameras || !qvecs_in || !tvecs_in || !refine_flags || !results_out))) return fail("NULL argument");
  dsm_pose_refinement_options o;
  if (options)
    o = *options;
  else
    dsm_default_pose_refinement_options(&o);
  if (!pr_options_ok(o)) return fail("option out of range");
  if (o.loss_function_scale == 0.0) return fail("loss_function_scale = 0 divides by zero in the loss");
  if (o.max_num_iterations > (int32_t)DSM_POSE_REFINEMENT_MAX_ITERATIONS)
    return fail("max_num_iterations above 1000: the loop runs inside one launch");
  if (offsets[0] != 0) return fail("offsets must start at 0");
  for (uint32_t b = 0; b < B; ++b) {
    if (offsets[b + 1] < offsets[b]) return fail("offsets must ascend");
    if (offsets[b + 1] - offsets[b] > DSM_ABSOLUTE_POSE_MAX_POINTS) return fail("more than 1048576 correspondences in one problem");
  }
  const uint64_t T = offsets[B];
  if (T >= 0x80000000ull / PR_ROW) return fail("too many correspondences in one call");
  if (T && (!points2D || !points3D || !inlier_mask)) return fail("NULL argument");
  for (uint64_t i = 0; i < 2 * T; ++i)
    if (!std::isfinite(points2D[i])) return fail("non-finite points2D");
  for (uint64_t i = 0; i < 3 * T; ++i)
    if (!std::isfinite(points3D[i])) return fail("non-finite points3D");
  for (uint32_t b = 0; b < B; ++b) {
    const dsm_camera& k = cameras[b];
    if (!cam_model_exists(k.model_id)) return fail("an unknown camera model");
    for (int i = 0; i < cam_num_params(k.model_id); ++i)
      if (!std::isfinite(k.params[i])) return fail("non-finite camera parameters");
    for (int i = 0; i < 4; ++i)
      if (!std::isfinite(qvecs_in[4 * (size_t)b + i])) return fail("non-finite qvec");
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(tvecs_in[3 * (size_t)b + i])) return fail("non-finite tvec");
    if (refine_flags[b] > 3) return fail("refine_flags above 3");
  }
  dsm_pose_refinement_report rep{};
  rep.num_problems = B;
  rep.num_points = T;
  for (int i = 0; i < PR_MARGINS; ++i) rep.min_margin[i] = INFINITY;
  rep.setup_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count();
  if (B == 0) {
    if (report) *report = rep;
    return DSM_OK;
  }
  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  PrBufs d;
  DevEvents<4> ev;
  HIPCHK(ctx, ev.create());
  HIPCHK(ctx, hipEventRecord(ev[0], st));
  const size_t steps_bytes = (size_t)B * (size_t)o.max_num_iterations;
  HIPCHK(ctx, dev_upload(d.cams, cameras, (size_t)B * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(d.offsets, offsets, ((size_t)B + 1) * 8, st));
  HIPCHK(ctx, dev_upload(d.xy, points2D, T * 16, st));
  HIPCHK(ctx, dev_upload(d.X, points3D, T * 24, st));
  HIPCHK(ctx, dev_upload(d.mask, inlier_mask, T, st));
  HIPCHK(ctx, dev_upload(d.q, qvecs_in, (size_t)B * 32, st));
  HIPCHK(ctx, dev_upload(d.t, tvecs_in, (size_t)B * 24, st));
  HIPCHK(ctx, dev_upload(d.flags, refine_flags, B, st));
  HIPCHK(ctx, d.ws.reserve(std::max<size_t>(T, 1) * PR_ROW * 8));
  HIPCHK(ctx, d.res.reserve((size_t)B * sizeof(dsm_pose_refinement_result)));
  HIPCHK(ctx, d.margins.reserve((size_t)B * PR_MARGINS * 8));
  HIPCHK(ctx, d.steps.reserve(std::max<size_t>(steps_bytes, 16)));
  if (steps_bytes) HIPCHK(ctx, hipMemsetAsync(d.steps.p, 0, steps_bytes, st));
  PrParams prm;
  prm.B = B;
  prm.tr = tr_ceres_defaults();
  prm.tr.max_iterations = o.max_num_iterations;
  prm.tr.gtol = o.gradient_tolerance;
  prm.b = o.loss_function_scale * o.loss_function_scale;  // CauchyLoss(a): b_(a * a), c_(1 / b_)
  prm.c = 1.0 / prm.b;
  prm.cams = d.cams.as<dsm_camera>();
  prm.offsets = d.offsets.as<uint64_t>();
  prm.xy = d.xy.as<double>();
  prm.X = d.X.as<double>();
  prm.mask = d.mask.as<uint8_t>();
  prm.q_in = d.q.as<double>();
  prm.t_in = d.t.as<double>();
  prm.flags = d.flags.as<uint8_t>();
  prm.ws = d.ws.as<double>();
  prm.res = d.res.as<dsm_pose_refinement_result>();
  prm.margins = d.margins.as<double>();
  prm.steps = steps_bytes ? d.steps.as<uint8_t>() : nullptr;
  HIPCHK(ctx, hipEventRecord(ev[1], st));
  hipLaunchKernelGGL(k_pr_refine, dim3(B), dim3(64), 0, st, prm);
  HIPCHK(ctx, hipGetLastError());
  HIPCHK(ctx, hipEventRecord(ev[2], st));
  std::vector<double> margins((size_t)B * PR_MARGINS);
  HIPCHK(ctx, hipMemcpyAsync(results_out, d.res.p, (size_t)B * sizeof(dsm_pose_refinement_result), hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(margins.data(), d.margins.p, margins.size() * 8, hipMemcpyDeviceToHost, st));
  if (steps_out && steps_bytes) HIPCHK(ctx, hipMemcpyAsync(steps_out, d.steps.p, steps_bytes, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipEventRecord(ev[3], st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (uint32_t b = 0; b < B; ++b) {
    rep.num_iterations += results_out[b].num_iterations;
    for (int i = 0; i < PR_MARGINS; ++i) {
      rep.min_margin[i] = std::min(rep.min_margin[i], margins[(size_t)b * PR_MARGINS + i]);
      if (margins_out) margins_out[(size_t)b * PR_MARGINS + i] = margins[(size_t)b * PR_MARGINS + i];
    }
  }
  HIPCHK(ctx, ev.ms(0, 1, &rep.upload_ms));
  HIPCHK(ctx, ev.ms(1, 2, &rep.solve_ms));
  HIPCHK(ctx, ev.ms(2, 3, &rep.download_ms));
  HIPCHK(ctx, ev.ms(0, 3, &rep.device_ms));
  if (report) *report = rep;
  return DSM_OK;
}
