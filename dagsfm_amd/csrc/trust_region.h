// trust_region.h -- Ceres' TrustRegionMinimizer and LevenbergMarquardtStrategy as DESIGN.md 12 rules on them, stated once for
// the four Levenberg-Marquardt solvers (bundle_adjustment.hip, local_bundle.hip, pose_refinement.hip, nonlinear_rotation.hip):
// the decision on one step and the checks that end an iteration.  A solver keeps how it reduces model_cost_change, |delta|^2
// and |x|^2, what makes its linear solve fail, and what it does with an accepted step; it calls tr_decide once per iteration
// from one thread, acts on the returned code, and calls tr_end_iteration once the gradient of an accepted step is there.
//
// Plain C++: no HIP in it beyond the function qualifier, so the host build (trust_region_host.cpp ->
// libdsm_trust_region.so) runs the same statements under tests/test_trust_region_cpu.py.  Plain IEEE double operations in a
// fixed order, no FMA (every build uses -ffp-contract=off): the host compiler and hipcc give the same bits.
#ifndef DAGSFM_AMD_CSRC_TRUST_REGION_H_
#define DAGSFM_AMD_CSRC_TRUST_REGION_H_

#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#define DSM_TR static __host__ __device__ inline
#else
#define DSM_TR static inline
#endif

// what became of a step: the codes dsm_refine_absolute_poses writes to steps_out
enum { TR_ACCEPTED = 1, TR_REJECTED = 2, TR_INVALID = 3, TR_TOLERANCE = 4 };
// ceres::TerminationType as include/dagsfm_mi355x.h names it (DSM_BA_*); a solver may add codes of its own above these
enum { TR_CONVERGENCE = 0, TR_NO_CONVERGENCE = 1, TR_FAILURE = 2 };

// ceres::Solver::Options' defaults that no public option of BA, local bundle or pose refinement reaches
constexpr double kTrInitialRadius = 1e4, kTrMaxRadius = 1e16, kTrMinRadius = 1e-32, kTrMinRelDecrease = 1e-3;
constexpr double kTrFunctionTolerance = 1e-6, kTrParameterTolerance = 1e-8;
constexpr int kTrMaxInvalidSteps = 5;
constexpr double kLmMinDiag = 1e-6, kLmMaxDiag = 1e32;  // LevenbergMarquardtStrategy's clamp of diag J'J

struct TrOptions {
  double ftol, gtol, ptol, min_relative_decrease, max_radius, min_radius;
  int max_iterations, max_consecutive_invalid_steps;
};

// The loop's state.  `done` ends the loop and `term` says how; while the loop runs term is TR_CONVERGENCE and means nothing.
// The margins are the smallest relative distance of each test from flipping over the calls so far: the acceptance test's in
// cost, the others |value - threshold| / max(|value|, |threshold|).
struct TrState {
  double cost, radius, dec, last_rho, gnorm;  // dec: the factor the next rejected or invalid step divides the radius by
  double m_accept, m_grad, m_func, m_param;
  int iter, n_succ, n_rej, n_invalid, n_invalid_total;  // n_invalid: consecutive
  int accepted, term, done;
};

DSM_TR TrOptions tr_ceres_defaults() {
  TrOptions o;
  o.ftol = kTrFunctionTolerance;
  o.gtol = 1e-10;
  o.ptol = kTrParameterTolerance;
  o.min_relative_decrease = kTrMinRelDecrease;
  o.max_radius = kTrMaxRadius;
  o.min_radius = kTrMinRadius;
  o.max_iterations = 50;
  o.max_consecutive_invalid_steps = kTrMaxInvalidSteps;
  return o;
}

DSM_TR void tr_init(TrState* s, double initial_radius) {
  s->cost = s->gnorm = 0.0;
  s->radius = initial_radius;
  s->dec = 2.0;
  s->last_rho = NAN;
  s->m_accept = s->m_grad = s->m_func = s->m_param = INFINITY;
  s->iter = s->n_succ = s->n_rej = s->n_invalid = s->n_invalid_total = 0;
  s->accepted = 0;
  s->term = TR_CONVERGENCE;
  s->done = 0;
}

DSM_TR void tr_finish(TrState* s, int term) {
  s->term = term;
  s->done = 1;
}

// the relative distance of a from its threshold; a non-finite a is no decision that rounding can flip
DSM_TR double tr_margin(double a, double thr) {
  if (!isfinite(a)) return INFINITY;
  const double den = fmax(fabs(a), fabs(thr));
  return den > 0.0 ? fabs(a - thr) / den : 0.0;
}
// a margin keeps its minimum; a NaN never replaces it
DSM_TR void tr_min(double* m, double v) {
  if (v < *m) *m = v;
}

// what every solver asks of a step before the candidate is worth evaluating
DSM_TR bool tr_step_usable(double model_cost_change, double step2) {
  return isfinite(model_cost_change) && model_cost_change > 0.0 && isfinite(step2);
}

// The decision of one iteration.  solved: the solver's own linear solve gave a step; cand_cost: the cost at x + step;
// step2 = |delta|^2 and x2 = |x|^2 over the variable blocks.  Counts the iteration, updates cost, radius and the counters, and
// returns the step's code; on TR_ACCEPTED the caller commits its candidate, on TR_TOLERANCE the step is not applied.
DSM_TR int tr_decide(TrState* s, const TrOptions& o, bool solved, double cand_cost, double model_cost_change, double step2, double x2) {
  s->iter += 1;
  s->accepted = 0;
  s->last_rho = NAN;
  if (!(solved && tr_step_usable(model_cost_change, step2) && isfinite(cand_cost))) {
    s->n_invalid += 1;
    s->n_invalid_total += 1;
    if (s->n_invalid >= o.max_consecutive_invalid_steps) {
      tr_finish(s, TR_FAILURE);
    } else {
      s->radius /= s->dec;
      s->dec *= 2.0;
    }
    return TR_INVALID;
  }
  s->n_invalid = 0;
  const double step_norm = sqrt(step2), ptol = o.ptol * (sqrt(x2) + o.ptol);
  tr_min(&s->m_param, tr_margin(step_norm, ptol));
  if (step_norm <= ptol) {
    tr_finish(s, TR_CONVERGENCE);
    return TR_TOLERANCE;
  }
  const double change = s->cost - cand_cost;
  tr_min(&s->m_func, tr_margin(fabs(change), o.ftol * s->cost));
  if (fabs(change) <= o.ftol * s->cost) {
    tr_finish(s, TR_CONVERGENCE);
    return TR_TOLERANCE;
  }
  const double rho = change / model_cost_change;
  s->last_rho = rho;
  // near the optimum the cost change itself is rounding, and so is rho: the distance from flipping is measured in cost
  tr_min(&s->m_accept, fabs(change - o.min_relative_decrease * model_cost_change) / fmax(s->cost, DBL_MIN));
  if (rho > o.min_relative_decrease) {
    s->accepted = 1;
    s->n_succ += 1;
    s->cost = cand_cost;
    const double tmp = 2.0 * rho - 1.0;
    s->radius = fmin(o.max_radius, s->radius / fmax(1.0 / 3.0, 1.0 - tmp * tmp * tmp));
    s->dec = 2.0;
    return TR_ACCEPTED;
  }
  s->n_rej += 1;
  s->radius /= s->dec;
  s->dec *= 2.0;
  return TR_REJECTED;
}

// The checks that end an iteration (and iteration 0): the cap, then with a fresh gradient max-norm in s->gnorm (after an
// accepted step, or at iteration 0) the gradient test, then the smallest radius.
DSM_TR void tr_end_iteration(TrState* s, const TrOptions& o, bool fresh) {
  if (s->done) return;
  if (s->iter >= o.max_iterations) {
    tr_finish(s, TR_NO_CONVERGENCE);
  } else if (fresh) {
    tr_min(&s->m_grad, tr_margin(s->gnorm, o.gtol));
    if (s->gnorm <= o.gtol) tr_finish(s, TR_CONVERGENCE);
  }
  if (!s->done && s->radius < o.min_radius) tr_finish(s, TR_CONVERGENCE);
}

#endif  // DAGSFM_AMD_CSRC_TRUST_REGION_H_
