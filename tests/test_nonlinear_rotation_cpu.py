"""The NONLINEAR global rotation estimator (dsm_view_graph_rotation_averaging_nonlinear) without a device: the numpy
restatement (tests/nonlinear_rotation_ref.py) -- its dual-number Jacobian on every branch, the loss corrector's branch, known
answers, an independent optimiser -- the option defaults, a call site in the reference's C++ dialect, and that every scene of
the device tests is clear by margins and by the conditioning probe."""
import os
import subprocess

import numpy as np
import pytest

from tests import nonlinear_rotation_ref as nl
from tests import rotation_averaging_ref as ra
from tests.nonlinear_rotation_scenes import CHAINED, SCENES
from tests.test_rotation_averaging import _edges_random, _expected_orientations, _graph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def near_pi_triples(angle=np.pi - 1e-3):
    """Three triples whose error rotation R2 R1^T R12^T is `angle` about an axis closest to x, y and z: RotationMatrixToQuaternion's
    three largest-diagonal cases.  R12 = target^T (R2 R1^T)."""
    rng = np.random.default_rng(7)
    a1, a2 = rng.normal(scale=0.7, size=(3, 3)), rng.normal(scale=0.7, size=(3, 3))
    axes = np.eye(3) + 0.2 * rng.normal(size=(3, 3))
    axes /= np.linalg.norm(axes, axis=1, keepdims=True)
    target = ra.angle_axis_to_rotation(angle * axes)
    loop = np.matmul(ra.angle_axis_to_rotation(a2), np.transpose(ra.angle_axis_to_rotation(a1), (0, 2, 1)))
    a12 = ra.rotation_to_angle_axis(np.matmul(np.transpose(target, (0, 2, 1)), loop))
    return a1, a2, a12


def branch_triples():
    """(rotation1, rotation2, relative_rotation) rows: zero orientations with a generic relative rotation (both matrices on the
    first-order branch), a generic triple, the three near-pi cases, and the exact zero residual."""
    rng = np.random.default_rng(3)
    g = rng.normal(scale=0.8, size=(3, 3))
    p1, p2, p12 = near_pi_triples()
    z = np.zeros((1, 3))
    return (np.vstack([z, g[:1], p1, z]), np.vstack([z, g[1:2], p2, z]), np.vstack([g[2:3] * 0.3, g[2:3], p12, z]))


def test_near_pi_triples_take_the_three_largest_diagonal_cases():
    a1, a2, a12 = near_pi_triples()
    M = [ra.angle_axis_to_rotation(a) for a in (a1, a2, a12)]
    err = np.matmul(np.matmul(M[1], np.transpose(M[0], (0, 2, 1))), np.transpose(M[2], (0, 2, 1)))
    assert (np.trace(err, axis1=1, axis2=2) < 0.0).all()
    assert list(np.argmax(err[:, [0, 1, 2], [0, 1, 2]], axis=1)) == [0, 1, 2]
    r = nl.pairwise_rotation_error(a1, a2, a12, corrected=False)[0]
    assert np.allclose(np.linalg.norm(r, axis=1), np.pi - 1e-3, atol=1e-9)


def test_dual_jacobian_equals_central_difference_on_every_branch():
    a1, a2, a12 = (v[:5] for v in branch_triples())
    _, J, _ = nl.pairwise_rotation_error(a1, a2, a12, corrected=False)
    h = 1e-6  # central difference: truncation h^2 |f'''| / 6 ~ 1e-12 |f'''|, rounding eps |f| / h ~ 1e-9 near pi: 1e-6 holds both
    for c in range(6):
        d = np.zeros((5, 6))
        d[:, c] = h
        rp = nl.pairwise_rotation_error(a1 + d[:, :3], a2 + d[:, 3:], a12, corrected=False)[0]
        rm = nl.pairwise_rotation_error(a1 - d[:, :3], a2 - d[:, 3:], a12, corrected=False)[0]
        num = (rp - rm) / (2.0 * h)
        gap = np.abs(num - J[:, c // 3, :, c % 3]).max(axis=1)
        assert (gap < 1e-6).all(), (c, gap)


def test_exact_zero_residual_takes_k2_branch_with_finite_derivatives():
    z = np.zeros((1, 3))
    r, J, rho = nl.pairwise_rotation_error(z, z, z)
    assert np.array_equal(r, z) and np.isfinite(J).all()
    # sin^2 = 0 -> k = 2: the residual is 2 (q1, q2, q3) and q = (R21 - R12, ...) / 4 of I + [w2 - w1]x to first order
    assert np.array_equal(J[0, 0], -np.eye(3)) and np.array_equal(J[0, 1], np.eye(3))
    assert np.array_equal(rho[0], [0.0, 1.0, -(1.0 / (0.1 * 0.1)) / 2.0])
    # an orientation pair that reproduces the relative rotation exactly up to rounding still differentiates finitely
    a = np.array([[0.3, -0.2, 0.5]])
    r, J, _ = nl.pairwise_rotation_error(z, a, a)
    assert np.abs(r).max() < 1e-15 and np.isfinite(J).all()


def test_corrector_takes_its_first_branch_for_every_s():
    s = np.concatenate([[0.0], np.logspace(-30, 2, 400)])
    for width in (0.01, 0.1, 1.0):
        rho = nl.soft_l1(s, width)
        assert (rho[:, 2] < 0.0).all() and (rho[:, 1] > 0.0).all() and (rho[:, 1] <= 1.0).all()
        scaling, alpha_sq, first = nl.corrector(s, rho)
        assert first.all() and np.array_equal(alpha_sq, np.zeros_like(s)) and np.array_equal(scaling, np.sqrt(rho[:, 1]))
    # the other branch exists and is stated: a loss with rho'' > 0 leaves the first one
    fake = np.array([[0.0, 1.0, 0.1]])
    assert not nl.corrector(np.array([0.5]), fake)[2][0]


def test_restatement_noiseless_graph_returns_generating_rotations():
    n = 30
    pairs = _edges_random(np.random.default_rng(1), n, 6)
    p, q, _, absq = _graph(2, n, pairs, shuffle=False)
    out = nl.rotation_averaging_nonlinear(p, q)
    assert out["report"]["num_images"] == n and (out["edge_state"] == 3).all() and out["in_final_cc"].all()
    assert out["report"]["termination"] == nl.CONVERGENCE and out["accepted"][-1] == 0
    gap = ra.angle_between(nl.relative_to_first(out["orientations"]), _expected_orientations(absq, np.arange(n))).max()
    # With ceres' defaults the run ends at the parameter tolerance: a valid step of |step| <= 1e-8 (|x| + 1e-8) is not applied
    # (DESIGN.md 12).  At a zero-residual optimum that Gauss-Newton step is the remaining error to second order, so every
    # orientation is within its norm and R_v R_v0^T, which takes two of them, within twice that: 2.3e-7 rad here (|x| = 11.7),
    # not the 1e-9 of the robust stage's check.  Measured: 1.0e-8 rad.
    ptol = nl.DEFAULTS["parameter_tolerance"]
    bound = 2.0 * ptol * (np.linalg.norm(out["orientations"]) + ptol)
    print("noiseless graph, defaults: gap %.3g rad, bound %.3g rad" % (gap, bound))
    assert gap <= bound and bound < 2.5e-7
    # the 1e-9 of tests/test_rotation_averaging.py holds once that last step is applied: the parameter tolerance off, nothing else
    out = nl.rotation_averaging_nonlinear(p, q, options={"parameter_tolerance": 0.0})
    assert out["accepted"][-1] == 1
    assert ra.angle_between(nl.relative_to_first(out["orientations"]), _expected_orientations(absq, np.arange(n))).max() < 1e-9


def test_scipy_finds_no_lower_cost_from_the_end_point():
    s = SCENES["corrupted40"]()
    out = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    cost = out["report"]["final_cost"]
    best = nl.scipy_optimum(s["pairs"], s["qvecs"], out["orientations"])
    assert cost - best <= 1e-4 * cost, (cost, best)
    assert out["report"]["termination"] == nl.CONVERGENCE and cost < 0.1 * out["report"]["initial_cost"]


def test_corrupted_edges_are_filtered_and_clean_ones_kept():
    s = SCENES["corrupted40"]()
    out = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    assert s["bad"].sum() == 6
    assert (out["edge_state"][s["bad"]] == 2).all() and (out["edge_state"][~s["bad"]] == 3).all()
    assert out["report"]["num_filtered_edges"] == 6


def test_max_num_iterations_zero_returns_the_start():
    s = SCENES["triangle"]()
    out = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], options={"max_num_iterations": 0})
    assert out["report"]["termination"] == nl.NO_CONVERGENCE and out["report"]["num_iterations"] == 0
    assert np.array_equal(out["orientations"], np.zeros((3, 3)))


def test_default_nonlinear_rotation_options_equal_reference_defaults():
    # nonlinear_rotation_estimator.h:86 (robust_loss_width 0.1), .cpp:123-125 (max_num_iterations = 200), and ceres::Solver::Options:
    #   function_tolerance 1e-6, gradient_tolerance 1e-10, parameter_tolerance 1e-8, initial_trust_region_radius 1e4,
    #   max_trust_region_radius 1e16, min_relative_decrease 1e-3, min_lm_diagonal 1e-6, max_lm_diagonal 1e32,
    #   max_num_consecutive_invalid_steps 5; min_trust_region_radius 1e-32 is a constant of the kernels
    from dagsfm_amd import capi
    o = capi.default_nonlinear_rotation_options()
    assert (o.robust_loss_width, o.max_num_iterations, o.max_num_consecutive_invalid_steps) == (0.1, 200, 5)
    assert (o.function_tolerance, o.gradient_tolerance, o.parameter_tolerance) == (1e-6, 1e-10, 1e-8)
    assert (o.initial_trust_region_radius, o.max_trust_region_radius, o.min_relative_decrease) == (1e4, 1e16, 1e-3)
    assert (o.min_lm_diagonal, o.max_lm_diagonal) == (1e-6, 1e32)
    assert (o.max_num_cg_iterations, o.cg_tolerance, o.cg_max_residual) == (0, 1e-14, 1e-9)
    assert o.max_relative_rotation_difference_degrees == 5.0
    for key, v in nl.DEFAULTS.items():
        assert getattr(o, key) == v, key


CALL_SITE = r"""
// GlobalRotationAveraging() with global_rotation_estimator_type = NONLINEAR in the style of DistributedMapperController
// (distributed_mapper_controller.cpp:945-1008), optionally polishing the ROBUST_L1L2 result
#include <cstdint>
#include <map>
#include <utility>
#include <vector>
#include "include/dagsfm_mi355x.h"

struct Vec3 { double x, y, z; };

bool NonlinearRotationAveragingOnDevice(dsm_ctx* ctx, const std::vector<std::pair<uint32_t, uint32_t> >& image_pairs,
                                        const std::vector<double>& qvecs, const std::vector<uint8_t>& keep, bool robust_first,
                                        std::map<uint32_t, Vec3>* rotations, std::vector<std::pair<uint32_t, uint32_t> >* dropped) {
  const uint32_t n = static_cast<uint32_t>(image_pairs.size());
  std::vector<uint32_t> pairs(2 * n), ids(2 * n), ids0(2 * n);
  for (uint32_t k = 0; k < n; ++k) {
    pairs[2 * k] = image_pairs[k].first;
    pairs[2 * k + 1] = image_pairs[k].second;
  }
  std::vector<double> orientations(6 * n), orientations0(6 * n), relative(3 * n);
  std::vector<uint8_t> in_final(2 * n), state(n);
  uint32_t n_images = 0, n_initial = 0;
  const uint8_t* use = keep.empty() ? NULL : keep.data();
  if (robust_first) {
    if (dsm_view_graph_rotation_averaging(ctx, n, pairs.data(), qvecs.data(), use, NULL, ids0.data(), orientations0.data(),
                                          in_final.data(), &n_initial, state.data(), relative.data(), NULL) != DSM_OK)
      return false;
  }
  dsm_nonlinear_rotation_options options;
  dsm_default_nonlinear_rotation_options(&options);
  dsm_nonlinear_rotation_report report;
  if (dsm_view_graph_rotation_averaging_nonlinear(ctx, n, pairs.data(), qvecs.data(), use, n_initial, ids0.data(),
                                                  orientations0.data(), &options, ids.data(), orientations.data(), in_final.data(),
                                                  &n_images, state.data(), relative.data(), &report, NULL) != DSM_OK)
    return false;
  for (uint32_t i = 0; i < n_images; ++i) {
    if (!in_final[i]) continue;
    Vec3 r = {orientations[3 * i], orientations[3 * i + 1], orientations[3 * i + 2]};
    (*rotations)[ids[i]] = r;
  }
  for (uint32_t k = 0; k < n; ++k)
    if (state[k] == 1 || state[k] == 2) dropped->push_back(image_pairs[k]);
  return report.termination != DSM_BA_FAILURE;
}
"""


def test_call_site_compiles_as_cxx11(tmp_path):
    src = tmp_path / "nlr_call_site.cc"
    src.write_text(CALL_SITE)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-pedantic-errors", "-c", str(src), "-I", ROOT, "-o",
                           str(tmp_path / "nlr_call_site.o")])


@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_gpu_scene_is_clear_by_margins_and_by_the_probe(name):
    s = SCENES[name]()
    assert len(np.unique(s["pairs"])) <= 600
    out = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], s["use"], options=s["options"])
    assert nl.clear_by_margins(out), out["margins"]
    assert nl.stable_under_rounding(s["pairs"], s["qvecs"], s["use"], options=s["options"], out=out)


def test_chained_scene_is_clear_from_the_robust_start_and_needs_fewer_iterations():
    s = SCENES[CHAINED]()
    rob = ra.rotation_averaging(s["pairs"], s["qvecs"])
    cold = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    warm = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], initial=rob)
    assert nl.clear_by_margins(warm), warm["margins"]
    assert nl.stable_under_rounding(s["pairs"], s["qvecs"], initial=rob, out=warm)
    assert warm["report"]["num_iterations"] < cold["report"]["num_iterations"]
    assert warm["report"]["initial_cost"] < cold["report"]["initial_cost"]
