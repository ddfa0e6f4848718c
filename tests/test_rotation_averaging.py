"""Global rotation averaging of the filtered view graph (dsm_view_graph_rotation_averaging; DistributedMapperController::
GlobalRotationAveraging, src/controllers/distributed_mapper_controller.cpp:945-1008).

CPU: the numpy restatement (tests/rotation_averaging_ref.py) on graphs whose answer is known by construction, ceres' conversions
on known answers, the option defaults, a call site in the reference's C++ dialect.  GPU: device == restatement by tolerance
(CHOLMOD there, a conjugate gradient here) with identical iteration counts and decisions, byte-identical repeats,
the stage's own output chained through the cycle filter into this call, the argument errors."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import rotation_averaging_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANGLE_TOL = 1e-8  # rad, device vs restatement (orientations and updated relative rotations)


def _rand_q(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _qmul(a, b):
    w1, x1, y1, z1 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    w2, x2, y2, z2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                     w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], axis=1)


def _conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _edges_random(rng, n_img, deg):
    s = set()
    for i in range(n_img):
        for j in rng.choice(n_img, min(deg, n_img - 1), replace=False):
            if i != int(j):
                s.add((min(i, int(j)), max(i, int(j))))
    return np.array(sorted(s), np.int64)


def _edges_sequence(n_img, half):
    return np.array([(i, j) for i in range(n_img) for j in range(i + 1, min(n_img, i + half + 1))], np.int64)


def _qvecs(rng, absq, pairs, noise=0.0, corrupt=()):
    """q_12 = q_2 * conj(q_1): the rotation from image 1 to image 2 of absolute (world -> camera) rotations."""
    q = _qmul(absq[pairs[:, 1]], _conj(absq[pairs[:, 0]]))
    if noise:
        q = q + rng.normal(scale=noise, size=q.shape)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
    for e in corrupt:
        q[e] = _rand_q(rng, 1)[0]
    return q


def _graph(seed, n_img, pairs, noise=0.0, n_corrupt=0, ids=None, shuffle=True):
    rng = np.random.default_rng(seed)
    absq = _rand_q(rng, n_img)
    corrupt = rng.choice(len(pairs), n_corrupt, replace=False) if n_corrupt else []
    q = _qvecs(rng, absq, pairs, noise, corrupt)
    bad = np.zeros(len(pairs), bool)
    bad[list(corrupt)] = True
    if ids is not None:
        pairs = ids[pairs]
    if shuffle:
        o = rng.permutation(len(pairs))
        pairs, q, bad = pairs[o], q[o], bad[o]
    return pairs.astype(np.uint32), q, bad, absq


def _expected_orientations(absq, img):
    """R_v = abs_v * abs_0^-1 (the smallest id held constant) as angle-axis."""
    rq = _qmul(absq[img], _conj(absq[img[:1]].repeat(len(img), 0)))
    return ref.quaternion_to_angle_axis(rq)


# ---------------------------------------------------------------- CPU
def test_restatement_noiseless_graph_returns_generating_rotations():
    n = 30
    pairs = _edges_random(np.random.default_rng(1), n, 6)
    p, q, _, absq = _graph(2, n, pairs, shuffle=False)
    out = ref.rotation_averaging(p, q)
    assert out["report"]["num_images"] == n and (out["edge_state"] == 3).all() and out["in_final_cc"].all()
    assert ref.angle_between(out["orientations"], _expected_orientations(absq, np.arange(n))).max() < 1e-9


def test_restatement_filters_corrupted_edges():
    n = 40
    pairs = _edges_random(np.random.default_rng(4), n, 8)
    p, q, bad, _ = _graph(5, n, pairs, noise=0.002, n_corrupt=12)
    out = ref.rotation_averaging(p, q)
    assert (out["edge_state"][bad] == 2).all() and (out["edge_state"][~bad] == 3).all()
    assert out["report"]["num_filtered_edges"] == 12


def test_ceres_conversions_known_answers():
    # 0, tiny angles, pi/2, near pi
    assert np.array_equal(ref.quaternion_to_angle_axis([1.0, 0, 0, 0]), np.zeros((1, 3)))
    assert np.array_equal(ref.angle_axis_to_rotation([0.0, 0, 0])[0], np.eye(3))
    tiny = np.array([1e-9, -2e-9, 3e-9])
    assert np.allclose(ref.angle_axis_to_rotation(tiny)[0], np.eye(3) + np.array([[0, -3e-9, -2e-9], [3e-9, 0, -1e-9], [2e-9, 1e-9, 0]]),
                       rtol=0, atol=1e-20)
    assert np.allclose(ref.rotation_to_angle_axis(ref.angle_axis_to_rotation(tiny)), tiny, rtol=1e-6, atol=0)
    half = np.pi / 2
    Rz = ref.angle_axis_to_rotation([0, 0, half])[0]
    assert np.allclose(Rz, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-15)
    assert np.allclose(ref.quaternion_to_angle_axis([np.cos(half / 2), 0, 0, np.sin(half / 2)]), [[0, 0, half]], atol=1e-15)
    near = np.pi - 1e-7
    aa = np.array([near, 0.0, 0.0])
    back = ref.rotation_to_angle_axis(ref.angle_axis_to_rotation(aa))[0]  # trace < 0: the largest-diagonal branch
    assert abs(np.linalg.norm(back) - near) < 1e-8 and ref.angle_between(back[None], aa[None])[0] < 1e-8
    # a quaternion with w < 0 gives the short way round
    assert np.allclose(ref.quaternion_to_angle_axis([-np.cos(0.1), np.sin(0.1), 0, 0]), [[-0.2, 0, 0]], atol=1e-15)


def test_default_rotation_averaging_options_equal_reference_defaults():
    # robust_rotation_estimator.h:96-115, l1_solver.h Options, SolveL1Regression's options.max_num_iterations = 5
    from dagsfm_amd import capi
    o = capi.default_rotation_averaging_options()
    assert (o.max_num_l1_iterations, o.max_num_irls_iterations, o.admm_initial_max_iterations) == (5, 100, 5)
    assert (o.l1_step_convergence_threshold, o.irls_step_convergence_threshold) == (0.001, 0.001)
    assert o.irls_loss_parameter_sigma == 5.0 * (np.pi / 180.0)
    assert (o.admm_rho, o.admm_alpha, o.admm_absolute_tolerance, o.admm_relative_tolerance) == (1.0, 1.0, 1e-4, 1e-2)
    assert o.max_relative_rotation_difference_degrees == 5.0
    assert (o.cg_tolerance, o.cg_max_residual) == (1e-12, 1e-9)


CALL_SITE = r"""
// GlobalRotationAveraging() in the style of DistributedMapperController (distributed_mapper_controller.cpp:945-1008)
#include <cstdint>
#include <map>
#include <utility>
#include <vector>
#include "include/dagsfm_mi355x.h"

struct Vec3 { double x, y, z; };

bool GlobalRotationAveragingOnDevice(dsm_ctx* ctx, const std::vector<std::pair<uint32_t, uint32_t> >& image_pairs,
                                     const std::vector<double>& qvecs, const std::vector<uint8_t>& keep,
                                     std::map<uint32_t, Vec3>* rotations, std::vector<std::pair<uint32_t, uint32_t> >* dropped) {
  const uint32_t n = static_cast<uint32_t>(image_pairs.size());
  std::vector<uint32_t> pairs(2 * n), ids(2 * n);
  for (uint32_t k = 0; k < n; ++k) {
    pairs[2 * k] = image_pairs[k].first;
    pairs[2 * k + 1] = image_pairs[k].second;
  }
  std::vector<double> orientations(6 * n), relative(3 * n);
  std::vector<uint8_t> in_final(2 * n), state(n);
  uint32_t n_images = 0;
  dsm_rotation_averaging_options options;
  dsm_default_rotation_averaging_options(&options);
  dsm_rotation_averaging_report report;
  if (dsm_view_graph_rotation_averaging(ctx, n, pairs.data(), qvecs.data(), keep.empty() ? NULL : keep.data(), &options, ids.data(),
                                        orientations.data(), in_final.data(), &n_images, state.data(), relative.data(),
                                        &report) != DSM_OK)
    return false;
  for (uint32_t i = 0; i < n_images; ++i) {
    if (!in_final[i]) continue;
    Vec3 r = {orientations[3 * i], orientations[3 * i + 1], orientations[3 * i + 2]};
    (*rotations)[ids[i]] = r;
  }
  for (uint32_t k = 0; k < n; ++k)
    if (state[k] == 1 || state[k] == 2) dropped->push_back(image_pairs[k]);  // the host deletes their DB rows
  return true;
}
"""


def test_call_site_compiles_as_cxx11(tmp_path):
    src = tmp_path / "ra_call_site.cc"
    src.write_text(CALL_SITE)
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-pedantic-errors", "-c", str(src), "-I", ROOT, "-o",
                           str(tmp_path / "ra_call_site.o")])


# ---------------------------------------------------------------- GPU
def _compare(dev, exp, tol=ANGLE_TOL):
    rd, re = dev["report"], exp["report"]
    assert rd.num_components == re["num_components"] and rd.num_images == re["num_images"] and rd.num_edges == re["num_edges"]
    assert rd.num_l1_iterations == re["num_l1_iterations"]
    assert list(rd.admm_iterations)[:rd.num_l1_iterations] == re["admm_iterations"]
    assert rd.num_irls_iterations == re["num_irls_iterations"]
    assert np.array_equal(dev["edge_state"], exp["edge_state"])
    assert np.array_equal(dev["image_ids"], exp["image_ids"]) and np.array_equal(dev["in_final_cc"], exp["in_final_cc"])
    assert rd.num_filtered_edges == re["num_filtered_edges"] and rd.num_final_images == re["num_final_images"]
    assert rd.max_cg_relative_residual <= 1e-9
    gap = ref.angle_between(dev["orientations"], exp["orientations"]).max() if len(exp["orientations"]) else 0.0
    k = dev["edge_state"] == 3
    rgap = ref.angle_between(dev["relative_rotations"][k], exp["relative_rotations"][k]).max() if k.any() else 0.0
    assert gap < tol and rgap < tol, (gap, rgap)
    return gap, rgap


def _same_bytes(a, b):
    for k in ("image_ids", "orientations", "in_final_cc", "edge_state", "relative_rotations"):
        assert a[k].tobytes() == b[k].tobytes(), k


CASES = {
    "triangle": lambda: _graph(11, 3, np.array([(0, 1), (0, 2), (1, 2)]), noise=0.01),
    "five": lambda: _graph(12, 5, _edges_random(np.random.default_rng(12), 5, 4), noise=0.005),
    "40x8_corrupt": lambda: _graph(13, 40, _edges_random(np.random.default_rng(13), 40, 8), noise=0.002, n_corrupt=10),
    "300x30_noise": lambda: _graph(14, 300, _edges_random(np.random.default_rng(14), 300, 30), noise=0.01, n_corrupt=40),
    "1000x12": lambda: _graph(15, 1000, _edges_random(np.random.default_rng(15), 1000, 12), noise=0.003, n_corrupt=30),
    "sequence400": lambda: _graph(16, 400, _edges_sequence(400, 4), noise=0.002, n_corrupt=8),
    "arbitrary_ids": lambda: _graph(17, 60, _edges_random(np.random.default_rng(17), 60, 6), noise=0.004, n_corrupt=5,
                                    ids=np.random.default_rng(18).permutation(100000)[:60].astype(np.int64) + 7),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(CASES))
def test_device_equals_restatement(dsm, case):
    p, q, _, _ = CASES[case]()
    exp = ref.rotation_averaging(p, q)
    assert ref.min_margin(exp["decisions"]) > 1e-6, "fixture on a knife edge"
    dev = dsm.rotation_averaging(p, q)
    _compare(dev, exp)
    # a second call, a permuted list (reversed pairs carry the conjugate rotation), the check build: the same bytes
    _same_bytes(dev, dsm.rotation_averaging(p, q))
    o = np.random.default_rng(1).permutation(len(p))
    devp = dsm.rotation_averaging(p[o], q[o])
    inv = np.argsort(o)
    assert devp["edge_state"][inv].tobytes() == dev["edge_state"].tobytes()
    assert devp["relative_rotations"][inv].tobytes() == dev["relative_rotations"].tobytes()
    assert devp["orientations"].tobytes() == dev["orientations"].tobytes()


@pytest.mark.gpu
def test_product_and_check_build_agree_and_batch_size_is_invisible():
    from dagsfm_amd import capi
    p, q, _, _ = CASES["300x30_noise"]()
    a = capi.Context(0, check=False).rotation_averaging(p, q)
    b = capi.Context(0, check=True).rotation_averaging(p, q)
    _same_bytes(a, b)
    c = capi.Context(0, check=False).rotation_averaging(p, q, options=capi.default_rotation_averaging_options(cg_batch_iterations=1))
    _same_bytes(a, c)
    assert a["report"].total_cg_iterations == c["report"].total_cg_iterations


@pytest.mark.gpu
def test_two_equal_components_tie_rule(dsm):
    # two 6-image cliques with disjoint ids: the one holding the smallest id wins (a free choice)
    c = np.array([(i, j) for i in range(6) for j in range(i + 1, 6)])
    pairs = np.vstack([c + 100, c + 10])
    p, q, _, _ = _graph(21, 200, pairs, noise=0.003)
    exp = ref.rotation_averaging(p, q)
    dev = dsm.rotation_averaging(p, q)
    _compare(dev, exp)
    assert dev["report"].num_components == 2 and list(dev["image_ids"]) == list(range(10, 16))
    st = dev["edge_state"]
    assert (st[p.min(axis=1) >= 100] == 1).all() and (st[p.max(axis=1) < 100] == 3).all()


@pytest.mark.gpu
def test_filter_splits_the_graph(dsm):
    # a sparse noisy graph under a 0.3 degree orientation filter: most edges go, the final component is a part of the first
    from dagsfm_amd import capi
    pairs = _edges_random(np.random.default_rng(25), 30, 3)
    rng = np.random.default_rng(25)
    q = _qvecs(rng, _rand_q(rng, 30), pairs, 0.004)
    p = pairs.astype(np.uint32)
    exp = ref.rotation_averaging(p, q, filter_degrees=0.3)
    assert ref.min_margin(exp["decisions"]) > 1e-6
    dev = dsm.rotation_averaging(p, q, options=capi.default_rotation_averaging_options(max_relative_rotation_difference_degrees=0.3))
    _compare(dev, exp)
    assert dev["report"].num_images == 30 and 1 < dev["report"].num_final_images < 30 and (dev["edge_state"] == 2).sum() > 0


@pytest.mark.gpu
def test_use_mask_from_cycle_filter(dsm):
    p, q, _, _ = CASES["40x8_corrupt"]()
    keep, _ = dsm.view_graph_filter_cycles(p, q, 5.0)
    exp = ref.rotation_averaging(p, q, use=keep)
    assert ref.min_margin(exp["decisions"]) > 1e-6
    dev = dsm.rotation_averaging(p, q, use=keep)
    _compare(dev, exp)
    assert (dev["edge_state"][~keep] == 0).all()


@pytest.mark.gpu
def test_noiseless_graph_and_repeats(dsm):
    n = 50
    pairs = _edges_random(np.random.default_rng(31), n, 6)
    p, q, _, absq = _graph(32, n, pairs)
    # a repeat of an earlier pair in reversed order with a wrong rotation is ignored
    p2 = np.vstack([p, p[:1, ::-1]])
    q2 = np.vstack([q, _rand_q(np.random.default_rng(3), 1)])
    dev = dsm.rotation_averaging(p2, q2)
    assert dev["edge_state"][-1] == 0 and (dev["edge_state"][:-1] == 3).all()
    assert ref.angle_between(dev["orientations"], _expected_orientations(absq, np.arange(n))).max() < 1e-9


@pytest.mark.gpu
def test_chained_over_the_stage_output(dsm):
    """synthetic.Scene -> match_pairs -> verify_pairs -> cycle filter -> rotation averaging: the orientations agree with the
    scene's camera rotations up to the gauge (image 0 held constant) within 1 degree."""
    from dagsfm_amd import capi, synthetic
    n_img = 9
    scene = synthetic.Scene(n_img, 640, seed=4, n_pool=1800)
    ims = [scene.image(i) for i in range(n_img)]
    cams = [capi.simple_pinhole(800.0, 500.0, 375.0, 1000, 750, True) for _ in range(n_img)]
    dsm.set_images([im[0] for im in ims], [im[1] for im in ims], cams)
    pairs = synthetic.exhaustive_pairs(n_img)
    dsm.match_pairs(pairs)
    dsm.verify_pairs(capi.default_two_view_options(), user_seed=2, stage_filter=True)
    tv = dsm.two_view_geometries()
    sel = [k for k in range(len(pairs)) if tv[k].config in (2, 3, 4, 5, 6)]
    p = np.asarray(pairs)[sel]
    q = np.array([list(tv[k].qvec) for k in sel])
    keep, _ = dsm.view_graph_filter_cycles(p, q, 5.0)
    out = dsm.rotation_averaging(p, q, use=keep)
    assert out["report"].num_images >= 6
    ids = out["image_ids"]
    Rw = np.array([scene.pose(int(i))[0] for i in ids])
    truth = ref.rotation_to_angle_axis(np.matmul(Rw, Rw[0].T[None]))
    gap = ref.angle_between(out["orientations"], truth)
    assert gap.max() < np.deg2rad(1.0), np.rad2deg(gap)


@pytest.mark.gpu
def test_argument_errors_and_empty(dsm):
    from dagsfm_amd import capi
    p = np.array([(1, 2), (2, 3), (1, 3)], np.uint32)
    q = np.tile([1.0, 0, 0, 0], (3, 1))
    for bad_p, bad_q in [(np.array([(1, 1), (2, 3), (1, 3)], np.uint32), q), (p, np.vstack([q[:2], [[np.nan, 0, 0, 0]]])),
                         (p, np.vstack([q[:2], [[0.0, 0, 0, 0]]]))]:
        with pytest.raises(capi.DsmError):
            dsm.rotation_averaging(bad_p, bad_q)
    # a bad edge that is not used is not looked at
    out = dsm.rotation_averaging(np.array([(1, 1), (2, 3)], np.uint32), np.array([[0.0, 0, 0, 0], [1.0, 0, 0, 0]]), use=[0, 1])
    assert out["report"].num_images == 2
    with pytest.raises(capi.DsmError):
        dsm.rotation_averaging(p, q, options=capi.default_rotation_averaging_options(max_num_l1_iterations=capi.RA_MAX_L1_ITERATIONS + 1))
    L = dsm._L
    assert L.dsm_view_graph_rotation_averaging(None, 0, None, None, None, None, None, None, None, None, None, None, None) == 1
    n = ctypes.c_uint32(7)
    assert L.dsm_view_graph_rotation_averaging(dsm._h, 3, p.ctypes.data, None, None, None, None, None, None, ctypes.addressof(n), None,
                                               None, None) == 1
    out = dsm.rotation_averaging(p, q, use=[0, 0, 0])
    assert len(out["image_ids"]) == 0 and (out["edge_state"] == 0).all()
    out = dsm.rotation_averaging(np.zeros((0, 2), np.uint32), np.zeros((0, 4)))
    assert len(out["image_ids"]) == 0
