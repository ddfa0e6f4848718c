"""The NONLINEAR global rotation estimator on the device (dsm_view_graph_rotation_averaging_nonlinear) against the
numpy restatement (tests/nonlinear_rotation_ref.py): the per-edge kernel through dsm_debug_pairwise_rotation_error, then whole
runs on the scene list of tests/nonlinear_rotation_scenes.py -- identical decisions, costs per iteration, gauge-free rotations.

The cost is invariant under one rotation of every image and nothing holds that gauge: orientations are compared relative to the
component's smallest image id (R_v R_v0^T) and as edge rotations, never absolutely."""
import ctypes
import functools

import numpy as np
import pytest

from tests import nonlinear_rotation_ref as nl
from tests import rotation_averaging_ref as ra
from tests.nonlinear_rotation_scenes import CHAINED, SCENES
from tests.test_nonlinear_rotation_cpu import branch_triples

pytestmark = pytest.mark.gpu

ANGLE_TOL = 1e-8  # rad, this stage's tolerance (tests/test_rotation_averaging.py): R_v R_v0^T and the updated relative rotations
COST_RTOL = 1e-9  # cost per LM iteration, relative; where the restatement's cost is exactly 0 the device's is too
# The per-edge kernel: the device may differ from the restatement by ROUNDING_FACTOR times the largest difference between the
# restatement in float64 and in numpy.longdouble on the same inputs (the rounding scale of these formulas: another libm and no
# contraction are each within a few ulp per operation), and never by less than ULP_FLOOR ulp of the largest entry.
ROUNDING_FACTOR = 16.0
ULP_FLOOR = 4.0


def _options(capi, s, **more):
    kw = dict(s["options"])
    kw.update(more)
    return capi.default_nonlinear_rotation_options(**kw)


@functools.lru_cache(maxsize=None)
def _expected(name):
    s = SCENES[name]()
    return s, nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], s["use"], options=s["options"])


def _compare(dev, exp):
    rd, re = dev["report"], exp["report"]
    assert (rd.num_components, rd.num_images, rd.num_edges) == (re["num_components"], re["num_images"], re["num_edges"])
    assert rd.termination == re["termination"] and rd.num_iterations == re["num_iterations"]
    assert list(dev["trace"][1:, 4].astype(int)) == exp["accepted"]
    assert (rd.num_successful_steps, rd.num_rejected_steps, rd.num_invalid_steps) == \
        (re["num_successful_steps"], re["num_rejected_steps"], re["num_invalid_steps"])
    assert np.array_equal(dev["edge_state"], exp["edge_state"])
    assert np.array_equal(dev["image_ids"], exp["image_ids"]) and np.array_equal(dev["in_final_cc"], exp["in_final_cc"])
    assert rd.num_filtered_edges == re["num_filtered_edges"] and rd.num_final_images == re["num_final_images"]
    assert rd.max_cg_relative_residual <= 1e-9
    cd, ce = dev["trace"][:, 0], exp["trace"][:, 0]
    cgap = np.abs(cd - ce)
    rel = float((cgap[ce != 0.0] / np.abs(ce[ce != 0.0])).max(initial=0.0))
    gap = ra.angle_between(nl.relative_to_first(dev["orientations"]), nl.relative_to_first(exp["orientations"])).max()
    k = dev["edge_state"] == 3
    rgap = ra.angle_between(dev["relative_rotations"][k], exp["relative_rotations"][k]).max() if k.any() else 0.0
    absolute = ra.angle_between(dev["orientations"], exp["orientations"]).max()
    print("cost gap %.3g (relative), R_v R_v0^T gap %.3g rad, edge gap %.3g rad, absolute (gauge) %.3g rad, "
          "%d LM / %d CG iterations" % (rel, gap, rgap, absolute, rd.num_iterations, rd.total_cg_iterations))
    assert np.all(cgap <= COST_RTOL * np.abs(ce)), (cd, ce)
    assert rd.initial_cost == dev["trace"][0, 0] and rd.final_cost == dev["trace"][-1, 0]
    assert gap < ANGLE_TOL and rgap < ANGLE_TOL, (gap, rgap)


def _same_bytes(a, b):
    for k in ("image_ids", "orientations", "in_final_cc", "edge_state", "relative_rotations", "trace"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---------------------------------------------------------------- the per-edge kernel
def _edge_tolerance(a1, a2, a12):
    r64 = nl.pairwise_rotation_error(a1, a2, a12)
    rld = nl.pairwise_rotation_error(a1, a2, a12, dtype=np.longdouble)
    tol = []
    for x64, xld in zip(r64, rld):
        scale = float(np.abs(x64 - xld).max())
        tol.append(max(ROUNDING_FACTOR * scale, ULP_FLOOR * np.finfo(np.float64).eps * float(np.abs(x64).max())))
    return r64, tol


@pytest.mark.parametrize("which", ["random", "branches"])
def test_per_edge_kernel_equals_restatement(dsm, which):
    if which == "random":
        rng = np.random.default_rng(71)
        a1, a2, a12 = (rng.normal(scale=0.9, size=(4096, 3)) for _ in range(3))
    else:
        a1, a2, a12 = branch_triples()
    (r, J, rho), tol = _edge_tolerance(a1, a2, a12)
    dr, dJ, drho = dsm.debug_pairwise_rotation_error(a1, a2, a12, 0.1)
    gaps = [float(np.abs(d - e).max()) for d, e in ((dr, r), (dJ, J), (drho, rho))]
    print("residual / jacobian / rho gaps", gaps, "tolerances", tol)
    assert np.isfinite(dJ).all()
    for g, t in zip(gaps, tol):
        assert g <= t, (gaps, tol)
    if which == "branches":  # the exact zero: k = 2, J1 = -I, J2 = I, rho' = 1
        assert np.array_equal(dr[-1], np.zeros(3)) and np.array_equal(dJ[-1, 0], -np.eye(3)) and np.array_equal(dJ[-1, 1], np.eye(3))
        assert drho[-1, 0] == 0.0 and drho[-1, 1] == 1.0


# ---------------------------------------------------------------- whole runs
@pytest.mark.parametrize("name", sorted(SCENES))
def test_device_equals_restatement(dsm, name):
    from dagsfm_amd import capi
    s, exp = _expected(name)
    dev = dsm.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], use=s["use"], options=_options(capi, s))
    _compare(dev, exp)


def test_identity_graph_converges_at_iteration_zero(dsm):
    s, _ = _expected("identity")
    dev = dsm.rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    rep = dev["report"]
    assert rep.termination == nl.CONVERGENCE and rep.num_iterations == 0 and rep.initial_cost == 0.0 and rep.final_cost == 0.0
    assert rep.total_cg_iterations == 0 and np.array_equal(dev["orientations"], np.zeros((12, 3)))
    assert (dev["edge_state"] == 3).all() and np.array_equal(dev["relative_rotations"], np.zeros((len(s["pairs"]), 3)))


def test_start_from_the_robust_result_needs_fewer_iterations(dsm):
    s, cold = _expected(CHAINED)
    rob = dsm.rotation_averaging(s["pairs"], s["qvecs"])
    exp = nl.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], initial=rob)
    assert nl.clear_by_margins(exp) and nl.stable_under_rounding(s["pairs"], s["qvecs"], initial=rob, out=exp)
    dev = dsm.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], initial=rob)
    _compare(dev, exp)
    assert dev["report"].num_iterations < cold["report"]["num_iterations"]
    assert dev["report"].initial_cost < cold["report"]["initial_cost"]
    # ids the component does not hold are ignored
    more = {"image_ids": np.concatenate([rob["image_ids"], [4000000000]]).astype(np.uint32),
            "orientations": np.vstack([rob["orientations"], [[9.0, 9.0, 9.0]]])}
    _same_bytes(dev, dsm.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], initial=more))


@pytest.mark.parametrize("name", ["corrupted40", "hub300", "img257_e513", "repeats_and_mask"])
def test_same_bytes_across_repeats_and_shuffles(dsm, name):
    from dagsfm_amd import capi
    s, _ = _expected(name)
    p, q, u = s["pairs"], s["qvecs"], s["use"]
    dev = dsm.rotation_averaging_nonlinear(p, q, use=u, options=_options(capi, s))
    _same_bytes(dev, dsm.rotation_averaging_nonlinear(p, q, use=u, options=_options(capi, s)))
    if len(np.unique(np.sort(p, axis=1), axis=0)) == len(p):
        o = np.random.default_rng(1).permutation(len(p))  # no pair twice: any order
    else:
        # the first used occurrence of an unordered pair wins, so the occurrences of one pair keep their order
        first = {}
        for e, (a, b) in enumerate(np.sort(p, axis=1)):
            first.setdefault((int(a), int(b)), e)
        key = np.array([first[(int(a), int(b))] for a, b in np.sort(p, axis=1)])
        rank = dict(zip(sorted(first.values()), np.random.default_rng(1).permutation(len(first))))
        o = np.lexsort((np.arange(len(p)), np.array([rank[k] for k in key])))
    devp = dsm.rotation_averaging_nonlinear(p[o], q[o], use=None if u is None else u[o], options=_options(capi, s))
    inv = np.argsort(o)
    assert devp["edge_state"][inv].tobytes() == dev["edge_state"].tobytes()
    assert devp["relative_rotations"][inv].tobytes() == dev["relative_rotations"].tobytes()
    assert devp["orientations"].tobytes() == dev["orientations"].tobytes() and devp["trace"].tobytes() == dev["trace"].tobytes()


def test_product_and_check_build_agree():
    from dagsfm_amd import capi
    s, _ = _expected("sparse_ids")
    a = capi.Context(0, check=False).rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    b = capi.Context(0, check=True).rotation_averaging_nonlinear(s["pairs"], s["qvecs"])
    _same_bytes(a, b)
    assert a["report"].total_cg_iterations == b["report"].total_cg_iterations


def test_chained_over_the_stage_output(dsm):
    """synthetic.Scene -> match_pairs -> verify_pairs -> cycle filter -> robust -> nonlinear: the polished orientations agree
    with the scene's camera rotations, relative to the first image, within 1 degree, at a cost no higher than the start's."""
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
    rob = dsm.rotation_averaging(p, q, use=keep)
    out = dsm.rotation_averaging_nonlinear(p, q, use=keep, initial=rob)
    assert out["report"].num_images >= 6 and np.array_equal(out["image_ids"], rob["image_ids"])
    assert out["report"].termination == nl.CONVERGENCE and out["report"].final_cost <= out["report"].initial_cost
    Rw = np.array([scene.pose(int(i))[0] for i in out["image_ids"]])
    truth = ra.rotation_to_angle_axis(np.matmul(Rw, Rw[0].T[None]))
    gap = ra.angle_between(nl.relative_to_first(out["orientations"]), truth)
    assert gap.max() < np.deg2rad(1.0), np.rad2deg(gap)


# ---------------------------------------------------------------- arguments and exits
def test_argument_errors_and_empty(dsm):
    from dagsfm_amd import capi
    s, _ = _expected("triangle")
    p, q = s["pairs"], s["qvecs"]
    ids = np.unique(p).astype(np.uint32)
    zeros = np.zeros((3, 3))
    bad_initials = [{"image_ids": ids[:2], "orientations": zeros[:2]},                       # does not cover the component
                    {"image_ids": ids[::-1].copy(), "orientations": zeros},                  # unsorted
                    {"image_ids": ids[[0, 1, 1]].copy(), "orientations": zeros},             # repeated
                    {"image_ids": ids, "orientations": np.array([[0.0, 0, 0], [0, np.nan, 0], [0, 0, 0]])}]
    for initial in bad_initials:
        with pytest.raises(capi.DsmError):
            dsm.rotation_averaging_nonlinear(p, q, initial=initial)
    for kw in ({"robust_loss_width": 0.0}, {"robust_loss_width": -0.1}, {"max_num_iterations": -1}):
        with pytest.raises(capi.DsmError):
            dsm.rotation_averaging_nonlinear(p, q, options=capi.default_nonlinear_rotation_options(**kw))
    for bad_p, bad_q in [(np.array([(1, 1), (2, 3), (1, 3)], np.uint32), q), (p, np.vstack([q[:2], [[np.nan, 0, 0, 0]]])),
                         (p, np.vstack([q[:2], [[0.0, 0, 0, 0]]]))]:
        with pytest.raises(capi.DsmError):
            dsm.rotation_averaging_nonlinear(bad_p, bad_q)
    L = dsm._L
    assert L.dsm_view_graph_rotation_averaging_nonlinear(None, 0, None, None, None, 0, None, None, None, None, None, None, None, None,
                                                         None, None, None) == 1
    n = ctypes.c_uint32(7)
    assert L.dsm_view_graph_rotation_averaging_nonlinear(dsm._h, 3, p.ctypes.data, None, None, 0, None, None, None, None, None, None,
                                                         ctypes.addressof(n), None, None, None, None) == 1
    out = dsm.rotation_averaging_nonlinear(p, q, use=[0, 0, 0])
    assert len(out["image_ids"]) == 0 and (out["edge_state"] == 0).all() and len(out["trace"]) == 0
    out = dsm.rotation_averaging_nonlinear(np.zeros((0, 2), np.uint32), np.zeros((0, 4)))
    assert len(out["image_ids"]) == 0
    with pytest.raises(capi.DsmError):
        dsm.debug_pairwise_rotation_error(zeros, zeros, zeros, loss_width=0.0)


def test_max_num_iterations_zero_returns_the_start(dsm):
    from dagsfm_amd import capi
    s, _ = _expected(CHAINED)
    rob = dsm.rotation_averaging(s["pairs"], s["qvecs"])
    out = dsm.rotation_averaging_nonlinear(s["pairs"], s["qvecs"], initial=rob,
                                           options=capi.default_nonlinear_rotation_options(max_num_iterations=0))
    rep = out["report"]
    assert rep.termination == nl.NO_CONVERGENCE and rep.num_iterations == 0 and rep.total_cg_iterations == 0
    assert out["orientations"].tobytes() == rob["orientations"].tobytes() and rep.initial_cost == rep.final_cost
    assert len(out["trace"]) == 1


def test_cg_cap_fails_the_call_and_leaves_the_context_usable():
    from dagsfm_amd import capi
    from tests.test_rotation_averaging import _edges_random, _graph
    p, q, _, _ = _graph(81, 200, _edges_random(np.random.default_rng(81), 200, 6), noise=0.004)
    ctx = capi.Context(0)
    with pytest.raises(capi.DsmError) as err:
        ctx.rotation_averaging_nonlinear(p, q, options=capi.default_nonlinear_rotation_options(max_num_cg_iterations=1))
    assert "conjugate-gradient" in str(err.value)
    after = ctx.rotation_averaging_nonlinear(p, q)
    fresh = capi.Context(0).rotation_averaging_nonlinear(p, q)
    _same_bytes(after, fresh)
    assert after["report"].termination == nl.CONVERGENCE
