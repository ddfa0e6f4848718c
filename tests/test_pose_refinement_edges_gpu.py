"""GPU: dsm_refine_absolute_poses at the edges its first module does not reach (DESIGN.md 15 "Edges"): rejected steps and the
dec update from far starts, loss_function_scale != 1, refine_flags 2 alone, point counts and masks at the wave's edges, the two
FAILURE exits with their neighbours and register_images' answer to them, zero and unnormalised quaternions, a batch above 256
problems, the size refusal and the iteration cap's limit.  The comparison rule is tests/test_pose_refinement_gpu.py's compare,
unchanged; the problems are tests/pose_refinement_scenes.py's edge_* builders, whose constructions and one-ulp sensitivity
tests/test_pose_refinement_edges_cpu.py holds on the restatement."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import pose_refinement_ref as ref
from tests import pose_refinement_scenes as sc
from tests.bundle_adjustment_ref import TWO_FOCAL
from tests.test_pose_refinement_gpu import close, compare, result_bytes, run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def wave(ctx):
    """The sixteen wave-edge problems and their one batch on the device, shared and left unchanged."""
    problems = sc.edge_wave_problems()
    return problems, run(ctx, problems)


def bits(res):
    return (np.array(list(res.qvec)).tobytes(), np.array(list(res.tvec)).tobytes(), list(res.camera_params))


def input_bits(p):
    return (np.asarray(p["qvec"], np.float64).tobytes(), np.asarray(p["tvec"], np.float64).tobytes(), list(p["cam"].params))


def test_far_starts_reject_steps_and_reset_dec(ctx):
    """The two rows that are not clear in the restatement are held to the other rule: success and the final cost within
    HAND_COST_TOLERANCE of the initial cost (2.7e-18 and 0 observed)."""
    rows = sc.edge_far_starts()
    out = run(ctx, [p for p, _ in rows])
    clear = 0
    for b, (p, listed) in enumerate(rows):
        want = ref.refine(*sc.args(p))
        c = compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, b)
        if listed:
            clear += c
            assert capi.POSE_STEP_REJECTED in list(out["steps"][b]), b
        else:
            assert not c, b
    assert clear >= 0.9 * sum(listed for _, listed in rows)
    last = out["results"][len(rows) - 1]
    assert last.termination == capi.BA_NO_CONVERGENCE and last.num_iterations == 100 and last.success == 1
    assert len(out["steps"][len(rows) - 1]) == 100 and 0 not in list(out["steps"][len(rows) - 1])


def test_loss_function_scale(ctx):
    p = sc.edge_loss_scale_problem()
    costs = [run(ctx, [p])["results"][0].initial_cost]
    for s in sc.LOSS_SCALES:
        out = run(ctx, [p], capi.default_pose_refinement_options(loss_function_scale=s))
        want = ref.refine(*sc.args(p), opts=dict(loss_function_scale=s))
        assert compare(out["results"][0], out["steps"][0], out["margins"][0], p, want, "scale %g" % s, dict(loss_function_scale=s))
        costs.append(out["results"][0].initial_cost)
    for i in range(4):
        for j in range(i):
            assert abs(costs[i] - costs[j]) > 0.1 * max(costs[i], costs[j]), costs


def test_refine_flags_2_alone(ctx):
    two = sc.edge_flags2()
    models = sorted(two)
    out = run(ctx, [two[m] for m in models])
    zero = sc.edge_flags2(flags=0)
    out0 = run(ctx, [zero[m] for m in (0, 1)])
    for b, m in enumerate(models):
        p, res = two[m], out["results"][b]
        want = ref.refine(*sc.args(p))
        assert compare(res, out["steps"][b], out["margins"][b], p, want, "flags 2 model %d" % m)
        nfoc = 2 if m in TWO_FOCAL else 1
        assert list(res.camera_params)[:nfoc + 2] == list(p["cam"].params)[:nfoc + 2], m  # focal length(s), principal point: the input bits
        if m in (0, 1):  # nothing to free: the problem of flags 0
            assert list(res.camera_params) == list(p["cam"].params), m
            assert result_bytes(out, b) == result_bytes(out0, b), m
        else:
            assert any(res.camera_params[j] != p["cam"].params[j] for j in range(nfoc + 2, capi.CAMERA_MODEL_NUM_PARAMS[m])), m


def test_wave_edge_sizes_in_one_batch(wave):
    problems, out = wave
    assert len(problems) == 16
    for b, p in enumerate(problems):
        n = len(p["xy"])
        want = ref.refine(*sc.args(p))
        c = compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, "N = %d, %d" % (n, b), exact_data=n < 3)
        assert c or n < 3, b
        assert out["results"][b].num_residual_blocks == n
    assert out["report"].num_points == sum(len(p["xy"]) for p in problems)


def test_masks_that_empty_lanes_and_passes(ctx, wave):
    masked = sc.edge_masks()
    out = run(ctx, masked)
    for b, (name, p) in enumerate(zip(sc.MASK_NAMES, masked)):
        want = ref.refine(*sc.args(p))
        # three points and one point are fitted exactly: the final cost goes against the initial cost, as the hand problems'
        compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, name, exact_data=want["num_residual_blocks"] <= 3)
        assert out["results"][b].num_residual_blocks == sc.MASK_RESIDUAL_BLOCKS[b]
    # any non-zero byte is an inlier: the same bytes as the mask of ones
    problems, base = wave
    mixed = np.ones(129, np.uint8)
    mixed[::2], mixed[1::3] = 2, 255
    for fill in (np.full(129, 2, np.uint8), np.full(129, 255, np.uint8), mixed):
        for b in (7, 15):  # N = 129: pose only, and SIMPLE_RADIAL free
            got = run(ctx, [dict(problems[b], mask=fill)])
            assert result_bytes(got, 0) == result_bytes(base, b), (b, int(fill[0]))


def test_failures_and_their_neighbours(ctx):
    ordinary = [sc.edge_wave_problems()[4], sc.edge_loss_scale_problem()]
    nonfinite, invalid0, invalid1 = sc.edge_nonfinite_cost(), sc.edge_invalid_steps(1e155, 0), sc.edge_invalid_steps(1e155, 1)
    problems = [ordinary[0], nonfinite, invalid0, invalid1, ordinary[1]]
    out = run(ctx, problems)
    # the non-finite initial cost: FAILURE before the first iteration
    res, want = out["results"][1], ref.refine(*sc.args(nonfinite))
    print("non-finite", res.termination, res.num_iterations, res.initial_cost, res.final_cost, "ref", want["termination"], want["initial_cost"])
    assert want["termination"] == ref.FAILURE and not want["success"]
    assert (res.termination, res.success, res.num_iterations, len(out["steps"][1])) == (capi.BA_FAILURE, 0, 0, 0)
    assert (res.num_successful_steps, res.num_invalid_steps, res.num_residual_blocks) == (0, 0, 64)
    assert res.initial_cost == np.inf and res.final_cost == np.inf
    close(list(res.qvec), want["qvec"], "qvec non-finite")
    assert abs(np.linalg.norm(list(res.qvec)) - 1.0) < 1e-15
    assert bits(res)[1:] == input_bits(nonfinite)[1:]
    # five invalid steps in a row
    for b, p in ((2, invalid0), (3, invalid1)):
        with np.errstate(over="ignore"):  # (the restatement's J'J overflows, as the device's)
            res, want = out["results"][b], ref.refine(*sc.args(p))
        print("invalid flags", p["flags"], "device", res.termination, list(out["steps"][b]), repr(res.initial_cost), "ref", want["termination"],
              want["steps"], repr(want["initial_cost"]))
        assert want["steps"] == [ref.INVALID] * 5 and want["termination"] == ref.FAILURE
        assert (res.termination, res.success) == (capi.BA_FAILURE, 0)
        assert (res.num_iterations, res.num_successful_steps, res.num_invalid_steps, res.num_residual_blocks) == (5, 0, 5, 70)
        assert list(out["steps"][b]) == [capi.POSE_STEP_INVALID] * 5
        assert res.final_cost == res.initial_cost
        close([res.initial_cost], [want["initial_cost"]], "initial cost invalid %d" % b)
        assert bits(res) == input_bits(p), b
    # the control, below the overflow: one iteration, usable
    control = [sc.edge_invalid_steps(1e150, f) for f in (0, 1)]
    outc = run(ctx, control)
    for b, p in enumerate(control):
        want = ref.refine(*sc.args(p))
        compare(outc["results"][b], outc["steps"][b], outc["margins"][b], p, want, "control %d" % b)
        assert outc["results"][b].success == 1 and list(outc["steps"][b]) == [capi.POSE_STEP_TOLERANCE]
    # the neighbours are what they are alone, and the report counts everybody's iterations
    for b, p in ((0, ordinary[0]), (4, ordinary[1])):
        alone = run(ctx, [p])
        assert result_bytes(alone, 0) == result_bytes(out, b), b
        assert out["results"][b].success == 1 and out["results"][b].num_iterations >= 2
    assert out["report"].num_iterations == sum(r.num_iterations for r in out["results"])


def test_failure_after_accepted_steps_keeps_the_last_accepted_state(ctx):
    """Not clear by the rule (the pivot margin of an invalid step is 0), so compare() does not apply; the CPU test holds that one
    ulp on the inputs flips none of its decisions and moves its result within the grid's constant, so everything is compared."""
    p, o = sc.edge_accepted_then_invalid()
    out = run(ctx, [p], capi.default_pose_refinement_options(**o))
    with np.errstate(all="ignore"):
        want = ref.refine(*sc.args(p), opts=o)
    res, steps = out["results"][0], list(out["steps"][0])
    print("device", res.termination, steps, "%.6g -> %.6g" % (res.initial_cost, res.final_cost),
          "ref", want["termination"], want["steps"], "%.6g -> %.6g" % (want["initial_cost"], want["final_cost"]))
    assert steps == want["steps"] and steps[-5:] == [capi.POSE_STEP_INVALID] * 5 and capi.POSE_STEP_REJECTED in steps
    assert (res.termination, res.success) == (capi.BA_FAILURE, 0) and want["termination"] == ref.FAILURE
    assert (res.num_iterations, res.num_successful_steps, res.num_invalid_steps) == (14, 7, 5)
    assert (want["num_iterations"], want["num_successful_steps"], want["num_invalid_steps"]) == (14, 7, 5)
    close([res.initial_cost], [want["initial_cost"]], "initial cost")
    close([res.final_cost], [want["final_cost"]], "final cost")
    close(list(res.qvec), want["qvec"], "qvec")
    close(list(res.tvec), want["tvec"], "tvec")
    assert list(res.camera_params) == list(p["cam"].params)


def test_register_images_reports_a_failed_refinement_as_not_registered(ctx):
    """incremental_mapper.cc:498-503.  The smallest construction that reaches FAILURE through the estimator: the estimate is
    ordinary, and the refinement's loss scale makes its initial cost infinite (FAILING_LOSS_SCALE)."""
    cams, offs, xy, X = sc.edge_registrations()
    kw = dict(estimate_focal_length=[0] * 3, refine_flags=[0, 3, 1])
    good = ctx.register_images(cams, offs, xy, X, **kw)
    assert list(good["registered"]) == [True] * 3 and all(r.success for r in good["refinement"]["results"])
    bad = ctx.register_images(cams, offs, xy, X, refinement_options=capi.default_pose_refinement_options(
        loss_function_scale=sc.FAILING_LOSS_SCALE), **kw)
    assert list(bad["registered"]) == [False] * 3 and list(bad["refined_index"]) == [0, 1, 2]
    for b in range(3):
        e, r = bad["estimate"]["results"][b], bad["refinement"]["results"][b]
        assert e.success and e.num_inliers >= 30  # the estimator registered it: the refinement alone says no
        assert (r.success, r.termination, r.num_iterations) == (0, capi.BA_FAILURE, 0) and r.initial_cost == np.inf
        sl = slice(int(offs[b]), int(offs[b + 1]))
        want = ref.refine(cams[b], xy[sl], X[sl], bad["inlier_mask"][sl], list(e.qvec), list(e.tvec), kw["refine_flags"][b],
                          opts=dict(loss_function_scale=sc.FAILING_LOSS_SCALE))
        assert want["termination"] == ref.FAILURE and not want["success"] and want["initial_cost"] == np.inf


def test_zero_and_unnormalised_quaternions(ctx):
    q = sc.edge_quaternion_problem()
    problems = [dict(q, qvec=np.zeros(4)), q, dict(q, qvec=q["qvec"] * 1.7)]
    out = run(ctx, problems)
    wants = [ref.refine(*sc.args(p)) for p in problems]
    for b, (p, want) in enumerate(zip(problems, wants)):
        assert compare(out["results"][b], out["steps"][b], out["margins"][b], p, want, ("zero qvec", "qvec", "qvec x 1.7")[b])
    assert out["results"][0].num_iterations == 11
    # normalisation comes first: the scaled start gives the same bytes where the restatement's normalisation does
    same = wants[1]["qvec"].tobytes() == wants[2]["qvec"].tobytes() and wants[1]["final_cost"] == wants[2]["final_cost"]
    print("restatement: the scaled start gives the same bytes:", same)
    if same:
        assert result_bytes(out, 1) == result_bytes(out, 2)
    assert list(out["steps"][1]) == list(out["steps"][2])


def test_batch_of_300_with_empty_and_masked_problems(ctx, wave):
    problems, base = wave
    big = sc.edge_big_batch()
    out = run(ctx, [p for p, _, _ in big])
    assert len(out["results"]) == 300 and out["report"].num_problems == 300
    for b, (p, k, masked) in enumerate(big):
        res = out["results"][b]
        if k < 0 or masked:  # an empty segment, a segment without an inlier: the input bits
            assert (res.success, res.termination, res.num_iterations, res.num_residual_blocks) == (1, capi.BA_CONVERGENCE, 0, 0), b
            assert bits(res) == input_bits(p) and res.initial_cost == 0.0 and res.final_cost == 0.0 and len(out["steps"][b]) == 0, b
        else:  # its first occurrence is the batch of sixteen's
            assert result_bytes(out, b) == result_bytes(base, k), (b, k)
    assert out["report"].num_iterations == sum(r.num_iterations for r in out["results"])
    for b in (0, 2, 101, 205, 299):
        p, k, masked = big[b]
        assert k >= 0 and not masked
        assert result_bytes(run(ctx, [p]), 0) == result_bytes(out, b), b
    # a call whose segments are all empty
    empty = [big[6][0]] * 3
    out = run(ctx, empty)
    assert out["report"].num_points == 0 and out["report"].num_iterations == 0
    for res in out["results"]:
        assert (res.success, res.termination, res.num_iterations) == (1, capi.BA_CONVERGENCE, 0) and bits(res) == input_bits(empty[0])


def test_size_refusal_and_the_iteration_caps_limit(ctx, wave):
    problems, base = wave
    kw = sc.batch([problems[3]])
    cams = (capi.Camera * 1)(*kw["cameras"])
    offs = np.array([0, 1048577], np.uint64)  # DSM_ABSOLUTE_POSE_MAX_POINTS + 1
    q, t = np.asarray(kw["qvecs"], np.float64).reshape(-1), np.asarray(kw["tvecs"], np.float64).reshape(-1)
    flags, res = np.zeros(1, np.uint8), capi.PoseRefinementResult()
    L = capi.lib()
    # the offsets are checked before any point is read: the point arrays hold 64 points
    rc = L.dsm_refine_absolute_poses(ctx._h, 1, ctypes.addressof(cams), offs.ctypes.data, kw["points2D"].ctypes.data, kw["points3D"].ctypes.data,
                                     kw["inlier_mask"].ctypes.data, q.ctypes.data, t.ctypes.data, flags.ctypes.data, None, ctypes.addressof(res),
                                     None, None, None)
    assert rc == 1 and b"more than 1048576" in L.dsm_last_error(ctx._h), L.dsm_last_error(ctx._h)
    # the largest accepted cap: runs that end before 100 iterations are the default's bytes
    four = [problems[i] for i in (2, 7, 10, 15)]
    out = run(ctx, four, capi.default_pose_refinement_options(max_num_iterations=capi.POSE_REFINEMENT_MAX_ITERATIONS))
    for b, i in enumerate((2, 7, 10, 15)):
        assert out["results"][b].num_iterations < 100 and result_bytes(out, b) == result_bytes(base, i), i
