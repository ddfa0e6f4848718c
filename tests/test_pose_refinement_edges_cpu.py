"""CPU: the constructions of the pose refinement's edge problems (tests/pose_refinement_scenes.py, DESIGN.md 15 "Edges") on the
numpy restatement alone: the far starts hold rejected steps, the loss scales change the cost, flags 2 frees the extras only, the
masks leave the lanes they name empty, the failing problems fail as the GPU test expects, and every problem the GPU test compares
by the clear rule stays within the measured one-ulp constants, so that test keeps REFINE_TOLERANCE and HAND_COST_TOLERANCE."""
import functools

import numpy as np

from dagsfm_amd import capi
from tests import pose_refinement_ref as ref
from tests import pose_refinement_scenes as sc
from tests.bundle_adjustment_ref import TWO_FOCAL
from tests.test_pose_refinement_cpu import one_ulp, rel

LETTER = {ref.ACCEPTED: "a", ref.REJECTED: "r", ref.INVALID: "i", ref.TOLERANCE: "t"}


def letters(r):
    return "".join(LETTER[s] for s in r["steps"])


def run(p, opts=None):
    r = ref.refine(*sc.args(p), opts=opts)
    return r, ref.is_clear(r["margins"]) and ref.stable_under_rounding(sc.args(p), opts, r)


@functools.lru_cache(maxsize=None)
def far_runs():
    return [(p, listed) + run(p) for p, listed in sc.edge_far_starts()]


@functools.lru_cache(maxsize=None)
def wave_runs():
    return [(p,) + run(p) for p in sc.edge_wave_problems()]


@functools.lru_cache(maxsize=None)
def mask_runs():
    return [(p,) + run(p) for p in sc.edge_masks()]


def test_far_starts_hold_rejected_steps_and_the_dec_reset():
    runs = far_runs()
    listed_clear = [(p, r, c) for p, listed, r, c in runs if listed]
    assert len(listed_clear) == 7 and len(runs) == 9
    for i, (p, listed, r, c) in enumerate(runs):
        print(i, len(p["xy"]), p["cam"].model_id, p["flags"], letters(r), r["termination"], "%.6g -> %.6g" % (r["initial_cost"], r["final_cost"]), "clear", c)
    for p, r, c in listed_clear:
        assert r["success"] and "r" in letters(r) and letters(r)[0] == "a", letters(r)
    # the project's bar: at least 90 % of what the GPU test compares by the clear rule is clear
    assert sum(c for _, _, c in listed_clear) >= 0.9 * len(listed_clear)
    assert any("rrrrr" in letters(r) for _, r, _ in listed_clear)  # dec 2, 4, 8, 16, 32
    # a rejection, accepted steps, a rejection again: the second one divides by the reset dec = 2
    assert any("r" in letters(r).split("r", 1)[1].lstrip("r").lstrip("a") for _, r, _ in listed_clear if "ra" in letters(r))
    assert any(letters(r).endswith("t") for _, r, _ in listed_clear) and any(letters(r).endswith("a") for _, r, _ in listed_clear)
    stopped = [r for p, r, _ in listed_clear if r["final_cost"] > 0.5 * r["initial_cost"]]
    assert len(stopped) == 1 and letters(stopped[0]) == "arrrrra"  # the gradient test ends it far from the others' minimum
    (p7, _, r7, c7), (p8, _, r8, c8) = runs[7:]
    assert not c7 and not c8  # the two rows of the other rule
    assert r7["success"] and r7["termination"] == ref.CONVERGENCE and r7["num_iterations"] == 50 and letters(r7).count("r") >= 10
    assert r8["success"] and r8["termination"] == ref.NO_CONVERGENCE and r8["num_iterations"] == 100 and len(r8["steps"]) == 100


def clear_rule_cases():
    """(name, problem, options, run) of everything the GPU test compares by the clear rule with REFINE_TOLERANCE."""
    out = [("far %d" % i, p, None, r) for i, (p, listed, r, c) in enumerate(far_runs()) if listed and c]
    out += [("wave %d" % i, p, None, r) for i, (p, r, c) in enumerate(wave_runs()) if c and len(p["xy"]) > 2]
    out += [("mask " + n, p, None, r) for n, (p, r, c) in zip(sc.MASK_NAMES, mask_runs()) if c]
    L = sc.edge_loss_scale_problem()
    out += [("scale %g" % s, L, dict(loss_function_scale=s), run(L, dict(loss_function_scale=s))[0]) for s in sc.LOSS_SCALES]
    out += [("flags 2 model %d" % m, p, None, run(p)[0]) for m, p in sc.edge_flags2().items()]
    q = sc.edge_quaternion_problem()
    for name, p in (("zero qvec", dict(q, qvec=np.zeros(4))), ("qvec x 1.7", dict(q, qvec=q["qvec"] * 1.7))):
        out.append((name, p, None, run(p)[0]))
    return out


def test_one_ulp_sensitivity_of_the_edge_problems_stays_within_the_grid_constant():
    """Measured as test_one_ulp_sensitivity_stays_within_the_measured_constants measures the grid: every input moved by one ulp,
    one seeded direction per problem, no decision flipped.  The far starts run three times as long as the grid's and reach
    6.11e-13 (the run that stops at a cost of 510); everything is far inside MEASURED_ULP_SENSITIVITY, so the GPU test keeps
    REFINE_TOLERANCE and no edge constant is added."""
    worst = {}
    for i, (name, p, o, r) in enumerate(clear_rule_cases()):
        u = ref.refine(*one_ulp(p, i), opts=o)
        assert u["steps"] == r["steps"] and u["termination"] == r["termination"], name
        w = max(rel(u["qvec"], r["qvec"]), rel(u["tvec"], r["tvec"]), rel(u["camera_params"], r["camera_params"]),
                rel([u["initial_cost"]], [r["initial_cost"]]))
        if r["final_cost"] > 1e-9 * r["initial_cost"]:  # (the exact three-point fit's final cost goes by the hand rule, below)
            w = max(w, rel([u["final_cost"]], [r["final_cost"]]))
        print(name, "%.3e" % w)
        worst[name.split()[0]] = max(worst.get(name.split()[0], 0.0), w)
    print({k: "%.3e" % v for k, v in worst.items()})
    assert len(worst) == 7 and max(worst.values()) <= sc.MEASURED_ULP_SENSITIVITY


def test_loss_scale_changes_the_cost_and_the_run():
    p = sc.edge_loss_scale_problem()
    costs, iters = [], []
    for s in (1.0,) + sc.LOSS_SCALES:
        r, c = run(p, dict(loss_function_scale=s))
        plain = ref.cauchy_cost(p["cam"], p["xy"], p["X"], p["mask"], p["qvec"], p["tvec"], scale=s)
        assert abs(r["initial_cost"] - plain) <= 1e-12 * plain, s
        assert c and r["success"] and r["final_cost"] < r["initial_cost"], s
        costs.append(r["initial_cost"])
        iters.append(r["num_iterations"])
    print(costs, iters)
    assert iters[1:] == [19, 5, 2]
    for i in range(4):
        for j in range(i):
            assert abs(costs[i] - costs[j]) > 0.1 * max(costs[i], costs[j])
    # b = scale^2 with c = 1 / b swapped (the loss of 1 / scale), or the square forgotten (the loss of sqrt(scale)), is another cost
    for s, cost in zip(sc.LOSS_SCALES, costs[1:]):
        for wrong in (1.0 / s, np.sqrt(s)):
            w = ref.cauchy_cost(p["cam"], p["xy"], p["X"], p["mask"], p["qvec"], p["tvec"], scale=wrong)
            assert abs(w - cost) > 0.1 * max(w, cost), (s, wrong)


def test_flags_2_frees_the_extras_alone():
    for m, p in sc.edge_flags2().items():
        r, c = run(p)
        assert c and r["success"] and len(p["xy"]) == 64, m
        before = np.array(list(p["cam"].params))
        nfoc = 2 if m in TWO_FOCAL else 1
        assert r["camera_params"][:nfoc + 2].tobytes() == before[:nfoc + 2].tobytes(), m
        moved = [j for j in range(12) if r["camera_params"][j] != before[j]]
        if m in (0, 1):  # no extras: the problem of flags 0, the same bits
            z = ref.refine(*sc.args(dict(p, flags=0)))
            assert not moved and ref.free_indices(m, 2) == []
            for key in ("qvec", "tvec", "camera_params"):
                assert r[key].tobytes() == z[key].tobytes(), (m, key)
            assert (r["steps"], r["final_cost"], r["margins"]) == (z["steps"], z["final_cost"], z["margins"]), m
        else:
            assert moved and moved == ref.free_indices(m, 2) and min(moved) >= nfoc + 2, (m, moved)


def test_wave_edge_sizes_and_masks():
    runs = wave_runs()
    assert [len(p["xy"]) for p, _, _ in runs] == list(sc.WAVE_SIZES) + list(sc.WAVE_SIZES[2:]) + [65, 129]
    assert all(p["mask"].all() for p, _, _ in runs)
    hand = sc.hand_problems()
    for (p, r, c), k in zip(runs[:2], ("n1", "n2")):
        # a segment of one or two points is the hand problem with one or two inliers among forty: masked points add +0.0
        h = ref.refine(*sc.args(hand[k]))
        assert r["steps"] == h["steps"] and r["final_cost"] == h["final_cost"] and r["initial_cost"] == h["initial_cost"], k
        assert r["qvec"].tobytes() == h["qvec"].tobytes() and r["tvec"].tobytes() == h["tvec"].tobytes(), k
        assert r["success"] and r["final_cost"] < 1e-3 * r["initial_cost"]
    for p, r, c in runs[2:]:
        assert c and r["success"] and r["num_successful_steps"] >= 2 and r["num_residual_blocks"] == len(p["xy"])
    lanes = np.arange(129) % 64
    masks = mask_runs()
    assert [r["num_residual_blocks"] for _, r, _ in masks] == list(sc.MASK_RESIDUAL_BLOCKS)
    m = [np.asarray(p["mask"], bool) for p, _, _ in masks]
    assert set(lanes[m[0]]) == {0} and not m[1][:64].any() and m[1][64:].all() and list(np.nonzero(m[2])[0]) == [128]
    assert 63 not in set(lanes[m[3]]) and len(set(lanes[m[3]])) == 63
    print([(n, letters(r), c) for n, (_, r, c) in zip(sc.MASK_NAMES, masks)])
    assert [c for _, _, c in masks] == [True, True, False, True]  # one inlier alone is not clear: the other rule
    # three inliers and one inlier are fitted exactly: their final cost is compared against the initial cost, as the hand problems'
    for k in (0, 2):
        p, r, c = masks[k]
        assert r["success"] and r["final_cost"] < 1e-9 * r["initial_cost"]
        for seed in range(16):
            u = ref.refine(*one_ulp(p, seed))
            assert u["success"] and abs(u["final_cost"] - r["final_cost"]) <= sc.MEASURED_ULP_SENSITIVITY_HAND * r["initial_cost"], (k, seed)
    # any non-zero byte is an inlier
    p = runs[-1][0]
    for fill in (2, 255):
        r = ref.refine(*sc.args(dict(p, mask=np.full(129, fill, np.uint8))))
        assert r["qvec"].tobytes() == runs[-1][1]["qvec"].tobytes() and r["steps"] == runs[-1][1]["steps"]


def test_failures_fail_as_stated():
    p = sc.edge_nonfinite_cost()
    assert np.isfinite(p["xy"]).all()
    r = ref.refine(*sc.args(p))
    assert (r["termination"], r["success"], r["num_iterations"], r["steps"]) == (ref.FAILURE, False, 0, [])
    assert r["initial_cost"] == np.inf and r["final_cost"] == np.inf and r["num_residual_blocks"] == 64
    assert abs(np.linalg.norm(r["qvec"]) - 1.0) < 1e-15 and r["tvec"].tobytes() == np.asarray(p["tvec"]).tobytes()
    for flags in (0, 1):
        p = sc.edge_invalid_steps(1e155, flags)
        with np.errstate(over="ignore"):  # (J'J overflows: that is the construction)
            r = ref.refine(*sc.args(p))
        assert letters(r) == "iiiii" and r["termination"] == ref.FAILURE and not r["success"], flags
        assert (r["num_iterations"], r["num_invalid_steps"], r["num_successful_steps"]) == (5, 5, 0)
        assert r["initial_cost"] == r["final_cost"] == 24.260151319598084  # 70 x 1/2 log 2, in the device's summation order
        assert abs(r["initial_cost"] - 35.0 * np.log(2.0)) < 1e-13
        assert r["qvec"].tobytes() == p["qvec"].tobytes() and r["tvec"].tobytes() == p["tvec"].tobytes()
        assert list(r["camera_params"]) == list(p["cam"].params)
        c = ref.refine(*sc.args(sc.edge_invalid_steps(1e150, flags)))  # the control: the same construction below the overflow
        assert letters(c) == "t" and c["success"] and c["termination"] == ref.CONVERGENCE and c["num_invalid_steps"] == 0
    # accepted steps, then five invalid ones: FAILURE keeps the last accepted state; one ulp on the inputs (16 directions) moves
    # neither the decisions nor, beyond the grid's constant, the result
    p, o = sc.edge_accepted_then_invalid()
    with np.errstate(all="ignore"):
        r = ref.refine(*sc.args(p), opts=o)
        assert letters(r) == "arraaaaaaiiiii" and r["termination"] == ref.FAILURE and not r["success"]
        assert (r["num_iterations"], r["num_successful_steps"], r["num_invalid_steps"]) == (14, 7, 5)
        assert np.isfinite(r["final_cost"]) and r["final_cost"] < 0.1 * r["initial_cost"] and rel(r["tvec"], p["tvec"]) > 0.1
        for seed in range(16):
            u = ref.refine(*one_ulp(p, seed), opts=o)
            assert u["steps"] == r["steps"] and u["termination"] == r["termination"], seed
            assert max(rel(u["qvec"], r["qvec"]), rel(u["tvec"], r["tvec"]), rel([u["final_cost"]], [r["final_cost"]]),
                       rel([u["initial_cost"]], [r["initial_cost"]])) <= sc.MEASURED_ULP_SENSITIVITY, seed
    # a loss scale so small that 1 + s / b overflows: the failure register_images is driven with
    q = sc.edge_quaternion_problem()
    r = ref.refine(*sc.args(q), opts=dict(loss_function_scale=sc.FAILING_LOSS_SCALE))
    assert r["termination"] == ref.FAILURE and not r["success"] and r["num_iterations"] == 0 and not np.isfinite(r["initial_cost"])


def test_quaternion_starts_and_the_big_batch_layout():
    q = sc.edge_quaternion_problem()
    z, cz = run(dict(q, qvec=np.zeros(4)))
    assert cz and z["num_iterations"] == 11 and z["success"]  # NormalizeQuaternion's identity, 0.9 rad from the planted pose
    a, ca = run(q)
    b, cb = run(dict(q, qvec=q["qvec"] * 1.7))
    assert ca and cb and a["steps"] == b["steps"]
    # normalisation comes first, so the scaled start is the same start up to the rounding of q * 1.7 / |q * 1.7|
    assert max(rel(a["qvec"], b["qvec"]), rel(a["tvec"], b["tvec"]), rel([a["final_cost"]], [b["final_cost"]])) <= sc.MEASURED_ULP_SENSITIVITY
    big = sc.edge_big_batch()
    assert len(big) == 300 > 256
    empty = [b for b, (p, k, masked) in enumerate(big) if k < 0]
    masked = [b for b, (p, k, m) in enumerate(big) if m]
    assert len(empty) == 42 and all(len(big[b][0]["xy"]) == 0 for b in empty) and 0 < empty[0] and empty[-1] < 299
    assert len(masked) >= 20 and all(not big[b][0]["mask"].any() and len(big[b][0]["xy"]) for b in masked)
    assert {k for _, k, m in big if k >= 0 and not m} == set(range(16))  # every one of the sixteen occurs unmasked
    assert max(len(p["xy"]) for p, _, _ in big) == 129
    assert capi.POSE_STEP_REJECTED == ref.REJECTED and capi.POSE_STEP_INVALID == ref.INVALID
