"""CPU-only: the conditions the edge tests of absolute pose estimation (tests/test_absolute_pose_edges_gpu.py) rest on -- the
committed edge scenes are clear in the restatement and are the scenes their names say, the one-ulp sensitivity of the new problems
stays within the measured constant POSE_TOLERANCE is built from -- and the stage's host-side tables against the restatement: the
constructor's trial cap, the focal-length factors, ComputeNumTrials.  Nothing here measures the device."""
import numpy as np

from dagsfm_amd import capi
from tests import absolute_pose_ref as ref
from tests import absolute_pose_scenes as scenes
from tests import oracle_lib
from tests.absolute_pose_compare import edge_names as _all_names, edge_problem as _problem, edge_want as want


def _cases():
    return scenes.edge_cases()


def test_clear_share_of_the_edge_grid():
    """At least 90 % of EDGE_GRID is clear in the restatement alone: a condition on the committed seeds."""
    sizes = sorted(set(e[1] for e in scenes.EDGE_GRID))
    assert set((6, 7, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 513, 1025)) <= set(sizes)
    assert any(e[4] in (1, 4, 5, 6, 7, 10) for e in scenes.EDGE_GRID) and len(set(e[4] for e in scenes.EDGE_GRID)) > 2
    clear, counts = 0, []
    for k in range(len(scenes.EDGE_GRID)):
        w = want(("grid", k))
        assert w["success"]
        clear += ref.is_clear(w["margins"])
        counts.append(w["num_inliers"])
    print("clear problems of the edge grid: %d of %d; inlier counts %s" % (clear, len(scenes.EDGE_GRID), counts))
    assert clear >= 0.9 * len(scenes.EDGE_GRID)
    for edge in (64, 128):  # the inlier counts fall on both sides of the wave's stride too
        assert any(c < edge for c in counts) and any(c == edge for c in counts) and any(edge < c <= edge + 1 for c in counts)


def test_named_cases_are_clear_and_are_what_their_names_say():
    """Every named case is clear in the restatement (a case that is not gets only the loose comparison on the device and tests
    nothing), and holds the condition it was built for."""
    c = _cases()
    for name in c:
        w = want(name)
        print(name, "success", w["success"], "factor", w["factor_index"], "inliers", w["num_inliers"], "trials", w["num_trials"],
              "local", w["model_is_local"], "least margin %.1e" % min(w["margins"]))
        assert ref.is_clear(w["margins"]), name
        assert len(w["runs"]) == len(c[name]["seeds"]) if c[name]["sweep"] else len(w["runs"]) == 1
    lane5 = set(range(5, 640, 64))
    w = want("one_lane")  # ten planted inliers of 640 are never sampled together: the run goes to the cap on chance support
    assert w["success"] and w["num_trials"] == 585 == w["runs"][0]["num_trials"]
    w = want("one_lane_found")  # the searched seed draws three of them in trial 38: the mask is lane 5 alone, on every stride
    assert w["success"] and set(np.nonzero(w["mask"])[0].tolist()) == lane5 and w["runs"][0]["num_lo"] > 0
    orc = oracle_lib.load()
    s = orc.sample_sequence(int(c["one_lane_found"]["seeds"][0]), 3, 640, 585)
    assert int(np.argmax((s % 64 == 5).all(axis=1))) == 38
    for name, first in (("first_late", 130), ("first_63", 63), ("first_64", 64)):
        w = want(name)
        assert w["success"] and int(np.argmax(w["mask"])) == first and w["runs"][0]["num_lo"] > 0, name
    w = want("last_stride")  # points 128 and 129 are the last, partial stride of 130; the searched seed draws three inliers in trial 37
    assert w["success"] and tuple(np.nonzero(w["mask"])[0].tolist()) == scenes.LAST_STRIDE_INLIERS and w["model_is_local"]
    s = orc.sample_sequence(int(c["last_stride"]["seeds"][0]), 3, 130, 585)
    assert int(np.argmax(np.isin(s, scenes.LAST_STRIDE_INLIERS).all(axis=1))) == 37
    assert want("all_64")["num_inliers"] == 64 and want("all_65")["num_inliers"] == 65
    assert want("confidence_half")["num_trials"] <= want("confidence_six_nines")["num_trials"]
    assert want("cap_5")["success"] and want("cap_5")["num_trials"] == 5
    # the earliest abort: trial 0 finds every point, ComputeNumTrials is 1, trial 1's first model meets nt >= 1 and aborts,
    # the loop's increment and the abort path's nt += 1 make it 3
    w = want("earliest_abort")
    assert w["success"] and w["num_inliers"] == 50 and w["num_trials"] == 3
    assert want("min_1000")["num_trials"] == 585
    w = want("no_trials")
    assert not w["success"] and w["num_trials"] == 0 and w["num_inliers"] == 0 and w["runs"][0]["num_trials"] == 0
    assert ref.max_num_trials(dict(ref.DEFAULTS, **c["no_trials"]["opts"])) == 0
    for name, n in (("sweep_1", 1), ("sweep_2", 2), ("sweep_7", 7)):
        w = want(name)
        assert len(w["runs"]) == len(ref.focal_length_factors(n, 0.5, 2.0)) == n + 1 and w["success"], name
        assert 0.9 * 800 < w["focal_params"][0] < 1.1 * 800, name
    assert c["sweep_7"]["cam"].model_id in (1, 4, 5, 6, 7, 10)
    w = want("factor_tie")
    tied = [s for s, r in enumerate(w["runs"]) if r["success"] and r["num_inliers"] == w["num_inliers"]]
    assert len(tied) >= 2 and w["factor_index"] == tied[0] and 0 < tied[0] and tied[-1] < len(w["runs"]) - 1
    w = want("same_point")
    assert not w["success"] and w["num_inliers"] == 0 and w["factor_index"] == -1
    assert w["runs"][0]["num_models"] == 0 and w["runs"][0]["num_trials"] == 585 and len(c["same_point"]["xy"]) == 8
    assert len(want("factors_1024")["runs"]) == len(ref.focal_length_factors(1023, 0.1, 10.0)) == 1024


def test_one_ulp_sensitivity_of_the_edge_problems():
    """What POSE_TOLERANCE rests on, re-measured on the new problems, on the restatement alone: every input of every clear one moved
    by one ulp, in two seeded random directions of its own, flips no decision and changes model / qvec / tvec by at most
    MEASURED_ULP_SENSITIVITY of the largest entry.  So the edge GPU tests use POSE_TOLERANCE unchanged."""
    worst, worst_name, measured = 0.0, None, 0
    for index, name in enumerate(_all_names()):
        a = want(name)
        if not ref.is_clear(a["margins"]) or not a["success"]:
            continue
        p = _problem(name)
        measured += 1
        for direction in range(2):
            rng = np.random.default_rng([2025, index, direction])
            b = ref.estimate_absolute_pose(p["cam"], scenes.ulp_perturbed(rng, p["xy"]), scenes.ulp_perturbed(rng, p["X"]), p["sweep"],
                                           opts=p["opts"], seeds=p["seeds"])
            assert (a["mask"] == b["mask"]).all() and a["num_trials"] == b["num_trials"], name
            assert a["factor_index"] == b["factor_index"] and a["model_is_local"] == b["model_is_local"], name
            for k in ("proj_matrix", "qvec", "tvec"):
                d = float(np.max(np.abs(np.asarray(a[k]) - np.asarray(b[k]))) / np.max(np.abs(np.asarray(a[k]))))
                if d > worst:
                    worst, worst_name = d, name
    print("largest relative change under one ulp over %d clear edge problems: %.3e (%s)" % (measured, worst, worst_name))
    assert measured >= 40
    assert worst <= scenes.MEASURED_ULP_SENSITIVITY


def test_batch_problems_against_the_restatement_inputs():
    """The five problems of the large batches: 10 <= N <= 40, four trials, and how many are clear (printed; the GPU test
    compares the clear ones decision for decision)."""
    for sweep in (False, True):
        clear = 0
        for k, p in enumerate(scenes.batch_five(sweep)):
            assert 10 <= len(p["xy"]) <= 40
            w = want(("five", sweep, k))
            assert all(r["num_trials"] <= 4 for r in w["runs"]) and len(w["runs"]) == (31 if sweep else 1)
            clear += ref.is_clear(w["margins"])
        print("clear problems of the batch's five, sweep %d: %d" % (sweep, clear))
        assert clear >= 3
    assert scenes.BATCH_PROBLEMS > 65535 and scenes.BATCH_PROBLEMS % 5 == 4
    assert scenes.BATCH_SWEEP_PROBLEMS <= 65535 < 31 * scenes.BATCH_SWEEP_PROBLEMS


def test_constructor_cap_against_the_restatement():
    """RANSAC's constructor cap (ransac.h:141-147) in the library and in the restatement, over confidence x min_inlier_ratio."""
    for max_trials in (None, 100):
        for confidence in (0.0, 0.5, 0.9999, 0.999999, 1.0):
            for ratio in (0.0, 1e-5, 0.25, 0.999, 1.0):
                kw = dict(confidence=confidence, min_inlier_ratio=ratio)
                if max_trials is not None:
                    kw["max_num_trials"] = max_trials
                got = capi.absolute_pose_max_trials(capi.default_absolute_pose_options(**kw))
                wanted = ref.max_num_trials(dict(ref.DEFAULTS, **kw))
                assert got == wanted, (kw, got, wanted)
                if wanted > ref.MAX_TRIALS:
                    assert got > ref.MAX_TRIALS and max_trials is None
    assert capi.absolute_pose_max_trials(capi.default_absolute_pose_options(confidence=0.0)) == 0


def test_factor_counts_against_the_restatement():
    """pose.cc:92-98: the library's factors equal the restatement's entry for entry; the loop's length is decided by the
    accumulated rounding of f += fstep, so the count is n or n + 1."""
    for lo, hi in ((0.1, 10.0), (0.5, 2.0)):
        for n in (1, 2, 3, 7, 49, 51, 64, 1000, 1023, 1024):
            f = ref.focal_length_factors(n, lo, hi)
            got = capi.absolute_pose_factors(capi.default_absolute_pose_options(
                num_focal_length_samples=n, min_focal_length_ratio=lo, max_focal_length_ratio=hi))
            print(n, lo, hi, len(f))
            assert len(f) in (n, n + 1) and f[0] == lo
            assert len(got) == len(f) and list(got) == f, (n, lo, hi)
    assert len(ref.focal_length_factors(1023, 0.1, 10.0)) == 1024 and len(ref.focal_length_factors(1024, 0.1, 10.0)) == 1025


def test_compute_num_trials_table_against_the_oracle():
    """The table the device reads (one entry per inlier count k = 0 .. N) is built by the library's host code; the restatement's
    is held to the oracle's ComputeNumTrials here.  Where the quotient is infinite, NaN or past 32 bits the oracle's cast is
    whatever the machine makes of it; it is never below a trial count, which is all the restatement's 2^32 - 1 says."""
    orc = oracle_lib.load()
    never = 2 ** 32 - 1
    for n in (3, 64, 65, 257):
        for confidence in (0.0, 0.5, 0.9999, 0.999999):
            for k in range(n + 1):
                got, wanted = ref.compute_num_trials(k, n, confidence), orc.compute_num_trials(k, n, confidence, 3)
                assert got == min(wanted, never), (k, n, confidence, got, wanted)
            assert ref.compute_num_trials(n, n, confidence) == 1
            assert ref.compute_num_trials(0, n, confidence) == never
