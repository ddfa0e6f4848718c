"""GPU: dsm_estimate_absolute_poses at its edges, against the sequential restatement (tests/absolute_pose_ref.py) under the same options
and the same explicit seeds, by the comparison rule of DESIGN.md 14 (tests/absolute_pose_compare.py): sizes at and beside the
multiples of 64 and 256, inliers placed among the lanes, the RANSAC and sweep options with both exits of the trial loop, a tie
among the factors, a run that fails with N >= 3, the report's sums, more than 65535 problems and runs in one call, and the factor
limit.  tests/test_absolute_pose_edges_cpu.py holds the committed scenes to the conditions assumed here, without a device."""
import numpy as np
import pytest

from dagsfm_amd import capi
from tests import absolute_pose_ref as ref
from tests import absolute_pose_scenes as scenes
from tests.absolute_pose_compare import compare, edge_problem, edge_want, run_batch

pytestmark = pytest.mark.gpu

TOLERANCE = scenes.POSE_TOLERANCE  # unchanged: the CPU test holds the edge problems to the constant it is built from


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def run_names(ctx, names):
    """The named edge problems as one batch under their (common) options and their own seeds."""
    problems = [edge_problem(n) for n in names]
    assert all(p["opts"] == problems[0]["opts"] for p in problems)
    options = capi.default_absolute_pose_options(**problems[0]["opts"])
    return run_batch(ctx, problems, options, np.stack([p["seeds"] for p in problems]))


def mask_of(out, offs, b):
    return out["inlier_mask"][int(offs[b]):int(offs[b + 1])]


def model_difference(res, want):
    """Printed beside every comparison: the largest difference of the device's model from the restatement's, relative."""
    if not (res.success and want["success"]):
        return 0.0
    return float(np.max(np.abs(np.array(list(res.proj_matrix)) - want["proj_matrix"].ravel())) / np.max(np.abs(want["proj_matrix"])))


def compare_names(ctx, names, all_clear=True):
    """Runs and compares; returns (out, offs, the list of clear flags).  all_clear: every problem must be clear on both sides."""
    out, offs = run_names(ctx, names)
    flags = []
    for b, n in enumerate(names):
        want, res = edge_want(n), out["results"][b]
        print(n, "device", res.success, res.factor_index, res.num_inliers, res.num_trials, res.model_is_local,
              "ref", want["success"], want["factor_index"], want["num_inliers"], want["num_trials"], want["model_is_local"],
              "margins %.1e %.1e" % (min(out["margins"][b]), min(want["margins"])), "model differs by %.1e" % model_difference(res, want))
        flags.append(compare(res, mask_of(out, offs, b), out["margins"][b], want, n, TOLERANCE))
        if all_clear:
            assert flags[-1], n
    return out, offs, flags


def record_bytes(out, offs, b):
    return bytes(out["results"][b]) + mask_of(out, offs, b).tobytes() + out["margins"][b].tobytes()


def run_sums(names):
    runs = [r for n in names for r in edge_want(n)["runs"]]
    return sum(r["num_trials"] for r in runs), sum(r["num_models"] for r in runs), sum(r["num_lo"] for r in runs)


def test_sizes_at_the_wave_and_tile_edges_and_the_reports_sums(ctx):
    """EDGE_GRID in one batch: N at and beside the multiples of 64 and 256, inlier counts on both sides of 64 and 128.  Then its
    clear subset as a batch of its own: the same bytes, and the report's sums equal the restatement's over the runs."""
    names = [("grid", k) for k in range(len(scenes.EDGE_GRID))]
    out, offs, flags = compare_names(ctx, names, all_clear=False)
    assert all(r.success for r in out["results"])
    print("clear on both sides: %d of %d" % (sum(flags), len(names)))
    assert sum(flags) >= 0.9 * len(names)
    assert out["report"].num_runs == len(names)
    sub = [n for n, f in zip(names, flags) if f]
    sout, soffs = run_names(ctx, sub)
    for k, n in enumerate(sub):
        assert record_bytes(sout, soffs, k) == record_bytes(out, offs, names.index(n)), n
    rep = sout["report"]
    assert (rep.num_trials, rep.num_models, rep.num_local_optimizations) == run_sums(sub)
    assert rep.num_runs == len(sub) and rep.num_problems == len(sub)


PLACED = ("one_lane", "one_lane_found", "first_late", "first_63", "first_64", "last_stride", "all_64", "all_65")


def test_where_the_inliers_sit_among_the_lanes(ctx):
    out, offs, _ = compare_names(ctx, PLACED)
    res = dict(zip(PLACED, out["results"]))
    mask = {n: mask_of(out, offs, b) for b, n in enumerate(PLACED)}
    assert res["one_lane"].num_trials == 585
    assert set(np.nonzero(mask["one_lane_found"])[0].tolist()) == set(range(5, 640, 64)) and res["one_lane_found"].model_is_local
    for n, first in (("first_late", 130), ("first_63", 63), ("first_64", 64)):
        assert int(np.argmax(mask[n])) == first and res[n].num_inliers == int(mask[n].sum()), n
    assert tuple(np.nonzero(mask["last_stride"])[0].tolist()) == scenes.LAST_STRIDE_INLIERS and res["last_stride"].model_is_local
    assert mask["all_64"].all() and len(mask["all_64"]) == 64 and mask["all_65"].all() and len(mask["all_65"]) == 65
    rep = out["report"]
    assert (rep.num_trials, rep.num_models, rep.num_local_optimizations) == run_sums(PLACED)


OPTION_CASES = ("max_error_1", "max_error_100", "confidence_half", "confidence_six_nines", "cap_5", "earliest_abort", "min_1000",
                "no_trials", "sweep_1", "sweep_2", "sweep_7")


@pytest.mark.parametrize("name", OPTION_CASES)
def test_options_against_the_restatement_under_the_same_options(ctx, name):
    out, offs, _ = compare_names(ctx, [name])
    res, rep, want = out["results"][0], out["report"], edge_want(name)
    assert (rep.num_trials, rep.num_models, rep.num_local_optimizations) == run_sums([name])
    assert rep.num_runs == len(want["runs"]) == (rep.num_factors if edge_problem(name)["sweep"] else 1)
    if name == "cap_5":  # the cap exit
        assert res.success and res.num_trials == 5
    if name == "earliest_abort":  # the abort exit with its nt += 1, as early as it can fire
        assert res.success and res.num_trials == 3 and res.num_inliers == 50
    if name == "min_1000":  # the constructor's cap of 585 wins over min_num_trials
        assert res.success and res.num_trials == 585
    if name == "no_trials":  # the cap is 0 trials
        assert capi.absolute_pose_max_trials(capi.default_absolute_pose_options(**edge_problem(name)["opts"])) == 0
        assert not res.success and res.factor_index == -1 and res.num_trials == 0 and res.num_inliers == 0
        assert not out["inlier_mask"].any() and rep.num_trials == 0 and rep.num_models == 0
    if name.startswith("sweep_"):
        n = int(name[6:])
        assert rep.num_runs == len(ref.focal_length_factors(n, 0.5, 2.0)) == rep.num_factors
        assert res.success and res.focal_params[0] == edge_problem(name)["cam"].params[0] * res.focal_length_factor


def test_a_tie_among_the_factors_keeps_the_lowest_index(ctx):
    want = edge_want("factor_tie")
    tied = [s for s, r in enumerate(want["runs"]) if r["success"] and r["num_inliers"] == want["num_inliers"]]
    assert len(tied) >= 2 and want["factor_index"] == tied[0]  # the tie itself: the scene cannot drift out of the condition
    out, _, _ = compare_names(ctx, ["factor_tie"])
    assert out["results"][0].factor_index == tied[0] and out["results"][0].num_inliers == want["num_inliers"]


def test_a_run_that_fails_with_eight_points(ctx):
    """Eight correspondences of one world point: P3P finds no model in any of the 585 trials."""
    want = edge_want("same_point")
    assert not want["success"] and want["num_inliers"] == 0 and want["runs"][0]["num_models"] == 0
    out, offs, _ = compare_names(ctx, ["same_point"])
    res, rep = out["results"][0], out["report"]
    assert res.success == 0 and res.factor_index == -1 and res.num_trials == 0 and res.num_inliers == 0
    assert len(out["inlier_mask"]) == 8 and not out["inlier_mask"].any()
    assert rep.num_trials == want["runs"][0]["num_trials"] == 585 and rep.num_models == 0 and rep.num_local_optimizations == 0
    # beside a good problem in one batch: the good one's bytes are unchanged, on either side of the failing one
    alone, aoffs = run_names(ctx, ["all_65"])
    for order in (["same_point", "all_65"], ["all_65", "same_point"]):
        both, boffs = run_names(ctx, order)
        g, f = order.index("all_65"), order.index("same_point")
        assert record_bytes(both, boffs, g) == record_bytes(alone, aoffs, 0)
        assert record_bytes(both, boffs, f) == record_bytes(out, offs, 0)
        assert both["results"][g].success and not both["results"][f].success


def repeated(ctx, five_names, B):
    """B problems made of the five repeated, in one call; every record must equal the five's own."""
    base, boffs, flags = compare_names(ctx, five_names, all_clear=False)
    assert sum(flags) >= 3
    five = [edge_problem(n) for n in five_names]
    idx = np.arange(B) % 5
    lens = np.array([len(p["xy"]) for p in five])
    offs = np.concatenate([[0], np.cumsum(lens[idx])]).astype(np.uint64)
    reps, rest = B // 5, B % 5
    xy = np.concatenate([np.tile(np.concatenate([p["xy"] for p in five]), (reps, 1))] + [p["xy"] for p in five[:rest]])
    X = np.concatenate([np.tile(np.concatenate([p["X"] for p in five]), (reps, 1))] + [p["X"] for p in five[:rest]])
    seeds = np.stack([p["seeds"] for p in five])[idx]
    cams = [five[i]["cam"] for i in idx]  # built once
    out = ctx.estimate_absolute_poses(cams, [int(five[i]["sweep"]) for i in idx], offs, xy, X,
                                      capi.default_absolute_pose_options(**five[0]["opts"]), seeds)
    size = len(bytes(base["results"][0]))
    got = np.frombuffer(b"".join(bytes(r) for r in out["results"]), np.uint8).reshape(B, size)
    wanted = np.stack([np.frombuffer(bytes(r), np.uint8) for r in base["results"]])[idx]
    wrong = np.nonzero((got != wanted).any(axis=1))[0]
    assert len(wrong) == 0, wrong[:10]
    base_masks = [mask_of(base, boffs, k) for k in range(5)]
    full = np.concatenate(base_masks)
    wanted_mask = np.concatenate([np.tile(full, reps)] + base_masks[:rest])
    assert len(out["inlier_mask"]) == len(wanted_mask) == int(offs[-1]) and (out["inlier_mask"] == wanted_mask).all()
    assert (out["margins"].view(np.uint64) == base["margins"][idx].view(np.uint64)).all()
    for b in range(B - 4, B):  # the problems past the last full grid row
        assert bytes(out["results"][b]) == bytes(base["results"][b % 5]), b
        assert (out["inlier_mask"][int(offs[b]):int(offs[b + 1])] == base_masks[b % 5]).all(), b
    rb, ro = base["report"], out["report"]
    assert ro.num_problems == B and ro.num_runs == sum(base["report"].num_runs // 5 for _ in range(B)) == B * (rb.num_runs // 5)
    trials = [sum(r["num_trials"] for r in edge_want(n)["runs"]) for n in five_names]
    if all(flags):
        assert ro.num_trials == sum(trials[i] for i in idx)
    return out


def test_more_than_65535_problems_in_one_call(ctx):
    """65539 problems: k_ap_prepare's and k_ap_mask's grids stop at 65535 rows and stride over the rest."""
    out = repeated(ctx, [("five", False, k) for k in range(5)], scenes.BATCH_PROBLEMS)
    assert out["report"].num_runs == 65539


def test_more_than_65535_runs_of_fewer_problems(ctx):
    """2115 sweep problems x 31 factors = 65565 runs: k_ap_prepare strides, k_ap_mask does not."""
    out = repeated(ctx, [("five", True, k) for k in range(5)], scenes.BATCH_SWEEP_PROBLEMS)
    assert out["report"].num_runs == 65565 and out["report"].num_factors == 31


def test_the_factor_limit(ctx):
    accepted, refused = ref.focal_length_factors(1023, 0.1, 10.0), ref.focal_length_factors(1024, 0.1, 10.0)
    limit = len(accepted)
    assert len(refused) == limit + 1
    p = edge_problem("factors_1024")
    assert p["opts"]["num_focal_length_samples"] == 1023 and len(p["seeds"]) == limit and len(p["xy"]) == 20
    out, _, _ = compare_names(ctx, ["factors_1024"])
    assert out["report"].num_runs == limit == out["report"].num_factors and out["results"][0].success
    rep = out["report"]
    assert (rep.num_trials, rep.num_models, rep.num_local_optimizations) == run_sums(["factors_1024"])
    over = capi.default_absolute_pose_options(**dict(p["opts"], num_focal_length_samples=1024))
    with pytest.raises(capi.DsmError) as e:
        run_batch(ctx, [p], over, np.zeros((1, len(refused)), np.uint32))
    assert "focal-length factors" in str(e.value) and "dsm_estimate_absolute_poses" in str(e.value)
