"""What the absolute pose GPU tests share (tests/test_absolute_pose_gpu.py, tests/test_absolute_pose_edges_gpu.py): the batch call, the
comparison rule of DESIGN.md 14, and the edge problems with their restatement records, computed once per process.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import absolute_pose_ref as ref
from tests import absolute_pose_scenes as scenes


def run_batch(ctx, problems, options=None, seeds=None):
    offs = np.concatenate([[0], np.cumsum([len(p["xy"]) for p in problems])]).astype(np.uint64)
    xy = np.concatenate([p["xy"].reshape(-1, 2) for p in problems] + [np.zeros((0, 2))])
    X = np.concatenate([p["X"].reshape(-1, 3) for p in problems] + [np.zeros((0, 3))])
    return ctx.estimate_absolute_poses([p["cam"] for p in problems], [int(p["sweep"]) for p in problems], offs, xy, X, options, seeds), offs


def result_bytes(out):
    return b"".join(bytes(r) for r in out["results"]) + out["inlier_mask"].tobytes()


def close(a, b, what, tolerance=scenes.POSE_TOLERANCE):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    scale = max(float(np.max(np.abs(b))), 1e-300)
    assert float(np.max(np.abs(a - b))) <= tolerance * scale, (what, float(np.max(np.abs(a - b))) / scale)


def compare(res, mask, margins, want, index, tolerance=scenes.POSE_TOLERANCE):
    """One problem of a batch against the restatement's record; returns whether it was clear on both sides."""
    clear = ref.is_clear(want["margins"]) and ref.is_clear(list(margins))
    assert bool(res.success) == want["success"], index
    if clear:
        assert res.factor_index == want["factor_index"], index
        assert res.num_inliers == want["num_inliers"], index
        if want["success"]:
            assert res.num_trials == want["num_trials"], index
            assert bool(res.model_is_local) == want["model_is_local"], index
            assert (mask == want["mask"]).all(), index
            close(list(res.proj_matrix), want["proj_matrix"], "model %s" % (index,), tolerance)
            close(list(res.qvec), want["qvec"], "qvec %s" % (index,), tolerance)
            close(list(res.tvec), want["tvec"], "tvec %s" % (index,), tolerance)
            assert list(res.focal_params) == list(want["focal_params"]), index
            assert res.focal_length_factor == want["focal_length_factor"], index
    else:
        assert abs(int(res.num_inliers) - want["num_inliers"]) <= 0.02 * max(want["num_inliers"], 1) + 0.5, index
    return clear


# ------------------------------------------------------------------------------------------------ the edge problems
@functools.lru_cache(maxsize=None)
def _edge_cases():
    return scenes.edge_cases()


@functools.lru_cache(maxsize=None)
def edge_problem(name):
    """name: an edge case's name, ("grid", k) for EDGE_GRID[k], or ("five", sweep, k) for the large batches' k-th problem.
    Returns dict(cam, xy, X, sweep, opts, seeds): opts the options that differ from the defaults, seeds one per factor."""
    if isinstance(name, str):
        return _edge_cases()[name]
    if name[0] == "grid":
        p = scenes.grid_problem(scenes.EDGE_GRID[name[1]])
        p.update(opts={}, seeds=scenes.edge_seeds(name[1]))
        return p
    return scenes.batch_five(name[1])[name[2]]


def edge_names():
    return [("grid", k) for k in range(len(scenes.EDGE_GRID))] + list(_edge_cases()) + \
        [("five", sweep, k) for sweep in (False, True) for k in range(len(scenes.BATCH_FIVE))]


@functools.lru_cache(maxsize=None)
def edge_want(name):
    """The restatement's record of an edge problem, under the problem's own options and seeds."""
    p = edge_problem(name)
    return ref.estimate_absolute_pose(p["cam"], p["xy"], p["X"], p["sweep"], opts=p["opts"], seeds=p["seeds"])
