"""Problems of the pose refinement tests (tests/test_pose_refinement_cpu.py, tests/test_pose_refinement_gpu.py): the registrations
of tests/absolute_pose_scenes.py with the mask and the starting pose a registration would hand over.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from dagsfm_amd import capi
from tests import absolute_pose_scenes as scenes
from tests.bundle_adjustment_ref import quat_plus, rot_to_quat

# The tolerances of the GPU comparison (DESIGN.md 15 "Parity"), measured on the restatement, never on the device: every input of
# every clear grid problem moved by one ulp in a seeded random direction (absolute_pose_scenes.ulp_perturbed) changes the costs and
# qvec / tvec / camera parameters by at most MEASURED_ULP_SENSITIVITY (relative; parameters relative to the block's largest entry);
# tests/test_pose_refinement_cpu.py re-measures it and holds it to the constant.  Times 16 for the device's different but equally
# valid operation order in the parts the restatement does not pin (libm's log / sin / cos, the dual numbers' order), as DESIGN.md 14.
# The grid has no problem that is not clear, so that class is represented by the hand problems (hand_problems below: one inlier and
# the collinear set are not clear).  Their data is exact, so their final cost is what the last step left, orders of magnitude below the
# initial cost, and its relative sensitivity is large (2e-8 observed); it is compared against the INITIAL cost instead:
# one ulp on every input, 16 seeded directions, moves the final cost of a hand problem, clear or not, by at most
# MEASURED_ULP_SENSITIVITY_HAND of its initial cost (5.49e-16 observed), times 16 as above.
MEASURED_ULP_SENSITIVITY = 5.5e-11  # 5.38e-11 observed (FULL_OPENCV with its eight extra parameters free)
MEASURED_ULP_SENSITIVITY_HAND = 6e-16
REFINE_TOLERANCE = 16 * MEASURED_ULP_SENSITIVITY
HAND_COST_TOLERANCE = 16 * MEASURED_ULP_SENSITIVITY_HAND

MAX_ERROR = 12.0  # abs_pose_max_error: the mask is the planted pose's inlier set at the estimator's threshold


def planted_quat(P):
    q = rot_to_quat(P[:, :3])
    return q / np.linalg.norm(q)


def problem(seed, n, outliers, noise, model, flags, focal_error=0.0, rot=0.004, trans=0.03):
    """One refinement problem: the registration (seed, n, outliers, noise, model) of absolute_pose_scenes, the mask of the points
    within MAX_ERROR of their planted projection, the planted pose moved by a seeded perturbation (rot rad in the tangent, trans in
    t), the true camera with its focal lengths off by focal_error (relative)."""
    cam, xy, X, P = scenes.registration(seed, n, outliers, noise, model)
    from dagsfm_amd import synthetic
    pc = X @ P[:, :3].T + P[:, 3]
    npar = capi.CAMERA_MODEL_NUM_PARAMS[model]
    u, v = synthetic.world_to_image(model, list(cam.params)[:npar], pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2])
    mask = (np.hypot(u - xy[:, 0], v - xy[:, 1]) <= MAX_ERROR).astype(np.uint8)
    rng = np.random.default_rng([seed, 0xF1E])
    q = quat_plus(planted_quat(P), rng.normal(scale=rot, size=3))[0]
    t = P[:, 3] + rng.normal(scale=trans, size=3)
    if focal_error:
        cam.params[0] *= 1.0 + focal_error
        if model in (1, 4, 5, 6, 7, 10):
            cam.params[1] *= 1.0 + focal_error
    return dict(cam=cam, xy=xy, X=X, mask=mask, qvec=q, tvec=t, flags=flags, P=P, noise=noise)


def grid():
    """The grid of the comparison rule: RANDOM_GRID with the camera constant (a camera another image already refined,
    incremental_mapper.cc:466-470), the two sweep scenes with the focal length free from a 3 % error (what the winning factor of
    the sweep leaves), and per camera model a focal-only and a focal + extras problem (a camera not refined before)."""
    out = []
    for e in scenes.RANDOM_GRID:
        out.append(problem(e[0], e[1], e[2], e[3], e[4], 0))
    for e in scenes.SWEEP_GRID:
        out.append(problem(e[0], e[1], e[2], e[3], e[4], capi.POSE_REFINE_FOCAL_LENGTH, focal_error=0.03))
    for m in range(11):
        out.append(problem(700 + m, 300, 0.2, 0.5, m, capi.POSE_REFINE_FOCAL_LENGTH, focal_error=-0.02))
        out.append(problem(800 + m, 300, 0.2, 0.5, m, capi.POSE_REFINE_FOCAL_LENGTH | capi.POSE_REFINE_EXTRA_PARAMS, focal_error=0.02))
    return out


def args(p):
    return (p["cam"], p["xy"], p["X"], p["mask"], p["qvec"], p["tvec"], p["flags"])


def batch(problems):
    """The arrays of Context.refine_absolute_poses for a list of problems."""
    offs = np.concatenate([[0], np.cumsum([len(p["xy"]) for p in problems])]).astype(np.uint64)
    cat = lambda key, w, dt: np.concatenate([np.asarray(p[key], dt).reshape(-1, w) for p in problems] + [np.zeros((0, w), dt)])
    return dict(cameras=[p["cam"] for p in problems], offsets=offs, points2D=cat("xy", 2, np.float64), points3D=cat("X", 3, np.float64),
                inlier_mask=cat("mask", 1, np.uint8).reshape(-1), qvecs=[p["qvec"] for p in problems],
                tvecs=[p["tvec"] for p in problems], refine_flags=[p["flags"] for p in problems])


def hand_problems():
    """Small and rank-deficient sets: 0, 1, 2, 3 inliers of an exact registration (pose only), and the planar and the collinear
    set of absolute_pose_scenes with the focal length free.  They must end without a fault: terminate and report."""
    out = {}
    base = problem(7, 40, 0.0, 0.0, 0, 0)
    for n in (0, 1, 2, 3):
        m = np.zeros(40, np.uint8)
        m[:n] = 1
        out["n%d" % n] = dict(base, mask=m)
    hand = scenes.hand_scenes()
    rng = np.random.default_rng(5)
    for k in ("planar", "collinear"):
        cam, xy, X = hand[k]
        q = quat_plus(np.array([1.0, 0.0, 0.0, 0.0]), rng.normal(scale=0.004, size=3))[0]
        t = np.array([0.1, 0.2, 9.0]) + rng.normal(scale=0.03, size=3)
        out[k] = dict(cam=scenes.camera(0, 800.0 * 1.02), xy=xy, X=X, mask=np.ones(len(xy), np.uint8), qvec=q, tvec=t,
                      flags=capi.POSE_REFINE_FOCAL_LENGTH, P=np.concatenate([np.eye(3), [[0.1], [0.2], [9.0]]], axis=1), noise=0.0)
    return out
