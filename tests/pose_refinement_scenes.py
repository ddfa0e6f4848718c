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


# ---- the edge problems (tests/test_pose_refinement_edges_cpu.py, tests/test_pose_refinement_edges_gpu.py) ----
# Far starts: (n, model, flags, rot, trans) of problem(1000 + n, n, 0.2, 0.5, ...) with the focal lengths 10 % off where they are
# free.  The restatement rejects steps on every FAR_CLEAR row (the CPU test holds the step strings); the FAR_UNCLEAR rows are not
# clear in the restatement and are compared by the other rule.
FAR_CLEAR = [(63, 4, 3, 0.3, 1.0), (64, 4, 3, 0.8, 3.0), (65, 2, 3, 0.3, 1.0), (128, 0, 0, 0.8, 3.0), (128, 2, 3, 0.8, 3.0),
             (129, 2, 3, 0.8, 3.0), (129, 4, 3, 0.8, 3.0)]
FAR_UNCLEAR = [(65, 2, 3, 0.8, 3.0), (128, 4, 3, 0.8, 3.0)]  # 50 iterations of r and a interleaved; 100 iterations, NO_CONVERGENCE
LOSS_SCALES = (0.25, 4.0, 100.0)
WAVE_SIZES = (1, 2, 63, 64, 65, 127, 128, 129)
MASK_NAMES = ("lane0", "second_pass", "last", "not_lane63")
MASK_RESIDUAL_BLOCKS = (3, 65, 1, 127)
# AbsolutePoseRefinementOptions::Check accepts it; b = scale^2 = 1e-308 and c = 1 / b = 1e308 are finite, and 1 + |r|^2 c overflows
# for every residual above 1.4 px: an infinite initial cost, FAILURE before the first iteration, whatever the estimate was
FAILING_LOSS_SCALE = 1e-154


def edge_far_starts():
    """[(problem, listed as clear)]: the seven clear rows, then the two that are not."""
    rows = [(r, True) for r in FAR_CLEAR] + [(r, False) for r in FAR_UNCLEAR]
    return [(problem(1000 + n, n, 0.2, 0.5, m, f, focal_error=0.1 if f else 0.0, rot=rot, trans=trans), c) for (n, m, f, rot, trans), c in rows]


def edge_loss_scale_problem():
    return problem(1100, 65, 0.3, 1.0, 2, 3, focal_error=0.02)


def edge_flags2(flags=capi.POSE_REFINE_EXTRA_PARAMS):
    """model -> the problem with the extras alone free (flags 2); flags=0 gives the same problems with the camera constant."""
    return {m: problem(1200 + m, 64, 0.2, 0.5, m, flags) for m in (0, 1, 2, 4, 8)}


def edge_wave_problems():
    """Sixteen problems, every point an inlier: the sizes at the wave's edges pose only (SIMPLE_PINHOLE; N = 1 and 2 are the first
    points of the hand problems' exact registration, so that their measured bound holds: the same data as hand_problems()'s n1 and
    n2 in a segment of that length instead of under a mask), the six sizes from 63 again through OPENCV's projection, and N = 65
    and 129 with SIMPLE_RADIAL's focal length and extra parameter free."""
    def full(seed, n, model, flags, **kw):
        p = problem(seed, n, 0.0, 0.5, model, flags, **kw)
        return dict(p, mask=np.ones(n, np.uint8))
    base = problem(7, 40, 0.0, 0.0, 0, 0)
    out = [dict(base, xy=base["xy"][:n], X=base["X"][:n], mask=np.ones(n, np.uint8)) for n in WAVE_SIZES[:2]]
    out += [full(1400 + n, n, 0, 0) for n in WAVE_SIZES[2:]]
    out += [full(1500 + n, n, 4, 0) for n in WAVE_SIZES[2:]]
    out += [full(1600 + n, n, 2, 3, focal_error=0.02) for n in (65, 129)]
    return out


def edge_masks():
    """The N = 129 pose-only problem of edge_wave_problems under four masks (MASK_NAMES): lane 0 alone holds inliers; every lane's
    first pass is empty; the last point alone; lane 63 holds none."""
    p = edge_wave_problems()[WAVE_SIZES.index(129)]
    i = np.arange(129)
    masks = (i % 64 == 0, i >= 64, i == 128, i % 64 != 63)
    return [dict(p, mask=m.astype(np.uint8)) for m in masks]


def edge_nonfinite_cost():
    """One observation so far away that its squared residual overflows: finite input, infinite initial cost."""
    p = problem(1300, 64, 0.0, 0.5, 0, 0)
    xy = np.array(p["xy"], np.float64)
    xy[0] = [1e200, 0.0]
    return dict(p, xy=xy, mask=np.ones(64, np.uint8))


def edge_invalid_steps(focal=1e155, flags=0):
    """70 points on the optical axis seen one pixel beside the principal point, identity pose: at focal 1e155 J'J overflows and
    every pivot of every solve is NaN (five invalid steps, FAILURE); at 1e150 it does not (the control)."""
    cam = scenes.camera(0, focal)
    z = np.linspace(5.0, 9.0, 70)
    X = np.stack([np.zeros(70), np.zeros(70), z], axis=1)
    xy = np.tile([cam.params[1] + 1.0, cam.params[2]], (70, 1))
    return dict(cam=cam, xy=xy, X=X, mask=np.ones(70, np.uint8), qvec=np.array([1.0, 0.0, 0.0, 0.0]), tvec=np.zeros(3), flags=flags,
                P=np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1), noise=0.0)


def edge_quaternion_problem():
    return problem(1301, 64, 0.0, 0.5, 0, 0)


def edge_big_batch(count=300):
    """[(problem, index into edge_wave_problems or -1 for an empty segment, fully masked)]: the sixteen cycled, every seventh an
    empty segment, every eleventh fully masked."""
    wave = edge_wave_problems()
    out = []
    for b in range(count):
        k = b % len(wave)
        p = wave[k]
        if b % 7 == 6:
            out.append((dict(p, xy=np.zeros((0, 2)), X=np.zeros((0, 3)), mask=np.zeros(0, np.uint8)), -1, False))
        elif b % 11 == 10:
            out.append((dict(p, mask=np.zeros(len(p["xy"]), np.uint8)), k, True))
        else:
            out.append((p, k, False))
    return out


def edge_registrations():
    """Three registrations for Context.register_images (2 px noise, so that every image has residuals above 1.4 px):
    (cameras, offsets, points2D, points3D)."""
    regs = [scenes.registration(1350 + i, 80, 0.2, 2.0, m) for i, m in enumerate((0, 2, 0))]
    offs = np.concatenate([[0], np.cumsum([len(r[1]) for r in regs])]).astype(np.uint64)
    return [r[0] for r in regs], offs, np.concatenate([r[1] for r in regs]), np.concatenate([r[2] for r in regs])


def edge_accepted_then_invalid():
    """(problem, options): the pose-only far start of 128 points with its pixels (focal length, principal point, observations)
    and the loss scale multiplied by 2^501.  A power of two scales the run exactly until something overflows: the Jacobian's
    columns grow as the residuals fall and rho' rises towards 1, and after the seventh accepted step J'J overflows (its largest
    diagonal entry is 0.53 of DBL_MAX one step earlier and 2.3 times DBL_MAX here, so rounding does not decide it).  Steps
    a r r a a a a a a i i i i i: FAILURE with seven successful steps behind it, the result the last accepted state."""
    p = problem(1128, 128, 0.2, 0.5, 0, 0, rot=0.8, trans=3.0)
    K = 2.0 ** 501
    cam = capi.Camera.from_buffer_copy(bytes(p["cam"]))
    for j in range(3):
        cam.params[j] *= K
    return dict(p, cam=cam, xy=np.asarray(p["xy"], np.float64) * K), dict(loss_function_scale=K)
