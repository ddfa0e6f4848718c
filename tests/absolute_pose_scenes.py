"""Scenes of the absolute pose tests (tests/test_absolute_pose_cpu.py, tests/test_absolute_pose_gpu.py): the reference's own
known-answer scene restated as data, hand scenes, and the seeded synthetic registrations.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from dagsfm_amd import capi, synthetic

# src/estimators/absolute_pose_test.cc:49-57 (the eight points of TestP3P / TestEPNP), :64-67 the planted transforms
KNOWN_POINTS3D = np.array([[1, 1, 1], [0, 1, 1], [3, 1.0, 4], [3, 1.1, 4], [3, 1.2, 4], [3, 1.3, 4], [3, 1.4, 4], [2, 1, 7]], np.float64)
KNOWN_QX = (0.0, 0.2, 0.4, 0.6000000000000001, 0.8)
KNOWN_TX = tuple(np.cumsum([0.0] + [0.1] * 9).tolist())


# The tolerance of the GPU comparison on model / qvec / tvec (DESIGN.md 14 "Parity"), measured on the restatement, never on the device:
# every input of every clear grid problem moved by one ulp in a seeded random direction (ulp_perturbed below) changes them by at most
# MEASURED_ULP_SENSITIVITY of the largest entry (3.82e-11 observed; tests/test_absolute_pose_cpu.py re-measures it and holds it to the
# constant), times 16 for the device's different but equally valid operation order in the parts the oracle blocks do not pin.
MEASURED_ULP_SENSITIVITY = 3.9e-11
POSE_TOLERANCE = 16 * MEASURED_ULP_SENSITIVITY


def ulp_perturbed(rng, a):
    """Every entry of a moved to its neighbouring double, up or down at random."""
    up = rng.integers(0, 2, a.shape) > 0
    return np.where(up, np.nextafter(a, np.inf), np.nextafter(a, -np.inf))


def quat_to_rot(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def known_scene(qx, tx):
    """The planted 3 x 4 transform and the exact normalised image points of the eight points."""
    P = np.concatenate([quat_to_rot([1, qx, 0, 0]), [[tx], [0.0], [0.0]]], axis=1)
    pc = KNOWN_POINTS3D @ P[:, :3].T + P[:, 3]
    return P, pc[:, :2] / pc[:, 2:3]


# mild distortion for every camera model (ids 0 .. 10); focal lengths are filled in by camera()
_EXTRA = {0: [], 1: [], 2: [0.02], 3: [0.02, -0.01], 4: [0.02, -0.01, 0.001, -0.001], 5: [0.01, -0.005, 0.002, -0.001],
          6: [0.02, -0.01, 0.001, -0.001, 0.003, 0.01, -0.004, 0.001], 7: [0.3], 8: [0.02], 9: [0.02, -0.01],
          10: [0.01, -0.005, 0.001, -0.001, 0.002, -0.001, 0.0005, -0.0005]}


def camera(model_id=0, focal=800.0, width=1000, height=750, prior=True):
    c = capi.Camera(model_id=model_id, has_prior_focal_length=int(prior), width=width, height=height)
    two = model_id in (1, 4, 5, 6, 7, 10)
    p = ([focal, focal * 1.01] if two else [focal]) + [width / 2.0, height / 2.0] + _EXTRA[model_id]
    for i, v in enumerate(p):
        c.params[i] = v
    return c


def registration(seed, n=200, outliers=0.3, noise=0.5, model_id=0, focal=800.0, prior_focal=None):
    """A seeded synthetic registration: n world points in front of a random camera, projected through the camera model, pixel noise,
    a share of outliers (uniform pixels).  prior_focal: the focal length the returned camera claims (a wrong prior).
    Returns (camera, points2D [n, 2], points3D [n, 3], planted 3 x 4)."""
    rng = np.random.default_rng([seed, 0xAB5])
    q = rng.normal(size=4)
    R = quat_to_rot(q)
    X = rng.uniform(-3.0, 3.0, (n, 3))
    t = np.array([rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), 8.0 + rng.uniform(0, 4)]) - R @ X.mean(axis=0)
    pc = X @ R.T + t  # the scene's centre sits 8 .. 12 in front of the camera
    true_cam = camera(model_id, focal)
    u, v = synthetic.world_to_image(model_id, list(true_cam.params)[:capi.CAMERA_MODEL_NUM_PARAMS[model_id]], pc[:, 0] / pc[:, 2],
                                    pc[:, 1] / pc[:, 2])
    xy = np.stack([u, v], axis=1) + rng.normal(scale=noise, size=(n, 2)) if noise > 0 else np.stack([u, v], axis=1)
    bad = rng.permutation(n)[:int(round(outliers * n))]
    xy[bad] = rng.uniform([0, 0], [1000, 750], (len(bad), 2))
    cam = camera(model_id, prior_focal if prior_focal is not None else focal, prior=prior_focal is None)
    return cam, xy, X, np.concatenate([R, t[:, None]], axis=1)


# the random grid the comparison rule and the clear-share cap are applied to: (seed, n, outlier share, pixel noise, model, sweep)
RANDOM_GRID = [(100 + i, n, o, s, m, False)
               for i, (n, o, s, m) in enumerate([
                   (30, 0.0, 0.5, 0), (30, 0.3, 0.5, 1), (60, 0.5, 1.0, 2), (60, 0.7, 0.5, 3), (120, 0.0, 0.0, 4), (120, 0.3, 1.0, 5),
                   (200, 0.5, 0.5, 6), (200, 0.7, 1.0, 7), (400, 0.1, 0.5, 8), (400, 0.3, 2.0, 9), (800, 0.5, 0.5, 10),
                   (800, 0.2, 1.0, 0), (1500, 0.3, 0.5, 2), (1500, 0.6, 1.0, 0), (3000, 0.3, 0.5, 0), (3000, 0.5, 1.0, 4),
                   (100, 0.3, 0.5, 0), (100, 0.3, 0.5, 1), (250, 0.4, 0.7, 3), (500, 0.2, 0.3, 6)])]
# focal sweeps (31 runs each): a right prior and a wrong prior that only the sweep recovers
SWEEP_GRID = [(300, 60, 0.2, 0.5, 0, True, None), (301, 80, 0.3, 0.5, 1, True, 2400.0)]


def grid_problem(entry):
    seed, n, o, s, m, sweep = entry[:6]
    prior = entry[6] if len(entry) > 6 else None
    cam, xy, X, P = registration(seed, n, o, s, m, prior_focal=prior)
    return dict(cam=cam, xy=xy, X=X, P=P, sweep=sweep)


def hand_scenes():
    """Exact data: N = 0, 2, 3, 4, 5; all points behind the camera; a planar and a collinear set; duplicated points."""
    cam = camera(0)
    out = {}
    _, xy, X, P = registration(7, 40, 0.0, 0.0, 0)
    for n in (0, 2, 3, 4, 5):
        out["n%d" % n] = (cam, xy[:n], X[:n])
    pc = X @ P[:, :3].T + P[:, 3]
    Rflip = np.diag([1.0, -1.0, -1.0])  # the same image points, the scene behind the planted camera (another pose may still fit a few)
    out["behind"] = (cam, xy, (np.linalg.inv(P[:, :3]) @ (Rflip @ (-(pc.T)) - P[:, 3:4])).T)
    rng = np.random.default_rng(11)
    Xp = np.concatenate([rng.uniform(-3, 3, (40, 2)), np.zeros((40, 1))], axis=1)  # an exact plane: EPnP's rank test fires
    Pp = np.concatenate([np.eye(3), [[0.1], [0.2], [9.0]]], axis=1)
    pcp = Xp @ Pp[:, :3].T + Pp[:, 3]
    out["planar"] = (cam, np.stack([800 * pcp[:, 0] / pcp[:, 2] + 500, 800 * pcp[:, 1] / pcp[:, 2] + 375], axis=1), Xp)
    Xl = np.stack([np.linspace(-3, 3, 20), np.zeros(20), np.zeros(20)], axis=1)
    pcl = Xl @ Pp[:, :3].T + Pp[:, 3]
    out["collinear"] = (cam, np.stack([800 * pcl[:, 0] / pcl[:, 2] + 500, 800 * pcl[:, 1] / pcl[:, 2] + 375], axis=1), Xl)
    out["duplicated"] = (cam, np.concatenate([xy[:10]] * 3), np.concatenate([X[:10]] * 3))
    return out


# ------------------------------------------------------------------------------------------------ the edge scenes
# (tests/test_absolute_pose_edges_cpu.py, tests/test_absolute_pose_edges_gpu.py).  The sizes sit at and beside the multiples of 64
# (the wave's stride over a run's points) and of 256 (the prepare and mask kernels' tile); the outlier shares put the inlier counts
# on both sides of 64 and 128 as well; models 1 and 4 have two focal lengths.  N = 6 and 7 carry no outlier: EPnP over fewer than six
# inliers leaves M^T M rank-deficient (2 n < 12), the null-space basis its SVD returns is decided by rounding and no margin records
# it (with five inliers of seven, one ulp on the inputs flipped model_is_local on a problem every margin called clear); and with six
# of seven the 210 ordered samples repeat within 30 trials, so the best P3P model ties with itself exactly.
# (seed, n, outlier share, pixel noise, model, sweep)
EDGE_GRID = [(900 + i, n, o, s, m, False)
             for i, (n, o, s, m) in enumerate([
                 (6, 0.0, 0.3, 0), (7, 0.0, 0.5, 1), (63, 0.0, 0.5, 2), (64, 0.2, 0.5, 0), (65, 0.0, 0.5, 4), (127, 0.5, 0.5, 0),
                 (128, 0.0, 0.3, 1), (129, 0.5, 0.5, 3), (255, 0.5, 0.5, 4), (256, 0.5, 1.0, 0), (257, 0.5, 0.5, 1), (511, 0.3, 0.5, 8),
                 (513, 0.1, 0.5, 0), (1025, 0.4, 0.5, 4), (128, 0.5, 0.5, 0), (130, 0.5, 0.5, 6), (65, 0.3, 0.5, 1), (256, 0.0, 0.5, 2)])]


def edge_seeds(case, num_factors=31):
    """The explicit run seeds of edge case number `case`: both sides of a comparison get these, so a case keeps its streams
    wherever it sits in a batch."""
    return np.array([(0x9E3779B1 * (case + 1) + 0x85EBCA6B * s) & 0xFFFFFFFF for s in range(num_factors)], np.uint32)


def placed_inliers(seed, n, inliers, noise=0.3, model_id=0):
    """A registration whose inliers are exactly the points listed: every other point is a uniform pixel."""
    cam, xy, X, P = registration(seed, n, 0.0, noise, model_id)
    rng = np.random.default_rng([seed, 0xED6E])
    bad = np.ones(n, bool)
    bad[np.asarray(inliers, np.int64)] = False
    xy[bad] = rng.uniform([0, 0], [1000, 750], (int(bad.sum()), 2))
    return cam, xy, X, P


LAST_STRIDE_INLIERS = (0, 1, 2, 3, 128, 129)  # lanes 0 and 1 hold two of them each: one on the last, partial stride of 130
EDGE_SEED0 = {"one_lane_found": 1118, "last_stride": 27}  # searched, see edge_cases()
TIE_SCENE = (950, 40, 0.0, 0.1, 0)  # registration()'s arguments
TIE_OPTIONS = dict(num_focal_length_samples=12, min_focal_length_ratio=0.8, max_focal_length_ratio=1.25)


def _case(reg, sweep=False, seed0=None, **opts):
    cam, xy, X, P = reg
    return dict(cam=cam, xy=xy, X=X, P=P, sweep=sweep, opts=opts, seed0=seed0)


def edge_cases():
    """The named edge problems, in a fixed order: name -> dict(cam, xy, X, P, sweep, opts, seeds).  opts holds the options that
    differ from the defaults (for capi.default_absolute_pose_options and for the restatement's opts=); seeds the explicit run
    seeds, one per focal-length factor of those options.  What was searched, always on the restatement alone:
    - seed0=True: the first run's seed (EDGE_SEED0), until the sampler draws three of the planted inliers in one trial;
    - factors_1024: the scene's seed and max_error, until none of its 1024 runs holds a near-tie;
    - max_error_100, sweep_2 and the third of BATCH_FIVE: the scene's seed.  The first choices were clear but ended on a P3P model
      that moves by 3e-10 .. 1e-9 under one ulp on the inputs, more than MEASURED_ULP_SENSITIVITY allows; with these the edge
      problems stay within it and the edge GPU tests use POSE_TOLERANCE unchanged."""
    lane5 = np.arange(5, 640, 64)
    c = {}
    # where the inliers sit among the 64 lanes
    c["one_lane"] = _case(placed_inliers(960, 640, lane5, 0.3))
    c["one_lane_found"] = _case(placed_inliers(960, 640, lane5, 0.3), seed0=True)
    c["first_late"] = _case(placed_inliers(961, 200, np.arange(130, 200), 0.3))
    c["first_63"] = _case(placed_inliers(962, 100, np.arange(63, 100), 0.3))
    c["first_64"] = _case(placed_inliers(963, 100, np.arange(64, 100), 0.3))
    c["last_stride"] = _case(placed_inliers(964, 130, LAST_STRIDE_INLIERS, 0.3), seed0=True)
    c["all_64"] = _case(registration(965, 64, 0.0, 0.3, 0))
    c["all_65"] = _case(registration(966, 65, 0.0, 0.3, 1))
    # options
    c["max_error_1"] = _case(registration(970, 100, 0.3, 0.5, 0), max_error=1.0)
    c["max_error_100"] = _case(registration(1972, 100, 0.3, 0.5, 0), max_error=100.0)
    c["confidence_half"] = _case(registration(970, 100, 0.3, 0.5, 0), confidence=0.5)
    c["confidence_six_nines"] = _case(registration(970, 100, 0.3, 0.5, 0), confidence=0.999999)
    c["cap_5"] = _case(registration(971, 100, 0.5, 0.5, 1), max_num_trials=5, min_num_trials=0)
    c["earliest_abort"] = _case(registration(972, 50, 0.0, 0.3, 0), min_num_trials=0)
    c["min_1000"] = _case(registration(973, 60, 0.2, 0.5, 0), min_num_trials=1000)
    c["no_trials"] = _case(registration(970, 100, 0.3, 0.5, 0), confidence=0.0, min_num_trials=0)
    c["sweep_1"] = _case(registration(974, 60, 0.2, 0.5, 0, prior_focal=1600.0), True, num_focal_length_samples=1,
                         min_focal_length_ratio=0.5, max_focal_length_ratio=2.0)
    c["sweep_2"] = _case(registration(1976, 60, 0.2, 0.5, 0, prior_focal=800.0 / 0.875), True, num_focal_length_samples=2,
                         min_focal_length_ratio=0.5, max_focal_length_ratio=2.0)
    c["sweep_7"] = _case(registration(976, 80, 0.3, 0.5, 4), True, num_focal_length_samples=7,
                         min_focal_length_ratio=0.5, max_focal_length_ratio=2.0)
    # two factors reach the winning inlier count
    c["factor_tie"] = _case(registration(*TIE_SCENE), True, **TIE_OPTIONS)
    # a run that fails with N >= 3: eight correspondences of one world point, P3P finds no model in any trial
    cam, xy, X, P = registration(977, 8, 0.0, 0.0, 0)
    c["same_point"] = _case((cam, xy, np.repeat(X[:1], 8, axis=0), P))
    # the factor limit: 1023 samples give 1024 factors
    # (1024 runs leave 1024 chances of a near-tie: the scene's seed and the tighter max_error were searched until none was left)
    c["factors_1024"] = _case(registration(979, 20, 0.1, 0.3, 0), True, num_focal_length_samples=1023, max_num_trials=4,
                              min_num_trials=0, max_error=1.0)
    for k, (name, p) in enumerate(c.items()):
        p["name"] = name
        p["seeds"] = edge_seeds(100 + k, len(capi.absolute_pose_factors(capi.default_absolute_pose_options(**p["opts"]))))
        if p.pop("seed0") is not None:
            p["seeds"][0] = EDGE_SEED0[name]
    return c


# more than 65535 runs and problems: five small problems repeated, four trials each
BATCH_OPTIONS = dict(max_num_trials=4, min_num_trials=0)
BATCH_FIVE = [(980, 10, 0.2, 0.5, 0), (981, 17, 0.2, 0.5, 1), (1983, 25, 0.2, 0.5, 2), (983, 33, 0.2, 0.5, 0), (984, 40, 0.2, 0.5, 4)]
BATCH_PROBLEMS = 65539       # > 65535 problems: the mask kernel's and the prepare kernel's stride loops
BATCH_SWEEP_PROBLEMS = 2115  # x 31 factors = 65565 runs with 2115 problems: the prepare kernel's stride loop alone


def batch_five(sweep):
    out = []
    for k, (seed, n, o, s, m) in enumerate(BATCH_FIVE):
        cam, xy, X, P = registration(seed, n, o, s, m)
        out.append(dict(cam=cam, xy=xy, X=X, P=P, sweep=sweep, opts=dict(BATCH_OPTIONS), seeds=edge_seeds(200 + k)))
    return out
