"""CPU-only: the restatement of dsm_adjust_local_bundles (tests/local_bundle_ref.py) against scipy, planted
scenes, the corrector's branch, the explicit reduced system against a dense solve, capi.local_bundle_problem against hand-built
expectations, the option defaults, and the restatement's verdict on every comparison the GPU file makes."""
import functools

import numpy as np
import pytest

from tests import local_bundle_ref as ref
from tests import local_bundle_scenes as scenes
from tests.bundle_adjustment_ref import make_scene, quat_plus

# Every input of a clear comparison moved by one ulp (seeded directions) changes the cost trace and the parameter blocks by at
# most 1.10e-10 relative with no decision flipped (re-measured below; the worst is shared_FULL_OPENCV, twelve parameters of
# one camera of which ten are free over six images; the median is 2e-14); held with a small head-room:
ULP_SENSITIVITY = 1.2e-10
# times 16 for what the restatement does not pin (libm's log / sin / cos, the dual numbers' order): the GPU file's tolerance
CLEAR_TOLERANCE = 16 * ULP_SENSITIVITY
# A comparison that is not clear (points1, loss_trivial; 39 of the 41 are clear): one ulp moves its final cost by at most 6.9e-16 of its initial cost;
# held to 8e-16, times 16
UNCLEAR_COST_SENSITIVITY = 8e-16
UNCLEAR_COST_TOLERANCE = 16 * UNCLEAR_COST_SENSITIVITY
FLOAT_KEYS = ("camera_params", "qvec", "tvec", "xyz", "obs_xy")


def one_ulp(scene, seed):
    rng = np.random.default_rng(seed)
    out = dict(scene)
    for k in FLOAT_KEYS:
        a = np.asarray(scene[k], np.float64)
        out[k] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return out


def rel_change(a, b):
    """The largest relative change of the cost trace and of the parameter blocks (a block's change over its largest entry)."""
    m = float(np.max(np.abs(a["trace"][:, 0] - b["trace"][:, 0]) / np.maximum(np.abs(a["trace"][:, 0]), 1e-300)))
    for k in ("camera_params", "qvec", "tvec", "xyz"):
        x, y = np.asarray(a[k], np.float64), np.asarray(b[k], np.float64)
        if x.size:
            m = max(m, float(np.max(np.abs(x - y)) / max(np.max(np.abs(x)), 1e-300)))
    return m


@functools.lru_cache(maxsize=None)
def verdicts():
    out = {}
    for name, sc, opt in scenes.comparisons():
        run = ref.adjust_local_bundle(sc, opt)
        out[name] = (run, ref.is_clear(sc, opt, run))
    return out


def test_option_defaults_match_the_reference():
    # src/controllers/incremental_mapper_controller.cc:234-255 and incremental_mapper_controller.h:90-98
    import os
    import re
    d = ref.DEFAULTS
    assert (d["max_num_iterations"], d["gradient_tolerance"], d["function_tolerance"], d["parameter_tolerance"]) == (25, 10.0, 0.0, 0.0)
    assert (d["refine_focal_length"], d["refine_principal_point"], d["refine_extra_params"]) == (1, 0, 1)
    assert (d["loss_function_type"], d["loss_function_scale"], d["max_num_consecutive_invalid_steps"]) == (ref.LOSS_SOFT_L1, 1.0, 10)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "dagsfm_amd", "csrc", "local_bundle.hip")).read()
    body = src[src.index('void dsm_default_local_bundle_options'):]
    body = body[:body.index("}")]
    got = dict(re.findall(r"o->(\w+) = ([\w.]+);", body))
    want = {k: v for k, v in d.items()}
    want["loss_function_type"] = "DSM_LOSS_SOFT_L1"
    assert set(got) == set(want)
    for k, v in want.items():
        assert got[k] == v or float(got[k]) == float(v), k


def test_corrector_takes_its_first_branch_for_both_losses():
    s = np.concatenate([[0.0], np.logspace(-12, 12, 200)])
    for kind in (ref.LOSS_SOFT_L1, ref.LOSS_CAUCHY):
        for scale in (0.1, 1.0, 7.0):
            rho, r1, r2 = ref.loss(kind, scale, s)
            assert (r2 < 0).all() and (r1 > 0).all()
            sq, scaling, asn, branch = ref.corrector(s, r1, r2)
            assert (branch == 1).all() and (asn == 0).all() and np.array_equal(scaling, sq)
    # the second branch exists: a loss with rho'' > 0 leaves the first
    assert ref.corrector(np.array([2.0]), np.array([1.0]), np.array([0.1]))[3][0] == 2
    # the losses themselves: rho(0) = 0, rho'(0) = 1, SoftLOne ~ 2 sqrt(s), Cauchy ~ log
    for kind in (ref.LOSS_SOFT_L1, ref.LOSS_CAUCHY):
        rho, r1, _ = ref.loss(kind, 1.0, np.array([0.0, 1e12]))
        assert rho[0] == 0.0 and r1[0] == 1.0
    assert abs(ref.loss(ref.LOSS_SOFT_L1, 1.0, np.array([1e12]))[0][0] / 2e6 - 1) < 1e-5
    assert abs(ref.loss(ref.LOSS_CAUCHY, 2.0, np.array([3.0]))[0][0] - 4 * np.log(1.75)) < 1e-15


def test_block_sum_is_the_stated_tree():
    rng = np.random.default_rng(0)
    for n in (0, 1, 255, 256, 257, 1000):
        v = rng.standard_normal(n)
        acc = [0.0] * 256
        for i, x in enumerate(v):
            acc[i % 256] += x
        for o in (32, 16, 8, 4, 2, 1):
            acc = [acc[i] + acc[i ^ o] for i in range(256)]
        assert ref.block_sum(v) == ((acc[0] + acc[64]) + acc[128]) + acc[192]


@pytest.mark.parametrize("kind,name", [(ref.LOSS_SOFT_L1, "soft_l1"), (ref.LOSS_CAUCHY, "cauchy"), (ref.LOSS_TRIVIAL, "linear")])
def test_restatement_reaches_scipys_optimum(kind, name):
    """One scalar |r_i| per observation, so that scipy's per-residual loss is Ceres' per-block loss: scipy's rho(z),
    z = (f / f_scale)^2, is 2 (sqrt(1 + z) - 1) / log(1 + z) / z, times f_scale^2 in its cost -- Ceres' with b = scale^2.
    scipy is asked twice, to tolerances of 1e-15: from the same perturbed start, and from the restatement's own result (a
    descent direction the restatement missed would show there).  Its Jacobian is analytic: d|r_i| = r_i' J_i / |r_i| with J_i
    the restatement's tangent Jacobian at the current point; for a qvec that tangent differs from the derivative with respect
    to scipy's variable by an invertible 3 x 3 map, which moves no stationary point.  The scene has 240 scalar residuals for
    49 unknowns (most points constant): with |r_i| as the residual the Gauss-Newton model is rank one per observation, and
    scipy crawls on scenes where that leaves it close to singular.

    Bound.  The restatement stops when |x - Plus(x, -g)|inf <= gtol, which is |g|inf for the Euclidean blocks and |g| (1 + O(g^2))
    for a qvec; so |g|_2 <= sqrt(dim) gtol.  Near a minimum cost - cost* <= |g|_2^2 / (2 lambda_min(H)); H is taken as J'J of
    the unscaled corrected Jacobian at the restatement's last linearisation (lambda_min computed here, asserted positive) with a
    factor 2 for the second-order terms Gauss-Newton leaves out.  Both costs are sums of n doubles: 2 n eps each.  As in
    DESIGN.md 15 the assertion is one-sided: a minimiser's result does not bound the minimum from below."""
    from scipy.optimize import least_squares
    scale, gtol = 1.5, 1e-7
    sc = scenes.local_scene(7, 4, 2, n_points=40, noise=0.7, arc=1.2, min_track=6, const_point_frac=0.7)
    opt = dict(loss_function_type=kind, loss_function_scale=scale, gradient_tolerance=gtol, max_num_iterations=200)
    dense = []
    out = ref.adjust_local_bundle(sc, opt, dense_check=dense)
    got = out["result"]["final_cost"]
    assert out["result"]["termination"] == ref.CONVERGENCE and out["result"]["num_successful_steps"] >= 3
    lam = np.linalg.eigvalsh(dense[-1][3]).min()
    dim, n = dense[-1][3].shape[0], len(sc["obs_image"])
    assert lam > 0.0
    bound = 2.0 * dim * gtol * gtol / (2.0 * lam) + 4.0 * n * np.finfo(float).eps * got

    def optimum(start):
        pb = ref.LocalProblem(start, dict(ref.DEFAULTS, **opt))
        q = np.asarray(start["qvec"], np.float64)
        st = {"qvec": q / np.linalg.norm(q, axis=1, keepdims=True), "tvec": np.asarray(start["tvec"], np.float64),
              "xyz": np.asarray(start["xyz"], np.float64), "camera_params": np.asarray(start["camera_params"], np.float64)}

        def f(d):
            r = pb.residuals(pb.plus(st, d))
            return np.sqrt((r * r).sum(1))

        def jac(d):
            r, J = pb.residuals(pb.plus(st, d), True)
            J = J.toarray()
            return (r[:, 0:1] * J[0::2] + r[:, 1:2] * J[1::2]) / np.sqrt((r * r).sum(1))[:, None]
        z = (f(np.zeros(pb.ne + pb.nf)) / scale) ** 2
        rho = {"soft_l1": 2.0 * (np.sqrt(1.0 + z) - 1.0), "cauchy": np.log1p(z), "linear": z}[name]
        sol = least_squares(f, np.zeros(pb.ne + pb.nf), jac=jac, method="trf", loss=name, f_scale=scale, x_scale="jac", xtol=1e-15,
                            ftol=1e-15, gtol=1e-10, max_nfev=1000)
        return 0.5 * scale * scale * float(rho.sum()), float(sol.cost)
    cost_at_start, from_start = optimum(sc)
    assert abs(cost_at_start - out["result"]["initial_cost"]) <= 4.0 * n * np.finfo(float).eps * cost_at_start  # the same function
    end = dict(sc, qvec=out["qvec"], tvec=out["tvec"], xyz=out["xyz"], camera_params=out["camera_params"])
    cost_at_end, from_result = optimum(end)
    assert abs(cost_at_end - got) <= 4.0 * n * np.finfo(float).eps * got
    print(name, got, from_start, from_result, bound)
    assert got <= from_start + bound and got <= from_result + bound
    assert from_start <= got * (1.0 + 1e-6)  # and scipy did arrive: not a vacuous run that stopped far above


def test_planted_parameters_are_recovered_on_exact_scenes():
    """Exact observations, the constant blocks at their planted values, the variable ones moved: every loss must bring them back
    (the constant pose, the constant tvec[0] and the outside images fix the gauge)."""
    truth = scenes.local_scene(3, 4, 2, n_points=40, noise=0.0)
    exact = make_scene(3, n_images=6, n_points=40, noise=0.0, perturb=0.0, gauge=False)
    for k in ("qvec", "tvec", "xyz", "camera_params"):
        truth[k] = exact[k]
    rng = np.random.default_rng(0)
    moved = dict(truth, qvec=truth["qvec"].copy(), tvec=truth["tvec"].copy())
    moved["qvec"][:3] = quat_plus(truth["qvec"][:3], rng.normal(scale=0.002, size=(3, 3)))
    moved["tvec"][:3] += rng.normal(scale=0.02, size=(3, 3))
    moved["tvec"][2, 0] = truth["tvec"][2, 0]
    moved["xyz"] = truth["xyz"] + rng.normal(scale=0.02, size=truth["xyz"].shape)
    moved["camera_params"] = truth["camera_params"] * np.array([1.01, 1.0, 1.0, 1.0])
    for kind in (ref.LOSS_TRIVIAL, ref.LOSS_SOFT_L1, ref.LOSS_CAUCHY):
        out = ref.adjust_local_bundle(moved, dict(loss_function_type=kind, gradient_tolerance=1e-10, max_num_iterations=60))
        assert out["result"]["final_cost"] < 1e-12 * out["result"]["initial_cost"], kind
        assert np.max(np.abs(out["xyz"] - truth["xyz"])) < 1e-6 and np.max(np.abs(out["tvec"] - truth["tvec"])) < 1e-6
        assert abs(out["camera_params"][0] / truth["camera_params"][0] - 1.0) < 1e-7


def test_explicit_reduced_system_equals_the_dense_solve():
    """Eliminating the points and solving S is algebraically the full damped normal equations.  The bound is the dense
    solve's conditioning: cond(A) eps times a small factor for the two factorisations."""
    for name, sc, opt in scenes.comparisons()[:6]:
        dense = []
        ref.adjust_local_bundle(sc, opt, dense_check=dense)
        assert dense
        for A, b, step, _ in dense:
            x = np.linalg.solve(A, b)
            bound = 64 * np.linalg.cond(A) * np.finfo(float).eps
            assert np.max(np.abs(x - step)) <= bound * np.max(np.abs(x)), (name, np.max(np.abs(x - step)) / np.max(np.abs(x)), bound)


def _recon():
    """A reconstruction of 6 images and 3 cameras: images 0-3 share camera 0, image 4 has camera 1, image 5 camera 2."""
    s = make_scene(1, n_images=6, n_points=12, models=(2, 0, 3), shared=True, gauge=False, min_track=2)
    s["image_camera"] = np.array([0, 0, 0, 0, 1, 2], np.uint32)
    tracks = [[0, 1], [0, 1, 2], [1, 2], [0, 3], [0, 4], [1, 5], [2, 3, 4], [3, 4, 5], [0, 1, 2, 3], [4, 5], [0, 5], [1, 2, 3]]
    s["track_offsets"] = np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32)
    s["obs_image"] = np.array([i for t in tracks for i in t], np.uint32)
    s["obs_xy"] = np.arange(2.0 * len(s["obs_image"])).reshape(-1, 2)
    s["point_ids"] = np.arange(12, dtype=np.uint64) + 100
    return s, tracks


def test_local_bundle_problem_against_hand_built_expectations():
    from dagsfm_amd import capi
    s, tracks = _recon()
    assert capi.local_bundle_problem(s, 0, [], []) is None
    # one neighbour: its pose constant, tvec[0] of the new image constant
    p = capi.local_bundle_problem(s, 0, [1], [4, 10])
    img = list(p["image_index"])
    assert img[:2] == [0, 1] and sorted(img[2:]) == [4, 5]  # the outside images of the variable points 4 and 10
    assert list(p["image_constant_pose"]) == [0, 1, 1, 1] and list(p["image_constant_tvec"]) == [1, 0, 0, 0]
    # points seen from image 0 or 1: 0 1 2 3 4 5 8 10 11
    assert list(p["point_index"]) == [0, 1, 2, 3, 4, 5, 8, 10, 11] and list(p["point_ids"]) == [100, 101, 102, 103, 104, 105, 108, 110, 111]
    # point 0 ({0, 1}) is fully inside and not variable: it stays variable; 1 ({0, 1, 2}) is cut: constant; 4 and 10 are variable
    assert list(p["point_constant"]) == [0, 1, 1, 1, 0, 1, 1, 0, 1]
    assert list(np.diff(p["track_offsets"])) == [2, 2, 1, 1, 2, 1, 2, 2, 1]  # track lengths of 1 are part of the problem
    # cameras: 0 (config), 1 and 2 (outside, unshared: constant)
    assert list(p["camera_index"]) == [0, 1, 2] and list(p["camera_constant"]) == [0, 1, 1]
    k = int(p["track_offsets"][4])
    assert list(p["image_index"][p["obs_image"][k:k + 2]]) == [0, 4]
    assert np.array_equal(p["obs_xy"][k], s["obs_xy"][int(s["track_offsets"][4])])
    # many neighbours: the last one constant, tvec[0] of the one before it
    p = capi.local_bundle_problem(s, 0, [1, 2, 3], [3])
    assert list(p["image_index"]) == [0, 1, 2, 3] and list(p["image_constant_pose"]) == [0, 0, 0, 1]
    assert list(p["image_constant_tvec"]) == [0, 0, 1, 0] and list(p["camera_constant"]) == [0]
    # fixed_image_ids: a fixed neighbour is constant-pose; when it is the one before the last, no tvec component is fixed
    p = capi.local_bundle_problem(s, 0, [1, 2, 3], [3], fixed_image_ids=[2])
    assert list(p["image_constant_pose"]) == [0, 0, 1, 1] and list(p["image_constant_tvec"]) == [0, 0, 0, 0]
    p = capi.local_bundle_problem(s, 0, [1, 2, 3], [3], fixed_image_ids=[1])
    assert list(p["image_constant_pose"]) == [0, 1, 0, 1] and list(p["image_constant_tvec"]) == [0, 0, 1, 0]
    # a shared outside camera: point 3 ({0, 3}) variable brings image 3, whose camera 0 a config image shares: not constant
    p = capi.local_bundle_problem(s, 0, [1], [3])
    assert list(p["image_index"]) == [0, 1, 3] and list(p["camera_index"]) == [0] and list(p["camera_constant"]) == [0]
    assert list(p["image_constant_pose"]) == [0, 1, 1]
    # the restatement accepts what the helper builds
    out = ref.adjust_local_bundle(capi.local_bundle_problem(s, 0, [1, 2], [0, 1, 2, 3, 4, 8, 10]), dict(max_num_iterations=2))
    assert out["result"]["solved"] == 1 and out["result"]["num_residuals"] > 0


def test_special_problems():
    sc = scenes.local_scene(4, 3, 0, n_points=10)
    empty = dict(sc, track_offsets=np.zeros(11, np.uint32), obs_image=np.zeros(0, np.uint32), obs_xy=np.zeros((0, 2)))
    out = ref.adjust_local_bundle(empty)
    assert out["result"]["solved"] == 0 and out["result"]["num_iterations"] == 0 and np.array_equal(out["qvec"], sc["qvec"])
    const = dict(sc, image_constant_pose=np.ones(3, np.uint8), point_constant=np.ones(10, np.uint8), camera_constant=np.ones(1, np.uint8))
    out = ref.adjust_local_bundle(const)
    assert out["result"]["solved"] == 1 and out["result"]["termination"] == ref.CONVERGENCE and out["result"]["num_iterations"] == 0
    assert out["result"]["final_cost"] == out["result"]["initial_cost"] > 0
    for k in ("qvec", "tvec", "xyz", "camera_params"):
        assert np.array_equal(out[k], np.asarray(sc[k], np.float64).reshape(out[k].shape)), k
    with pytest.raises(ValueError):
        ref.adjust_local_bundle(scenes.reduced_dim_scene(True), scenes.REDUCED_DIM_OPTIONS)
    assert ref.adjust_local_bundle(scenes.reduced_dim_scene(False), dict(scenes.REDUCED_DIM_OPTIONS, max_num_iterations=0))["result"]["reduced_dim"] == 128


def test_result_does_not_depend_on_the_order_of_the_blocks():
    name, sc, opt = scenes.comparisons()[3]
    a = ref.adjust_local_bundle(sc, opt)
    rng = np.random.default_rng(1)
    N, P = len(sc["image_camera"]), len(sc["point_ids"])
    ip, pp = rng.permutation(N), rng.permutation(P)
    toff = np.asarray(sc["track_offsets"], np.int64)
    tracks = [rng.permutation(np.arange(toff[p], toff[p + 1])) for p in pp]
    inv = np.empty(N, np.int64)
    inv[ip] = np.arange(N)
    sh = dict(sc, image_camera=sc["image_camera"][ip], qvec=sc["qvec"][ip], tvec=sc["tvec"][ip], image_constant_pose=sc["image_constant_pose"][ip],
              image_constant_tvec=sc["image_constant_tvec"][ip], point_ids=sc["point_ids"][pp], xyz=sc["xyz"][pp], point_constant=sc["point_constant"][pp],
              track_offsets=np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32),
              obs_image=inv[sc["obs_image"][np.concatenate(tracks)]].astype(np.uint32), obs_xy=sc["obs_xy"][np.concatenate(tracks)])
    b = ref.adjust_local_bundle(sh, opt)
    assert a["trace"].tobytes() == b["trace"].tobytes()
    assert np.array_equal(a["qvec"][ip], b["qvec"]) and np.array_equal(a["xyz"][pp], b["xyz"]) and np.array_equal(a["camera_params"], b["camera_params"])


def test_at_least_nine_in_ten_comparisons_are_clear():
    """The project's bar: the restatement alone must call at least 90 % of the comparisons clear."""
    v = verdicts()
    unclear = [n for n, (_, c) in v.items() if not c]
    print("not clear:", unclear)
    assert len(unclear) <= len(v) // 10, unclear
    for name, (run, _) in v.items():
        assert run["result"]["num_iterations"] >= 1 and run["result"]["num_successful_steps"] >= 1, name


def test_one_ulp_sensitivity_stays_within_the_measured_constants():
    worst_clear = worst_unclear = 0.0
    for name, sc, opt in scenes.comparisons():
        a, clear = verdicts()[name]
        b = ref.adjust_local_bundle(one_ulp(sc, 1), opt)
        if clear:
            assert a["steps"] == b["steps"] and a["result"]["termination"] == b["result"]["termination"], name
            worst_clear = max(worst_clear, rel_change(a, b))
        else:
            assert a["result"]["termination"] == b["result"]["termination"], name
            worst_unclear = max(worst_unclear, abs(a["result"]["final_cost"] - b["result"]["final_cost"]) / a["result"]["initial_cost"])
    print("one ulp: clear %.3e (held %.1e), not clear final / initial cost %.3e (held %.1e)"
          % (worst_clear, ULP_SENSITIVITY, worst_unclear, UNCLEAR_COST_SENSITIVITY))
    assert worst_clear <= ULP_SENSITIVITY and worst_unclear <= UNCLEAR_COST_SENSITIVITY
