"""dsm_adjust_local_bundles on the device against the restatement (tests/local_bundle_ref.py).

Rule of comparison: on a problem the restatement calls clear (every margin >= 1e-9, stable under the conditioning probe) the
termination, the accepted / rejected / invalid sequence and the iteration count are identical, the device's own margins are
>= 1e-9, and costs and parameters agree within CLEAR_TOLERANCE = 16 x the restatement's one-ulp sensitivity (1.2e-10, measured
and held in tests/test_local_bundle_cpu.py) = 1.92e-9.  A problem that is not clear: the same termination, and the final cost
within UNCLEAR_COST_TOLERANCE = 16 x 8e-16 = 1.28e-14 of the initial cost."""
import functools

import numpy as np
import pytest

from tests import local_bundle_ref as ref
from tests import local_bundle_scenes as scenes
from tests.test_local_bundle_cpu import CLEAR_TOLERANCE, UNCLEAR_COST_TOLERANCE, rel_change

pytestmark = pytest.mark.gpu
COMPARISONS = scenes.comparisons()


@pytest.fixture(scope="module")
def ctx():
    from dagsfm_amd import capi
    c = capi.Context(0)
    yield c
    c.close()


def options(opt):
    from dagsfm_amd import capi
    return capi.default_local_bundle_options(**opt)


@functools.lru_cache(maxsize=None)
def restated(i):
    name, sc, opt = COMPARISONS[i]
    run = ref.adjust_local_bundle(sc, opt)
    return run, ref.is_clear(sc, opt, run)


def steps_of(trace):
    """What the trace shows per iteration: 'a' accepted, 'r' rejected (rho is a number), 'n' no ratio (rho is NaN: an invalid
    step, or a step that ended the run at the parameter or function tolerance before rho was formed)."""
    return "".join("a" if row[3] == 1.0 else ("n" if np.isnan(row[2]) else "r") for row in trace[1:])


def shown(steps):
    """The restatement's step string reduced to what a trace can show ('i' and 't' both read 'n'; num_invalid_steps, compared
    beside it, tells them apart)."""
    return steps.replace("i", "n").replace("t", "n")


def compare(name, dev, run, clear):
    r, w = dev["result"], run["result"]
    print("%s: clear %s, device cost %.17g -> %.17g, restatement %.17g -> %.17g, steps %s / %s, device margins %s"
          % (name, clear, r.initial_cost, r.final_cost, w["initial_cost"], w["final_cost"], steps_of(dev["trace"]), run["steps"], dev["margins"]))
    assert r.solved == w["solved"] and r.termination == w["termination"], name
    assert (r.num_residuals, r.num_effective_parameters, r.reduced_dim) == (w["num_residuals"], w["num_effective_parameters"], w["reduced_dim"]), name
    if not clear:
        assert abs(r.final_cost - w["final_cost"]) <= UNCLEAR_COST_TOLERANCE * w["initial_cost"], name
        return
    assert (r.num_iterations, r.num_successful_steps, r.num_invalid_steps) == (w["num_iterations"], w["num_successful_steps"], w["num_invalid_steps"]), name
    assert steps_of(dev["trace"]) == shown(run["steps"]), name
    assert min(dev["margins"].values()) >= 1e-9, (name, dev["margins"])
    d = rel_change(run, dev)
    print("   relative difference %.3e (tolerance %.3e)" % (d, CLEAR_TOLERANCE))
    assert d <= CLEAR_TOLERANCE, (name, d)
    assert abs(r.initial_mean_reprojection_error - w["initial_mean_reprojection_error"]) <= CLEAR_TOLERANCE * w["initial_mean_reprojection_error"]
    assert abs(r.final_mean_reprojection_error - w["final_mean_reprojection_error"]) <= CLEAR_TOLERANCE * w["final_mean_reprojection_error"]


@pytest.mark.parametrize("i", range(len(COMPARISONS)), ids=[c[0] for c in COMPARISONS])
def test_device_agrees_with_the_restatement(ctx, i):
    name, sc, opt = COMPARISONS[i]
    run, clear = restated(i)
    dev = ctx.adjust_local_bundles([sc], options(opt))["problems"][0]
    compare(name, dev, run, clear)


def test_reduced_dimension_128_is_accepted_and_129_refused(ctx):
    from dagsfm_amd import capi
    sc = scenes.reduced_dim_scene(False)
    dev = ctx.adjust_local_bundles([sc], options(scenes.REDUCED_DIM_OPTIONS))["problems"][0]
    assert dev["result"].reduced_dim == 128 == capi.LOCAL_BUNDLE_MAX_REDUCED_DIM
    run = ref.adjust_local_bundle(sc, scenes.REDUCED_DIM_OPTIONS)
    compare("reduced_dim_128", dev, run, ref.is_clear(sc, scenes.REDUCED_DIM_OPTIONS, run))
    with pytest.raises(capi.DsmError, match="129 columns.*dsm_bundle_adjust"):
        ctx.adjust_local_bundles([scenes.reduced_dim_scene(True)], options(scenes.REDUCED_DIM_OPTIONS))


def same_bytes(a, b):
    return (all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("camera_params", "qvec", "tvec", "xyz", "trace"))
            and bytes(a["result"]) == bytes(b["result"]) and a["margins"] == b["margins"])


@pytest.mark.parametrize("B", [1, 2, 70])
def test_batches_of_mixed_sizes_and_a_problem_alone(ctx, B):
    """B problems of mixed sizes in ONE call under one option set (the options do not depend on the scene): every problem's
    bytes are those of the same problem alone, of a repeat, and of its other places in the batch."""
    from dagsfm_amd import capi
    opt = dict(gradient_tolerance=1e-3, max_num_iterations=6)
    idx = [(7 * k + 3) % len(COMPARISONS) for k in range(B)]
    batch = ctx.adjust_local_bundles([COMPARISONS[k][1] for k in idx], options(opt))
    assert batch["report"].num_problems == B == len(batch["problems"])
    assert batch["report"].num_points == sum(len(COMPARISONS[k][1]["point_ids"]) for k in idx)
    assert batch["report"].num_observations == sum(len(COMPARISONS[k][1]["obs_image"]) for k in idx)
    if B == 70:
        assert len({len(COMPARISONS[k][1]["obs_image"]) for k in idx}) > 20 and len(set(idx)) < B  # mixed sizes, and repeats
    again = ctx.adjust_local_bundles([COMPARISONS[k][1] for k in idx], options(opt))
    alone = {}
    for pos, k in enumerate(idx):
        assert same_bytes(batch["problems"][pos], again["problems"][pos])
        if k not in alone:
            alone[k] = ctx.adjust_local_bundles([COMPARISONS[k][1]], options(opt))["problems"][0]
        assert same_bytes(batch["problems"][pos], alone[k]), COMPARISONS[k][0]
    assert batch["report"].num_iterations == sum(p["result"].num_iterations for p in batch["problems"])
    for m, key in enumerate(capi.LOCAL_BUNDLE_MARGINS):
        assert batch["report"].min_margin[m] == min(p["margins"][key] for p in batch["problems"])


def test_a_step_that_ends_at_the_function_tolerance_reads_as_the_restatement_says(ctx):
    """function_tolerance > 0: the run ends in CONVERGENCE on a valid step that is not applied and forms no rho."""
    name, sc, _ = COMPARISONS[2]
    opt = dict(gradient_tolerance=1e-10, function_tolerance=1e-3, max_num_iterations=30)
    run = ref.adjust_local_bundle(sc, opt)
    assert run["steps"].endswith("t") and run["result"]["num_invalid_steps"] == 0
    dev = ctx.adjust_local_bundles([sc], options(opt))["problems"][0]
    compare(name + "_function_tolerance", dev, run, ref.is_clear(sc, opt, run))
    assert steps_of(dev["trace"]).endswith("n") and dev["result"].num_invalid_steps == 0


def shuffled(sc, seed, images=True, cameras=True):
    rng = np.random.default_rng(seed)
    N, P, C = len(sc["image_camera"]), len(sc["point_ids"]), len(sc["camera_model_ids"])
    ip = rng.permutation(N) if images else np.arange(N)
    cp = rng.permutation(C) if cameras else np.arange(C)
    pp = rng.permutation(P)
    toff = np.asarray(sc["track_offsets"], np.int64)
    tracks = [rng.permutation(np.arange(toff[p], toff[p + 1])) for p in pp]
    order = np.concatenate(tracks) if tracks else np.zeros(0, np.int64)
    iinv, cinv = np.empty(N, np.int64), np.empty(C, np.int64)
    iinv[ip], cinv[cp] = np.arange(N), np.arange(C)
    poff = np.concatenate([[0], np.cumsum([ref.NUM_PARAMS[m] for m in sc["camera_model_ids"]])])
    out = dict(sc, camera_model_ids=sc["camera_model_ids"][cp], camera_params=np.concatenate([sc["camera_params"][poff[c]:poff[c + 1]] for c in cp]),
               camera_constant=np.asarray(sc["camera_constant"])[cp], image_camera=cinv[sc["image_camera"][ip]].astype(np.uint32),
               qvec=sc["qvec"][ip], tvec=sc["tvec"][ip], image_constant_pose=sc["image_constant_pose"][ip],
               image_constant_tvec=sc["image_constant_tvec"][ip], point_ids=sc["point_ids"][pp], xyz=sc["xyz"][pp],
               point_constant=np.asarray(sc["point_constant"])[pp], track_offsets=np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32),
               obs_image=iinv[sc["obs_image"][order]].astype(np.uint32), obs_xy=sc["obs_xy"][order])
    return out, ip, cp, pp, poff


@pytest.mark.parametrize("name", ["config6_outside4", "per_image_focal", "tracks_16_17"])
def test_shuffles_of_points_tracks_images_and_cameras_give_the_same_bytes(ctx, name):
    _, sc, opt = next(c for c in COMPARISONS if c[0] == name)
    a = ctx.adjust_local_bundles([sc], options(opt))["problems"][0]
    for seed in (1, 2):
        sh, ip, cp, pp, poff = shuffled(sc, seed)
        b = ctx.adjust_local_bundles([sh], options(opt))["problems"][0]
        assert a["trace"].tobytes() == b["trace"].tobytes() and bytes(a["result"]) == bytes(b["result"]) and a["margins"] == b["margins"]
        assert a["qvec"][ip].tobytes() == b["qvec"].tobytes() and a["tvec"][ip].tobytes() == b["tvec"].tobytes()
        assert a["xyz"][pp].tobytes() == b["xyz"].tobytes()
        assert np.concatenate([a["camera_params"][poff[c]:poff[c + 1]] for c in cp]).tobytes() == b["camera_params"].tobytes()


def test_no_residual_and_all_constant_problems_keep_their_bits(ctx):
    sc = scenes.local_scene(4, 3, 0, n_points=10)
    empty = dict(sc, track_offsets=np.zeros(11, np.uint32), obs_image=np.zeros(0, np.uint32), obs_xy=np.zeros((0, 2)))
    const = dict(sc, image_constant_pose=np.ones(3, np.uint8), point_constant=np.ones(10, np.uint8), camera_constant=np.ones(1, np.uint8))
    out = ctx.adjust_local_bundles([empty, const, sc])["problems"]
    for o in out[:2]:
        for k in ("qvec", "tvec", "xyz", "camera_params"):
            assert np.array_equal(o[k], np.asarray(sc[k], np.float64).reshape(o[k].shape)), k
        assert o["result"].num_iterations == 0 and o["result"].termination == 0
    assert out[0]["result"].solved == 0 and out[0]["result"].num_residuals == 0 and len(out[0]["trace"]) == 0
    w = ref.adjust_local_bundle(const)["result"]
    assert out[1]["result"].solved == 1 and out[1]["result"].num_effective_parameters == 0
    assert abs(out[1]["result"].final_cost - w["final_cost"]) <= CLEAR_TOLERANCE * w["final_cost"] and out[1]["result"].final_cost == out[1]["result"].initial_cost
    assert out[2]["result"].solved == 1
    # an image and a point without residuals come back bit-identical inside a problem that moves
    more = dict(sc, image_camera=np.append(sc["image_camera"], 0).astype(np.uint32), qvec=np.vstack([sc["qvec"], [[2.0, 0.0, 0.0, 0.0]]]),
                tvec=np.vstack([sc["tvec"], [[1.0, 2.0, 3.0]]]), image_constant_pose=np.append(sc["image_constant_pose"], 0).astype(np.uint8),
                image_constant_tvec=np.append(sc["image_constant_tvec"], 0).astype(np.uint8))
    o = ctx.adjust_local_bundles([more], options(dict(gradient_tolerance=1e-3)))["problems"][0]
    assert list(o["qvec"][3]) == [2.0, 0.0, 0.0, 0.0] and list(o["tvec"][3]) == [1.0, 2.0, 3.0] and o["result"].num_successful_steps >= 1
    assert abs(np.linalg.norm(o["qvec"][2]) - 1.0) < 1e-15  # a constant-pose image with residuals is returned normalised


def test_refusals(ctx):
    from dagsfm_amd import capi
    sc = scenes.local_scene(4, 3, 0, n_points=10)

    def refused(scene, match, **opt):
        with pytest.raises(capi.DsmError, match=match):
            ctx.adjust_local_bundles([scene], options(opt))
    refused(dict(sc, camera_model_ids=np.array([11], np.int32)), "unknown camera model")
    refused(dict(sc, image_camera=np.array([0, 1, 0], np.uint32)), "image_camera out of range")
    refused(dict(sc, obs_image=np.where(np.arange(len(sc["obs_image"])) == 0, 3, sc["obs_image"]).astype(np.uint32)), "obs_image out of range")
    for key in ("camera_params", "qvec", "tvec", "xyz", "obs_xy"):
        bad = np.array(sc[key], np.float64, copy=True)
        bad.reshape(-1)[0] = np.nan
        refused(dict(sc, **{key: bad}), "non-finite")
    q = sc["qvec"].copy()
    q[1] = 0.0
    refused(dict(sc, qvec=q), "zero qvec")
    refused(dict(sc, image_constant_tvec=np.array([0, 8, 0], np.uint8)), "above 7")
    toff = np.asarray(sc["track_offsets"], np.int64)
    twice = sc["obs_image"].copy()
    twice[toff[0] + 1] = twice[toff[0]]
    refused(dict(sc, obs_image=twice), "observes one point twice")
    refused(dict(sc, point_ids=np.zeros(10, np.uint64)), "repeated point id")
    refused(sc, "unknown loss", loss_function_type=3)
    refused(sc, "loss_function_scale", loss_function_scale=0.0)
    refused(sc, "loss_function_scale", loss_function_scale=-1.0)
    refused(sc, "above 1000", max_num_iterations=1001)
    assert ctx.adjust_local_bundles([sc], options(dict(loss_function_type=capi.LOSS_TRIVIAL, loss_function_scale=0.0)))["problems"][0]["result"].solved == 1
    L = ctx._L  # NULL where data is needed
    off = (np.array([0, 1], np.uint32), np.array([0, 3], np.uint32), np.array([0, 10], np.uint32), np.array([0, len(sc["obs_image"])], np.uint64))
    res = (capi.LocalBundleResult * 1)()
    rc = L.dsm_adjust_local_bundles(ctx._h, 1, off[0].ctypes.data, None, None, None, off[1].ctypes.data, None, None, None, None, None,
                                    off[2].ctypes.data, None, None, None, None, off[3].ctypes.data, None, None, None, res, None, None, None)
    assert rc == 1
    # offsets that do not ascend from 0
    # (the binding always builds ascending offsets, so these go through the C call)
    import ctypes
    pr = {k: np.ascontiguousarray(v) for k, v in sc.items()}
    o = options({})

    def raw(coff, ioff, poff, ooff, toff=None):
        a = [np.asarray(x, dt) for x, dt in ((coff, np.uint32), (ioff, np.uint32), (poff, np.uint32), (ooff, np.uint64))]
        t = np.asarray(pr["track_offsets"] if toff is None else toff, np.uint32)
        q, tv, x, prm = (np.array(pr[k], np.float64, copy=True) for k in ("qvec", "tvec", "xyz", "camera_params"))
        ptr = lambda z: z.ctypes.data
        mids, icam, pids = pr["camera_model_ids"].astype(np.int32), pr["image_camera"].astype(np.uint32), pr["point_ids"].astype(np.uint64)
        oimg, oxy = pr["obs_image"].astype(np.uint32), pr["obs_xy"].astype(np.float64)  # (kept alive across the call)
        rc = L.dsm_adjust_local_bundles(ctx._h, 1, ptr(a[0]), ptr(mids), ptr(prm), None, ptr(a[1]), ptr(icam), ptr(q), ptr(tv), None, None,
                                        ptr(a[2]), ptr(pids), ptr(x), None, ptr(t), ptr(a[3]), ptr(oimg), ptr(oxy), ctypes.byref(o), res,
                                        None, None, None)
        return rc, L.dsm_last_error(ctx._h).decode()
    n = len(sc["obs_image"])
    assert raw([0, 1], [0, 3], [0, 10], [0, n])[0] == 0
    rc, msg = raw([1, 2], [0, 3], [0, 10], [0, n])
    assert rc == 1 and "start at 0" in msg
    rc, msg = raw([0, 1], [0, 3], [0, 10], [0, n], toff=np.r_[1, np.asarray(sc["track_offsets"])[1:]])
    assert rc == 1 and "track_offsets of a problem must start at 0" in msg
    two = (capi.LocalBundleResult * 2)()
    a = [np.array([0, 1, 0], np.uint32), np.array([0, 3, 3], np.uint32), np.array([0, 10, 10], np.uint32), np.array([0, n, n], np.uint64)]
    rc = L.dsm_adjust_local_bundles(ctx._h, 2, a[0].ctypes.data, None, None, None, a[1].ctypes.data, None, None, None, None, None,
                                    a[2].ctypes.data, None, None, None, None, a[3].ctypes.data, None, None, None, two, None, None, None)
    assert rc == 1 and "ascend" in L.dsm_last_error(ctx._h).decode()
    down = np.asarray(sc["track_offsets"]).copy()
    down[3] = down[2] - 1
    rc, msg = raw([0, 1], [0, 3], [0, 10], [0, n], toff=down)
    assert rc == 1 and "track_offsets must ascend" in msg
    with pytest.raises(capi.DsmError, match="parameter counts"):
        ctx.adjust_local_bundles([dict(sc, camera_params=np.asarray(sc["camera_params"])[:-1])])


def test_chain_register_cut_adjust_filter(ctx):
    """Context.register_images -> capi.local_bundle_problem -> adjust_local_bundles -> Context.filter_points3D on one planted scene."""
    from dagsfm_amd import capi
    from tests.bundle_adjustment_ref import DEFAULT_PARAMS, quat_rotate
    from dagsfm_amd.synthetic import world_to_image
    s = scenes.local_scene(21, 5, 0, n_points=120, noise=0.3, min_track=4, max_track=5, arc=0.9)
    new = 0  # register image 0 from the points it sees
    toff, oimg = np.asarray(s["track_offsets"], np.int64), np.asarray(s["obs_image"], np.int64)
    ks = np.nonzero(oimg == new)[0]
    pts = np.searchsorted(toff, ks, side="right") - 1
    cam = capi.camera(2, s["camera_params"], 640, 480)
    reg = ctx.register_images([cam], [0, len(ks)], s["obs_xy"][ks], s["xyz"][pts], refine_flags=[0])
    assert reg["registered"][0]
    s2 = dict(s, qvec=s["qvec"].copy(), tvec=s["tvec"].copy())
    s2["qvec"][new], s2["tvec"][new] = reg["qvec"][0], reg["tvec"][0]
    prob = capi.local_bundle_problem(s2, new, [1, 2, 3, 4], np.unique(pts))
    out = ctx.adjust_local_bundles([prob], options(dict(gradient_tolerance=1e-3)))["problems"][0]
    r = out["result"]
    assert r.solved == 1 and r.num_successful_steps >= 1 and r.final_cost < r.initial_cost
    assert r.num_residuals == 2 * len(prob["obs_image"])
    s3 = dict(s2, qvec=s2["qvec"].copy(), tvec=s2["tvec"].copy(), xyz=np.array(s2["xyz"], copy=True), camera_params=out["camera_params"])
    s3["qvec"][prob["image_index"]], s3["tvec"][prob["image_index"]] = out["qvec"], out["tvec"]
    s3["xyz"][prob["point_index"]] = out["xyz"]
    f = ctx.filter_points3D(s3)
    assert f["point_keep"].sum() >= 0.9 * len(f["point_keep"])
    assert f["report"].mean_point_error < 1.0
