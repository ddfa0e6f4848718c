"""dsm_bundle_adjust on the device against the restatement on the scenes of tests/bundle_adjustment_scenes.py: camera groups,
constant-tvec masks, exits, block edges and gaps in the lists.  Every comparison is the strict compare() of
tests/test_bundle_adjustment_gpu.py, unchanged; tests/test_bundle_adjustment_edges_cpu.py holds that every scene is clear
in the restatement, and each test here asserts it again before it compares, so the weak rule is out of reach."""
import functools

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import bundle_adjustment_ref as ref
from tests import bundle_adjustment_scenes as scenes
from tests.test_bundle_adjustment_gpu import MARGIN, clear, compare, run, shuffled

pytestmark = pytest.mark.gpu
COMPARISONS = scenes.comparisons()
KEYS = ("xyz", "qvec", "tvec", "camera_params")


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


def named(name):
    return next(c for c in COMPARISONS if c[0] == name)


@functools.lru_cache(maxsize=None)
def restated(name):
    _, scene, opt = named(name)
    rr = ref.bundle_adjust(scene, opt)
    assert MARGIN == 1e-9 and clear(rr["report"]) and ref.stable_under_rounding(scene, opt, rr), name
    return rr


@functools.lru_cache(maxsize=None)
def device(ctx, name):
    _, scene, opt = named(name)
    return run(ctx, scene, **opt)


def strict(ctx, name):
    _, scene, _ = named(name)
    dev, rr = device(ctx, name), restated(name)
    print("%s: device CG %s, restatement CG %s; cost %.17g / %.17g" % (name, list(dev["trace"][1:, 3].astype(int)), rr["cg_iterations"],
                                                                      dev["report"].final_cost, rr["report"]["final_cost"]))
    compare(dev, rr, scene)
    return dev, rr


def names(kind):
    return [c[0] for c in scenes.of_kind(kind)]


@pytest.mark.parametrize("name", names("groups"))
def test_cameras_shared_by_some_of_the_images(ctx, name):
    strict(ctx, name)


def test_groups_give_the_same_bytes_for_every_order_of_points_tracks_images_and_cameras(ctx):
    _, scene, opt = named("groups_600")
    a = device(ctx, "groups_600")
    swapped = False
    for seed in (1, 2):
        sc, perm = shuffled(scene, seed)
        sc, ip, cp = scenes.permuted_images_and_cameras(sc, seed)
        assert list(ip) != sorted(ip)
        c = run(ctx, sc, **opt)
        assert c["trace"].tobytes() == a["trace"].tobytes()
        assert c["xyz"].tobytes() == a["xyz"][perm].tobytes()
        assert c["qvec"].tobytes() == a["qvec"][ip].tobytes() and c["tvec"].tobytes() == a["tvec"][ip].tobytes()
        assert c["camera_params"].tobytes() == scenes.camera_blocks(a["camera_params"], scene["camera_model_ids"], cp).tobytes()
        swapped = swapped or list(cp) == [1, 0]
    assert swapped  # one of the two seeds lists the cameras the other way round


@pytest.mark.parametrize("name", names("masks"))
def test_constant_tvec_masks(ctx, name):
    _, scene, _ = named(name)
    dev, rr = strict(ctx, name)
    i, m = scenes.MASKED_IMAGE, int(scene["image_constant_tvec"][scenes.MASKED_IMAGE])
    for a in range(3):
        if (m >> a) & 1:
            assert dev["tvec"][i, a].tobytes() == scene["tvec"][i, a].tobytes()
        else:
            assert dev["tvec"][i, a] != scene["tvec"][i, a]
    if m == 7:
        assert dev["report"].num_effective_parameters == rr["report"]["num_effective_parameters"]
        assert all(np.isfinite(dev[k]).all() for k in KEYS) and np.isfinite(dev["trace"][:, [0, 1, 3, 4, 5]]).all()
        assert np.isfinite(dev["trace"][1:, 2]).all()  # rho of every step; row 0 has none


@pytest.mark.parametrize("name", names("exits"))
def test_exits(ctx, name):
    dev, rr = strict(ctx, name)
    if name in ("exit_function_tolerance", "exit_parameter_tolerance"):
        # CONVERGENCE on a valid step that is not applied: no rho, not accepted, the cost of the row before
        assert dev["report"].termination == capi.BA_CONVERGENCE and dev["report"].num_invalid_steps == 0
        last = dev["trace"][-1]
        assert np.isnan(last[2]) and last[4] == 0 and last[0] == dev["trace"][-2, 0] == dev["report"].final_cost
    if name.startswith("exit_cg_cap"):
        cap = named(name)[2]["max_linear_solver_iterations"]
        assert dev["trace"][1:, 3].max() == cap and (dev["trace"][2:, 3] == cap).all()


def test_non_finite_initial_cost_is_a_failure_that_changes_nothing(ctx):
    scene = scenes.failure_scene()
    dev = run(ctx, scene)
    rep = dev["report"]
    assert rep.termination == capi.BA_FAILURE and rep.num_iterations == 0 and rep.num_successful_steps == 0
    assert dev["trace"].shape == (1, capi.BA_TRACE_COLUMNS) and not np.isfinite(dev["trace"][0, 0])
    assert not np.isfinite(rep.initial_cost)
    qn = scene["qvec"] / np.linalg.norm(scene["qvec"], axis=1, keepdims=True)
    assert dev["qvec"].tobytes() == qn.tobytes()
    for k in ("tvec", "xyz", "camera_params"):
        assert dev[k].tobytes() == np.asarray(scene[k], np.float64).tobytes(), k


@pytest.mark.parametrize("name", names("edges"))
def test_block_edges(ctx, name):
    dev, rr = strict(ctx, name)
    if name in scenes.NF_EXPECTED:  # the device's f columns are 6 per image and the free camera parameters
        pb = rr["problem"]
        assert 6 * len(pb.icam) + sum(len(c) for c in pb.ccol) == scenes.NF_EXPECTED[name]


@pytest.mark.parametrize("name", names("gaps"))
def test_gaps_in_the_image_and_camera_lists(ctx, name):
    _, scene, _ = named(name)
    _, base, _ = named("groups_600")
    dev, rr = strict(ctx, name)
    assert list(dev["qvec"][scenes.GAP_IMAGE]) == scenes.GAP_QVEC and list(dev["tvec"][scenes.GAP_IMAGE]) == scenes.GAP_TVEC
    poff = np.concatenate([[0], np.cumsum([ref.NUM_PARAMS[m] for m in scene["camera_model_ids"]])])
    assert list(dev["camera_params"][poff[scenes.GAP_CAMERA]:poff[scenes.GAP_CAMERA + 1]]) == scenes.GAP_PARAMS
    plain, cut = device(ctx, "groups_600"), scenes.without_gaps(dev, base)
    assert dev["trace"].tobytes() == plain["trace"].tobytes()
    for k in KEYS:
        assert cut[k].tobytes() == plain[k].tobytes(), k
