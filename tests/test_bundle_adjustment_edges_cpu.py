"""CPU-only: what the restatement (tests/bundle_adjustment_ref.py) alone must satisfy on every scene of
tests/bundle_adjustment_scenes.py, so that tests/test_bundle_adjustment_edges_gpu.py can hold the device to the strict rule
on all of them: each scene is clear (every margin >= MARGIN, stable under the conditioning probe) and has the shape its name
promises -- the camera runs, the block sizes, the exits."""
import functools

import numpy as np
import pytest

from tests import bundle_adjustment_ref as ref
from tests import bundle_adjustment_scenes as scenes

MARGIN = 1e-9  # tests/test_bundle_adjustment_gpu.py's (importing that file needs the device library)
COMPARISONS = scenes.comparisons()
NAMES = [c[0] for c in COMPARISONS]


@functools.lru_cache(maxsize=None)
def restated(name):
    _, scene, opt = next(c for c in COMPARISONS if c[0] == name)
    return ref.bundle_adjust(scene, opt)


def named(name):
    return next(c for c in COMPARISONS if c[0] == name)


def test_names_are_unique_and_every_kind_is_there():
    assert len(set(NAMES)) == len(NAMES)
    for kind, _ in scenes.KINDS:
        assert len(scenes.of_kind(kind)) >= 1
    assert sum(len(scenes.of_kind(kind)) for kind, _ in scenes.KINDS) == len(COMPARISONS)


@pytest.mark.parametrize("name", NAMES)
def test_every_scene_is_clear_in_the_restatement(name):
    """The condition under which the GPU file applies the strict compare() and never the weak branch."""
    _, scene, opt = named(name)
    rr = restated(name)
    rep = rr["report"]
    margin = min(rep["min_rho_margin"], rep["min_cg_margin"], rep["min_gradient_margin"])
    print("%s: margin %.3e, termination %d after %d iterations, CG %s, accepted %s"
          % (name, margin, rep["termination"], rep["num_iterations"], rr["cg_iterations"], rr["accepted"]))
    assert margin >= MARGIN
    assert ref.stable_under_rounding(scene, opt, rr)
    assert rep["num_successful_steps"] >= 1


def camera_runs(scene):
    """Per track the number of its images on each camera."""
    toff = scene["track_offsets"].astype(np.int64)
    icam = scene["image_camera"].astype(np.int64)
    return [np.bincount(icam[scene["obs_image"][toff[p]:toff[p + 1]]]) for p in range(len(toff) - 1)]


@pytest.mark.parametrize("name", [c[0] for c in scenes.of_kind("groups") + scenes.of_kind("gaps")])
def test_group_scenes_hold_a_camera_run_inside_a_track(name):
    """A run of two or more images of one camera that is not the whole track: neither of the two cases the older scenes
    cover (one camera for all images: every run is its track; one camera per image: every run has length 1)."""
    _, scene, _ = named(name)
    runs = camera_runs(scene)
    inside = [p for p, b in enumerate(runs) if any(2 <= v < b.sum() for v in b)]
    assert inside, name
    # and a run that starts past the track's first element: in (camera, image) order that is a run of a camera other than
    # the track's lowest one
    assert any(np.nonzero(runs[p] >= 2)[0].max() > np.nonzero(runs[p])[0].min() for p in inside), name
    per_camera = np.bincount(scene["image_camera"][np.unique(scene["obs_image"])], minlength=len(scene["camera_model_ids"]))
    assert (per_camera < len(np.unique(scene["obs_image"]))).all() and per_camera.max() >= 2  # shared by some, by none all


def test_groups_602_has_runs_of_five():
    assert max(b.max() for b in camera_runs(named("groups_602")[1])) == 5


@pytest.mark.parametrize("m", range(2, 8))
def test_mask_scenes_free_the_unmasked_components_only(m):
    name, scene, _ = named("mask_%d" % m)
    i = scenes.MASKED_IMAGE
    assert scene["image_constant_tvec"][i] == m and not scene["image_constant_pose"][i]
    rr = restated(name)
    pb = rr["problem"]
    for a in range(3):
        if (m >> a) & 1:
            assert pb.tcol[i, a] < 0 and rr["tvec"][i, a] == scene["tvec"][i, a]
        else:
            assert pb.tcol[i, a] >= 0 and rr["tvec"][i, a] != scene["tvec"][i, a]
    if m == 7:  # no tvec block at all
        assert not any(set(blk) & set(pb.tcol[i]) for blk in pb.fblocks)
        # 100 points; images 1..5 free (0 is the gauge): 5 qvecs; tvecs 2 (the gauge's mask 1) + 3 + 0 + 3 + 3; f and k
        assert rr["report"]["num_effective_parameters"] == 3 * 100 + 3 * 5 + (2 + 3 + 0 + 3 + 3) + 2


def test_exits_end_as_stated():
    for name, iterations in (("exit_function_tolerance", 7), ("exit_parameter_tolerance", 13)):
        rr = restated(name)
        assert rr["report"]["termination"] == ref.CONVERGENCE and rr["report"]["num_iterations"] == iterations
        last = rr["trace"][-1]
        assert np.isnan(last[2]) and last[4] == 0 and rr["accepted"][-1] == 0  # a valid step that is not applied
        assert last[0] == rr["trace"][-2][0] and rr["report"]["num_invalid_steps"] == 0
        assert last[5] > named(name)[2]["gradient_tolerance"]  # not the gradient test
    assert restated("exit_cg_cap_3")["cg_iterations"] == [2, 3, 3, 3, 3, 3]  # the cap binds
    assert restated("exit_cg_cap_1")["cg_iterations"] == [1] * 6
    assert max(restated("exit_cg_past_two_resets")["cg_iterations"]) == 21  # past the residual resets at 10 and 20


def test_failure_scene_fails_at_iteration_zero():
    scene = scenes.failure_scene()
    toff = scene["track_offsets"].astype(np.int64)
    for p in range(len(toff) - 1):
        assert len(set(scene["obs_image"][toff[p]:toff[p + 1]])) == toff[p + 1] - toff[p]
    with np.errstate(all="ignore"):
        rr = ref.bundle_adjust(scene, {})
    assert rr["report"]["termination"] == ref.FAILURE and rr["report"]["num_iterations"] == 0
    assert rr["trace"].shape == (1, 6) and not np.isfinite(rr["trace"][0, 0])


def test_block_edges_have_the_sizes_their_names_promise():
    for P in (1, 2, 255, 256, 257):
        assert len(named("points_%d" % P)[1]["point_ids"]) == P
    for n in (256, 512):
        assert len(named("observations_%d" % n)[1]["obs_image"]) == n
    for n in (64, 65):
        assert list(np.bincount(named("image_observations_%d" % n)[1]["obs_image"])) == [n] * 4
    for name, nf in scenes.NF_EXPECTED.items():
        _, scene, opt = named(name)
        assert opt["refine_extra_params"] == 0 and not opt.get("refine_principal_point", 0)
        k = [2 if m in ref.TWO_FOCAL else 1 for m in scene["camera_model_ids"]]  # the focal lengths
        assert len(scene["image_camera"]) == scenes.NF_IMAGES and 6 * scenes.NF_IMAGES + sum(k) == nf
        assert len(np.unique(scene["obs_image"])) == scenes.NF_IMAGES  # every image in the problem
        assert [len(c) for c in restated(name)["problem"].ccol] == k


def test_gaps_leave_an_empty_segment_before_live_ones():
    name, scene, _ = named("gaps_in_groups_600")
    _, base, _ = named("groups_600")
    N, C = len(scene["image_camera"]), len(scene["camera_model_ids"])
    assert N == len(base["image_camera"]) + 1 and C == len(base["camera_model_ids"]) + 1
    assert scenes.GAP_IMAGE not in scene["obs_image"] and scene["obs_image"].max() == N - 1
    assert scenes.GAP_CAMERA not in scene["image_camera"] and scene["image_camera"].max() == C - 1
    assert 0 < scenes.GAP_IMAGE < N - 1 and 0 < scenes.GAP_CAMERA < C - 1
    a, b = restated("groups_600"), restated(name)
    assert a["trace"].tobytes() == b["trace"].tobytes()
    cut = scenes.without_gaps(b, base)
    for k in ("qvec", "tvec", "xyz", "camera_params"):
        assert cut[k].tobytes() == a[k].tobytes(), k
    assert list(b["qvec"][scenes.GAP_IMAGE]) == scenes.GAP_QVEC and list(b["tvec"][scenes.GAP_IMAGE]) == scenes.GAP_TVEC


def test_permuted_images_and_cameras_are_the_same_problem():
    _, base, opt = named("groups_600")
    sh, ip, cp = scenes.permuted_images_and_cameras(base, 1)
    assert list(ip) != sorted(ip) and list(cp) != sorted(cp)
    a = restated("groups_600")
    b = ref.bundle_adjust(sh, opt)
    assert (b["accepted"], b["cg_iterations"]) == (a["accepted"], a["cg_iterations"])
    np.testing.assert_allclose(b["trace"][:, 0], a["trace"][:, 0], rtol=1e-9)  # the GPU file's rule: only the order of sums differs
    np.testing.assert_allclose(b["qvec"], a["qvec"][ip], rtol=0, atol=1e-7)
    np.testing.assert_allclose(b["tvec"], a["tvec"][ip], rtol=0, atol=1e-7 * float(np.abs(base["xyz"]).max()))
    np.testing.assert_allclose(b["camera_params"], scenes.camera_blocks(a["camera_params"], base["camera_model_ids"], cp), rtol=1e-7)
