"""GPU: the undistortion stage against its numpy restatement (tests/undistortion_ref.py, held to the reference's
known answers by tests/test_undistortion_cpu.py) -- `==` on every byte of every image and camera and on every double of the
map of source points and of the undistorted 2D points.  Shapes are the smallest at which the kernels can go wrong: sides that
are no multiple of the four pixels of a lane or of the 256 x 4 tile, more than one tile, borders that span more than one block
and end off a block edge."""
import ctypes

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import undistortion_ref as ref
from tests import undistortion_scenes as scenes

pytestmark = pytest.mark.gpu

ROI = dict(roi_min_x=0.1, roi_min_y=0.2, roi_max_x=0.9, roi_max_y=0.8)
_SHARED = {}


def _same_camera(a, b):
    assert bytes(a) == bytes(b), ([a.model_id, a.width, a.height] + list(a.params), [b.model_id, b.width, b.height] + list(b.params))


def _check_cameras(dsm, oracle, cams, **options):
    got = dsm.undistort_cameras(cams, **options)
    assert len(got) == len(cams)
    for g, c in zip(got, cams):
        _same_camera(g, ref.undistort_camera(oracle, c, **options))
    return got


def _check_warp(dsm, oracle, source, target, images, H=None):
    want = ref.warp_images(oracle, source, target, images, H)
    got = dsm.warp_images(source, target, images, H=H, return_map=True)
    g, w = got["source_xy"], want["source_xy"]
    assert g.shape == w.shape
    # the same bits, or a NaN on both sides (the sign of a generated NaN is the hardware's)
    assert ((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all(), "the map differs"
    assert got["images"].shape == want["images"].shape and (got["images"] == want["images"]).all(), "the samples differ"
    _same_camera(got["scaled_target"], want["scaled_target"])
    assert got["needs_rescale"] == want["needs_rescale"]
    return got, want


# ---- cameras ----
@pytest.mark.parametrize("model_id", scenes.MODELS)
def test_cameras_every_model_and_blank_pixels(dsm, oracle, model_id):
    cam = scenes.camera(model_id, 67, 45)
    for bp in (0.0, 0.5, 1.0):
        und = _check_cameras(dsm, oracle, [cam], blank_pixels=bp)[0]
        assert und.model_id == 1 and und.has_prior_focal_length == 0


def test_cameras_roi_and_max_image_size(dsm, oracle):
    cams = [scenes.camera(m, 67, 45) for m in scenes.MODELS]
    _check_cameras(dsm, oracle, cams, blank_pixels=1.0, max_scale=1.0, **ROI)
    small = _check_cameras(dsm, oracle, cams, max_image_size=30)  # below the size: Camera::Rescale(scale)
    assert all(max(c.width, c.height) <= 30 for c in small)
    _check_cameras(dsm, oracle, cams, max_image_size=1000)  # above it: untouched


def test_cameras_mixed_batch_and_long_borders(dsm, oracle):
    """One launch over the borders of all cameras: every model, and 300 x 7 / 7 x 300 whose borders span more than one block of
    256 and end off a block edge, between cameras without a scan (PINHOLE)."""
    cams = ([scenes.camera(m, 67, 45) for m in scenes.MODELS] + [scenes.camera(4, 300, 7), scenes.camera(1, 50, 40),
                                                                   scenes.camera(9, 7, 300), scenes.camera(0, 9, 9), scenes.camera(6, 300, 7)])
    _check_cameras(dsm, oracle, cams, blank_pixels=0.5)


def test_cameras_known_answers_on_the_device(dsm):
    """undistortion_test.cc:40-100 through the device, the NaN of the 1 x 1 SIMPLE_RADIAL case included."""
    for model_id in (0, 2):
        u = dsm.undistort_cameras([capi.camera(model_id, [1.0, 0.5, 0.5, 0.0][:3 + (model_id == 2)], 1, 1)])[0]
        assert (u.model_id, u.params[0], u.params[1], u.width, u.height) == (1, 1, 1, 1, 1)
    cam = capi.camera(2, [100.0, 50.0, 50.0, 0.5], 100, 100)
    u = dsm.undistort_cameras([cam])[0]
    assert (u.width, u.height, u.params[2], u.params[3]) == (84, 84, 42.0, 42.0)
    u = dsm.undistort_cameras([cam], blank_pixels=1)[0]
    assert (u.width, u.height, u.params[2], u.params[3]) == (90, 90, 45.0, 45.0)
    u = dsm.undistort_cameras([cam], blank_pixels=1, max_scale=0.75)[0]
    assert (u.width, u.height) == (75, 75)
    u = dsm.undistort_cameras([cam], blank_pixels=1, max_scale=1.0, **ROI)[0]
    assert (u.width, u.height, u.params[2], u.params[3]) == (80, 60, 40.0, 30.0)
    assert dsm.undistort_cameras([]) == []


# ---- warp ----
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("width,height", [(1, 1), (2, 2), (67, 45), (130, 33), (257, 3)])
def test_warp_sizes(dsm, oracle, width, height, channels):
    """SIMPLE_RADIAL into its undistorted camera; three images in one batch, rows longer than width * channels."""
    source = scenes.camera(2, width, height)
    target = dsm.undistort_cameras([source])[0]
    images = scenes.with_row_padding(scenes.stack(width, height, 3, channels), 5)
    got, _ = _check_warp(dsm, oracle, source, target, images)
    if width == 1:
        assert not got["images"].any()  # every sample needs a neighbour the image does not have
    else:
        # 2 x 2 has exactly one cell of four taps (x0 = y0 = 0 passes bitmap.cc:235), so its samples are not all refused
        assert got["images"].any()
    one, _ = _check_warp(dsm, oracle, source, target, np.ascontiguousarray(images[:1]))
    assert (one["images"][0] == got["images"][0]).all()


@pytest.mark.parametrize("equal_size", [True, False])
@pytest.mark.parametrize("model_id", scenes.MODELS)
def test_warp_every_model_into_its_undistorted_camera(dsm, oracle, model_id, equal_size):
    source = scenes.camera(model_id, 67, 45)
    opts = dict(min_scale=1.0, max_scale=1.0) if equal_size else dict(min_scale=0.5, max_scale=0.8, blank_pixels=0.5)
    target = dsm.undistort_cameras([source], **opts)[0]
    assert ((target.width, target.height) == (67, 45)) == (equal_size or model_id in (0, 1))
    got, _ = _check_warp(dsm, oracle, source, target, scenes.stack(67, 45, 1, 1, seed=model_id + 1))
    assert got["needs_rescale"] == ((target.width, target.height) != (67, 45))
    assert got["images"].any()


def test_warp_non_pinhole_target(dsm, oracle):
    """RADIAL -> OPENCV: the target's IterativeUndistortion runs per lane."""
    got, _ = _check_warp(dsm, oracle, scenes.camera(3, 67, 45), scenes.camera(4, 67, 45), scenes.stack(67, 45, 1, 3))
    assert got["images"].any()
    _check_warp(dsm, oracle, scenes.camera(3, 67, 45), scenes.camera(4, 80, 50), scenes.stack(67, 45, 1, 1))


HOMOGRAPHIES = {
    "identity": np.eye(3),
    "transposition": np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
    "general": np.array([[0.93, -0.11, 3.7], [0.08, 1.04, -2.2], [3.1e-4, -2.3e-4, 1.01]]),
}


@pytest.mark.parametrize("name", sorted(HOMOGRAPHIES))
def test_warp_homography_modes(dsm, oracle, name):
    H = HOMOGRAPHIES[name]
    grey, colour = scenes.stack(67, 45, 2, 1), scenes.stack(67, 45, 1, 3)
    # WarpImageWithHomography: no cameras; the target image of its own size
    got, _ = _check_warp(dsm, oracle, capi.size_only_camera(67, 45), None, grey, H=H)
    if name == "identity":
        assert (got["images"][:, 1:-1, 1:-1] == grey[:, 1:-1, 1:-1]).all()
    got, _ = _check_warp(dsm, oracle, capi.size_only_camera(67, 45), capi.size_only_camera(45, 67), colour, H=H)
    assert got["images"].shape == (1, 67, 45, 3)
    if name == "transposition":
        assert (got["images"][0, 1:-1, 1:-1] == colour[0].transpose(1, 0, 2)[1:-1, 1:-1]).all()
    # WarpImageWithHomographyBetweenCameras: the UNSCALED target camera takes the warped point (warp.cc:154), with a target of the
    # source's size and with one of another size
    source = scenes.camera(3, 67, 45)
    _check_warp(dsm, oracle, source, scenes.camera(1, 67, 45), grey, H=H)
    got, want = _check_warp(dsm, oracle, source, scenes.camera(4, 80, 50), colour, H=H)
    assert got["needs_rescale"] and (got["scaled_target"].width, got["scaled_target"].height) == (67, 45)
    scaled_map = ref.source_points(oracle, source, want["scaled_target"], H)[0]
    assert not (scaled_map == want["source_xy"]).all(), "the test cannot tell the scaled target from the unscaled one"


# ---- points ----
@pytest.mark.parametrize("n", [0, 1, 65, 1000])
def test_points(dsm, oracle, n):
    cams = [scenes.camera(4, 130, 33), scenes.camera(9, 67, 45)]
    und = dsm.undistort_cameras(cams)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, 2, n).astype(np.uint32)
    xy = rng.uniform(0, 1, (n, 2)) * np.array([[130.0, 33.0], [67.0, 45.0]])[idx] if n else np.zeros((0, 2))
    got = dsm.undistort_points2D(cams, und, idx, xy)
    want = ref.undistort_points2D(oracle, cams, und, idx, xy)
    assert got.shape == (n, 2) and (got.view(np.uint64) == want.view(np.uint64)).all()
    if n:
        assert (got != xy).any()


# ---- errors, then an exact call ----
def _raw_undistort_cameras(dsm, cams, options):
    arr, out = (capi.Camera * len(cams))(*cams), (capi.Camera * len(cams))()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    rc = dsm._L.dsm_undistort_cameras(dsm._h, ctypes.byref(options), len(cams), ctypes.addressof(arr), ctypes.addressof(out))
    return rc, bytes(out)


REFUSED_OPTIONS = [dict(blank_pixels=-0.1), dict(blank_pixels=1.1), dict(min_scale=0.0), dict(min_scale=2.5), dict(max_image_size=0),
                   dict(roi_min_x=-0.1), dict(roi_min_y=-0.1), dict(roi_max_x=1.1), dict(roi_max_y=1.1), dict(roi_min_x=0.6, roi_max_x=0.6),
                   dict(roi_min_y=0.7, roi_max_y=0.6), dict(blank_pixels=float("nan"))]


def test_refused_options_and_cameras(dsm, oracle):
    cams = [scenes.camera(2, 67, 45), scenes.camera(5, 67, 45)]
    untouched = b"\x5a" * (2 * ctypes.sizeof(capi.Camera))
    for kw in REFUSED_OPTIONS:
        rc, out = _raw_undistort_cameras(dsm, cams, capi.default_undistort_options(**kw))
        assert rc == capi.DSM_ERR_INVALID_ARGUMENT and out == untouched, kw
        with pytest.raises(capi.DsmError):
            dsm.undistort_cameras(cams, **kw)
    for bad in (capi.camera(11, [1.0] * 12, 67, 45), capi.camera(2, [50.0, 30.0, 20.0, 0.1], 0, 45)):
        rc, out = _raw_undistort_cameras(dsm, [cams[0], bad], capi.default_undistort_options())
        assert rc == capi.DSM_ERR_INVALID_ARGUMENT and out == untouched
    with pytest.raises(capi.DsmError):
        dsm.undistort_points2D(cams, cams, np.array([2], np.uint32), np.ones((1, 2)))
    with pytest.raises(capi.DsmError):
        dsm.undistort_points2D([cams[0], capi.camera(11, [1.0] * 12, 67, 45)], cams, np.array([0], np.uint32), np.ones((1, 2)))
    _check_cameras(dsm, oracle, cams)


def test_refused_warps(dsm, oracle):
    source = scenes.camera(2, 67, 45)
    target = dsm.undistort_cameras([source])[0]
    images = scenes.stack(67, 45, 2, 1)
    out = np.full((2, 45, 67), 0x5A, np.uint8)

    def refused(src_cam, tgt_cam, im, H=None, dst=None):
        dst = out if dst is None else dst
        with pytest.raises(capi.DsmError):
            dsm.warp_images(src_cam, tgt_cam, im, H=H, out=dst)
        assert (dst == 0x5A).all()

    refused(scenes.camera(2, 66, 45), target, images)                                    # a camera of another size than the images
    refused(scenes.camera(2, 67, 44), target, images)
    refused(source, target, np.zeros((2, 45, 67, 2), np.uint8), dst=np.full((2, 45, 67, 2), 0x5A, np.uint8))  # channels = 2
    short = np.lib.stride_tricks.as_strided(np.zeros(2 * 45 * 67, np.uint8), shape=(2, 45, 67), strides=(45 * 66, 66, 1))
    refused(source, target, short)                                                       # a row stride below the width
    refused(capi.camera(11, [1.0] * 12, 67, 45), target, images)                         # model id 11
    refused(source, capi.camera(11, [1.0] * 12, 67, 45), images)
    refused(source, None, images)                                                        # no target
    refused(source, None, images, H=np.eye(3))
    refused(capi.size_only_camera(67, 45), None, images)                                 # a size-only camera without H
    refused(capi.size_only_camera(67, 45), target, images, H=np.eye(3), dst=np.full((2, target.height, target.width), 0x5A, np.uint8))
    got = dsm.warp_images(source, target, images, out=out)
    assert got["images"] is out and (out == ref.warp_images(oracle, source, target, images)["images"]).all()


# ---- state ----
def test_repeat_and_no_stale_scratch(dsm, oracle):
    big_source = scenes.camera(5, 257, 40)
    big_target = dsm.undistort_cameras([big_source])[0]
    big = scenes.stack(257, 40, 3, 3)
    a = dsm.warp_images(big_source, big_target, big, return_map=True)
    b = dsm.warp_images(big_source, big_target, big, return_map=True)
    assert (a["images"] == b["images"]).all() and (a["source_xy"].view(np.uint64) == b["source_xy"].view(np.uint64)).all()
    # a small call on the scratch the larger one left
    source = scenes.camera(2, 13, 9)
    _check_warp(dsm, oracle, source, dsm.undistort_cameras([source])[0], scenes.stack(13, 9, 2, 1))
    _check_cameras(dsm, oracle, [scenes.camera(3, 9, 5)])
    t = dsm.undistortion_time()
    assert sorted(t) == sorted(capi.UNDISTORTION_STAGES) and all(v >= 0 for v in t.values()) and t["warp_kernel"] > 0


def test_budget_cuts_the_batch_into_chunks(oracle):
    source = scenes.camera(8, 130, 33)
    images = scenes.stack(130, 33, 7, 3)
    ctx = capi.Context(0)
    try:
        target = ctx.undistort_cameras([source])[0]
        whole = ctx.warp_images(source, target, images)["images"]
        _, scratch_whole = ctx.memory_footprint()
        per_image = 2 * 130 * 33 * 3
        assert scratch_whole >= 7 * per_image
        ctx.set_memory_budget(3 * per_image)  # two images a chunk: four chunks, the last of one image
        assert ctx.memory_footprint()[1] == 0
        chunked = ctx.warp_images(source, target, images)["images"]
        _, scratch = ctx.memory_footprint()
        assert 0 < scratch <= 3 * per_image
        assert (chunked == whole).all()
        ctx.set_memory_budget(1)  # one image always runs
        assert (ctx.warp_images(source, target, images, return_map=True)["images"] == whole).all()
    finally:
        ctx.close()
    assert (whole == ref.warp_images(oracle, source, target, images)["images"]).all()


# ---- the chain ----
def test_undistort_images_chain(dsm):
    cam = capi.camera(2, [100.0, 50.0, 50.0, 0.5], 100, 100)
    warped, und, owed = dsm.undistort_images(np.full((2, 100, 100), 255, np.uint8), cam)
    assert (und.model_id, und.width, und.height, und.params[2], und.params[3]) == (1, 84, 84, 42.0, 42.0)
    assert owed and warped.shape == (2, 100, 100) and not (warped == 0).any()
    warped, und, owed = dsm.undistort_images(np.full((1, 100, 100), 255, np.uint8), cam, blank_pixels=1)
    assert (und.width, und.height) == (90, 90) and owed and (warped == 0).any()
