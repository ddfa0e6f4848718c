"""CPU-only: the numpy restatement of the undistortion stage (tests/undistortion_ref.py) held to the reference's own known
answers -- undistortion_test.cc:40-213 and warp_test.cc:91-220 -- and the binding of the new entry points (struct sizes,
defaults, every new symbol exported by both builds).  The GPU tests compare the device with this restatement."""
import ctypes
import os

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import undistortion_ref as ref
from tests import undistortion_scenes as scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _initialized(model_id, focal, width, height):
    """Camera::InitializeWithId: the focal length(s), the principal point at the centre, every other parameter 0."""
    n = capi.CAMERA_MODEL_NUM_PARAMS[model_id]
    two = model_id in ref.TWO_FOCAL
    p = ([focal, focal] if two else [focal]) + [width / 2.0, height / 2.0]
    return capi.camera(model_id, p + [0.0] * (n - len(p)), width, height)


def _radial100():
    cam = _initialized(2, 100, 100, 100)
    cam.params[3] = 0.5
    return cam


def _pinhole(cam):
    return (cam.model_id, cam.params[0], cam.params[1], cam.params[2], cam.params[3], cam.width, cam.height)


# ---- undistortion_test.cc:40-101 ----
def test_simple_pinhole_1x1(oracle):
    u = ref.undistort_camera(oracle, _initialized(0, 1, 1, 1))
    assert (u.model_id, u.params[0], u.params[1], u.width, u.height) == (1, 1, 1, 1, 1)


def test_simple_radial_1x1_goes_through_nan(oracle):
    """inf * 0 = NaN in the interpolated scale; Clip(NaN) = min_scale, and max(1.0, 0.2 * 1) = 1."""
    u = ref.undistort_camera(oracle, _initialized(2, 1, 1, 1))
    assert (u.model_id, u.params[0], u.params[1], u.width, u.height) == (1, 1, 1, 1, 1)
    assert ref.clip(float("nan"), 0.2, 2.0) == 0.2
    # the arguments the other way round would have kept the NaN out of min and taken max_scale
    assert max(0.2, min(2.0, float("nan"))) == 2.0


def test_simple_radial_100(oracle):
    u = ref.undistort_camera(oracle, _radial100())
    assert _pinhole(u) == (1, 100, 100, 84.0 / 2.0, 84.0 / 2.0, 84, 84)


def test_simple_radial_100_blank_pixels(oracle):
    u = ref.undistort_camera(oracle, _radial100(), blank_pixels=1)
    assert _pinhole(u) == (1, 100, 100, 90.0 / 2.0, 90.0 / 2.0, 90, 90)


def test_simple_radial_100_max_scale(oracle):
    u = ref.undistort_camera(oracle, _radial100(), blank_pixels=1, max_scale=0.75)
    assert (u.model_id, u.params[0], u.params[1], u.width, u.height) == (1, 100, 100, 75, 75)


def test_simple_radial_100_roi(oracle):
    u = ref.undistort_camera(oracle, _radial100(), blank_pixels=1, max_scale=1.0, roi_min_x=0.1, roi_min_y=0.2, roi_max_x=0.9,
                             roi_max_y=0.8)
    assert _pinhole(u) == (1, 100, 100, 40, 30, 80, 60)


# ---- undistortion_test.cc:103-178, at the source resolution ----
@pytest.mark.parametrize("blank_pixels,zeros", [(1, True), (0, False)])
def test_blank_pixels_of_a_filled_image(oracle, blank_pixels, zeros):
    cam = _radial100()
    und = ref.undistort_camera(oracle, cam, blank_pixels=blank_pixels)
    assert (und.width, und.height) == ((90, 90) if blank_pixels else (84, 84))
    r = ref.warp_images(oracle, cam, und, np.full((1, 100, 100), 255, np.uint8))
    assert r["needs_rescale"] and (r["scaled_target"].width, r["scaled_target"].height) == (100, 100)
    assert r["images"].shape == (1, 100, 100)
    assert bool((r["images"] == 0).any()) == zeros
    assert (r["images"][r["images"] != 0] == 255).all()


# ---- undistortion_test.cc:180-213 ----
def test_undistort_reconstruction_moves_the_points(oracle):
    cam = _initialized(4, 1, 1, 1)
    cam.params[4] = 1.0
    und = ref.undistort_camera(oracle, cam)
    assert und.model_id == 1
    xy = ref.undistort_points2D(oracle, [cam], [und], np.zeros(10, np.uint32), np.ones((10, 2)))
    assert (xy != 1.0).all() and np.isfinite(xy).all() and (xy == xy[0]).all()


# ---- warp_test.cc:91-220 ----
def _random_images(channels):
    rng = np.random.default_rng(channels)
    return rng.integers(0, 256, (1, 100, 100) + ((3,) if channels == 3 else ()), dtype=np.uint8)


@pytest.mark.parametrize("channels", [1, 3])
def test_identical_cameras_reproduce_the_interior(oracle, channels):
    cam = _initialized(1, 1, 100, 100)
    src = _random_images(channels)
    r = ref.warp_images(oracle, cam, cam, src)
    assert not r["needs_rescale"]
    assert (r["images"][0, 1:-1, 1:-1] == src[0, 1:-1, 1:-1]).all()
    # the sample needs the pixel to the right and the scanline above: the last column and the first row are refused
    assert (r["images"][0, :, -1] == 0).all() and (r["images"][0, 0, :] == 0).all()


def test_shifted_principal_point(oracle):
    source = _initialized(1, 1, 100, 100)
    target = _initialized(1, 1, 100, 100)
    target.params[2] = 0.0
    src = _random_images(1)
    out = ref.warp_images(oracle, source, target, src)["images"][0]
    assert (out[1:, :49] == src[0, 1:, 50:99]).all()
    assert (out[:, 50:] == 0).all()


@pytest.mark.parametrize("with_cameras", [False, True])
@pytest.mark.parametrize("channels", [1, 3])
def test_identity_homography(oracle, channels, with_cameras):
    cam = _initialized(1, 1, 100, 100) if with_cameras else capi.size_only_camera(100, 100)
    src = _random_images(channels)
    out = ref.warp_images(oracle, cam, cam if with_cameras else None, src, H=np.eye(3))["images"]
    assert (out[0, 1:-1, 1:-1] == src[0, 1:-1, 1:-1]).all()


@pytest.mark.parametrize("with_cameras", [False, True])
def test_transposing_homography(oracle, with_cameras):
    src = _random_images(3)
    H = np.array([[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    if with_cameras:
        # K^-1 . K is exact for focal length 1 and the principal point (50, 50) on the pixel centres x + 0.5
        cam = _initialized(1, 1, 100, 100)
        out = ref.warp_images(oracle, cam, cam, src, H=H)["images"]
    else:
        out = ref.warp_images(oracle, capi.size_only_camera(100, 100), None, src, H=H)["images"]
    assert (out[0, 1:-1, 1:-1] == src[0].transpose(1, 0, 2)[1:-1, 1:-1]).all()


def test_float_step_decides_ties():
    """The interpolated double goes through float before std::round: 0.5 - 2^-30 rounds to 0 as a double and to 1 as a float."""
    im = np.array([[0, 0], [0, 1]], np.uint8)
    # dy = 0 puts all weight on scanline y0 = 0, the bottom row; dx just below one half
    dx = 0.5 - 2.0 ** -30
    out = ref.interpolate_bilinear_u8(im, np.array([dx + 0.5]), np.array([1.0 + 0.5]))
    assert float(np.float32(dx)) == 0.5 and round(dx) == 0
    assert out[0] == 1
    # a NaN, a coordinate outside int and one outside the image write 0
    bad = ref.interpolate_bilinear_u8(np.full((4, 4), 255, np.uint8), np.array([np.nan, 1e300, -3e9, 7.0, 1.5]),
                                      np.array([1.5, 1.5, 1.5, 1.5, 1.5]))
    assert list(bad) == [0, 0, 0, 0, 255]


def test_rescale_to_size():
    cam = capi.camera(2, [100.0, 40.0, 30.0, 0.1], 80, 60)
    c = ref.rescale_to_size(cam, 40, 90)
    assert (c.width, c.height, c.params[0], c.params[1], c.params[2], c.params[3]) == (40, 90, (0.5 + 1.5) / 2.0 * 100.0, 20.0, 45.0, 0.1)
    c = ref.rescale_by(capi.camera(1, [100.0, 100.0, 40.0, 30.0], 80, 60), 0.26)
    assert (c.width, c.height) == (21, 16) and c.params[0] == 21 / 80 * 100.0 and c.params[3] == 16 / 60 * 30.0


# ---- the binding ----
def test_struct_and_defaults():
    assert ctypes.sizeof(capi.UndistortOptions) == 64
    assert ctypes.sizeof(capi.Camera) == 120
    o = capi.default_undistort_options()
    assert (o.blank_pixels, o.min_scale, o.max_scale, o.max_image_size, o.roi_min_x, o.roi_min_y, o.roi_max_x, o.roi_max_y) == \
        (0.0, 0.2, 2.0, -1, 0.0, 0.0, 1.0, 1.0)
    assert capi.default_undistort_options(blank_pixels=0.5, max_image_size=640).max_image_size == 640
    d = ref.default_options()
    assert all(getattr(o, k) == v for k, v in d.items())
    assert capi.size_only_camera(7, 9).model_id == capi.CAMERA_SIZE_ONLY == ref.SIZE_ONLY == -1
    header = open(os.path.join(ROOT, "include", "dagsfm_mi355x.h")).read()
    assert "#define DSM_UNDISTORTION_STAGES %d" % len(capi.UNDISTORTION_STAGES) in header
    assert "#define DSM_CAMERA_SIZE_ONLY (-1)" in header


def test_both_builds_export_the_new_symbols():
    for path in (capi.LIB_PATH, capi.CHECK_LIB_PATH):
        lib = ctypes.CDLL(path)
        for s in ("dsm_default_undistort_options", "dsm_undistort_cameras", "dsm_undistort_points2D", "dsm_warp_images",
                  "dsm_get_undistortion_time"):
            assert hasattr(lib, s), "missing export in %s: %s" % (os.path.basename(path), s)


def test_scene_helpers():
    im = scenes.stack(13, 5, 2, 3)
    assert im.shape == (2, 5, 13, 3) and im.dtype == np.uint8 and len(np.unique(im)) > 8
    pad = scenes.with_row_padding(im, 5)
    assert (pad == im).all() and pad.strides == (5 * (39 + 5), 39 + 5, 3, 1)
    cam = scenes.camera(4, 67, 45)
    assert (cam.width, cam.height) == (67, 45) and cam.params[2] == 386.123 * 67 / 800.0 and cam.params[4] == -0.471
