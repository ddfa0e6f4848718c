"""Inputs of the undistortion tests: images made by integer arithmetic (sift_scenes.texture) and the camera list -- one
parameter vector per model from tests/test_camera_models.py (the reference's camera_models_test.cc), rescaled from its
800 x 800 pixel grid to the small sizes the tests use."""
import numpy as np

from dagsfm_amd import capi
from tests import sift_scenes

TWO_FOCAL = (1, 4, 5, 6, 7, 10)
# the most distorted vector of every model in test_camera_models.REFERENCE_TEST_PARAMS
MODEL_PARAMS = {
    0: [655.123, 386.123, 511.123],
    1: [651.123, 655.123, 386.123, 511.123],
    2: [651.123, 386.123, 511.123, 0.1],
    3: [651.123, 386.123, 511.123, 0.05, 0.03],
    4: [651.123, 655.123, 386.123, 511.123, -0.471, 0.223, -0.001, 0.001],
    5: [651.123, 655.123, 386.123, 511.123, -0.471, 0.223, -0.001, 0.001],
    6: [651.123, 655.123, 386.123, 511.123, -0.471, 0.223, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001],
    7: [651.123, 655.123, 386.123, 511.123, 0.9],
    8: [651.123, 386.123, 511.123, 0.1],
    9: [651.123, 386.123, 511.123, 0.05, 0.03],
    10: [651.123, 655.123, 386.123, 511.123, -0.471, 0.223, -0.001, 0.001, 0.001, 0.02, -0.02, 0.001],
}
MODELS = tuple(range(11))


def camera(model_id, width, height, params=None):
    """The model's reference parameter vector rescaled from 800 x 800 to width x height: the focal lengths and the principal
    point by the side they belong to (a single focal length by the longer side), the distortion parameters as they are."""
    p = list(MODEL_PARAMS[model_id] if params is None else params)
    sx, sy = width / 800.0, height / 800.0
    if model_id in TWO_FOCAL:
        p[0], p[1], p[2], p[3] = p[0] * sx, p[1] * sy, p[2] * sx, p[3] * sy
    else:
        p[0], p[1], p[2] = p[0] * max(sx, sy), p[1] * sx, p[2] * sy
    return capi.camera(model_id, p, width, height)


def grey(width, height, seed=1):
    """uint8 [height, width]; sift_scenes.texture needs a few pixels per side, so the smallest images are cut from a larger one."""
    return np.ascontiguousarray(sift_scenes.texture(max(width, 16), max(height, 16), seed)[:height, :width])


def rgb(width, height, seed=1):
    """uint8 [height, width, 3]: three textures of different seeds."""
    return np.ascontiguousarray(np.stack([grey(width, height, seed * 3 + k) for k in range(3)], axis=-1))


def stack(width, height, n, channels, seed=1):
    """uint8 [n, height, width] or [n, height, width, 3]."""
    make = grey if channels == 1 else rgb
    return np.ascontiguousarray(np.stack([make(width, height, seed + 7 * k) for k in range(n)]))


def with_row_padding(images, pad):
    """The same images as a view of a buffer whose rows are `pad` bytes longer (filled with 0xAB)."""
    images = np.asarray(images)
    n, h, w = images.shape[:3]
    c = images.shape[3] if images.ndim == 4 else 1
    buf = np.full((n, h, w * c + pad), 0xAB, np.uint8)
    buf[:, :, :w * c] = images.reshape(n, h, w * c)
    return buf[:, :, :w * c].reshape(images.shape)
