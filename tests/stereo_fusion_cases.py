"""The fusion cases of the CPU and GPU tests: the scenes of tests/patch_match_scenes.py with their truth depth
and normal maps as fusion's input, every image listing all others (so a traversal re-enters the current image), and the
restatement's result of each, computed once per process."""
import functools

import numpy as np

from dagsfm_amd import capi
from tests import patch_match_scenes as scenes
from tests import stereo_fusion_ref as ref

# name: (kind, sizes, options, depth noise, holes, bitmap factor of image 1)
CASES = {
    "slanted": ("slanted", [(37, 23)] * 4, {}, 0.0, 0.0, 1),
    "step_sizes": ("step", [(37, 23), (23, 37), (30, 26), (37, 23)], {}, 0.0, 0.0, 1),
    "step_max_pixels": ("step", [(37, 23)] * 4, {"max_num_pixels": 3, "min_num_pixels": 2}, 0.0, 0.0, 1),
    "slanted_depth_limit": ("slanted", [(37, 23)] * 4, {"max_traversal_depth": 2, "min_num_pixels": 2}, 0.0, 0.0, 1),
    "slanted_wave_edge": ("slanted", [(65, 9), (37, 23), (23, 37)], {"min_num_pixels": 2}, 0.0, 0.0, 1),
    "step_noise_holes": ("step", [(37, 23)] * 5, {}, 0.004, 0.10, 1),
    "slanted_80x60": ("slanted", [(80, 60)] * 4, {}, 0.002, 0.0, 1),
    # a bitmap twice the size of the depth map (image 1), as max_image_size leaves it for the depth maps only
    "slanted_bitmap_2x": ("slanted", [(37, 23)] * 4, {}, 0.0, 0.0, 2),
    # clusters of one or two pixels: a fused point is a pixel's back-projection or the midpoint of two (test_stereo_fusion_cpu)
    "slanted_pairs": ("slanted", [(37, 23)] * 4, {"max_num_pixels": 2, "min_num_pixels": 1}, 0.0, 0.0, 1),
}
TABLE = ("slanted", "step_sizes", "step_max_pixels", "slanted_depth_limit", "slanted_wave_edge", "step_noise_holes", "slanted_80x60")
DEFAULT_CASES = ("slanted", "step_sizes", "step_noise_holes", "slanted_80x60")
SLANTED_PLANE = (np.array([0.35, -0.2, -1.0]) / np.linalg.norm([0.35, -0.2, -1.0]), 4.0)  # n . X = -d (patch_match_scenes.make_scene)


def make_images(kind, sizes, noise=0.0, holes=0.0, bitmap_factor=1, seed=0):
    views, truth = scenes.make_scene(kind, sizes=sizes, n_views=len(sizes), seed=seed)
    rng = np.random.RandomState(1234 + seed)
    images = []
    for i, (v, t) in enumerate(zip(views, truth)):
        depth = t["depth"].copy()
        if noise:
            depth *= 1.0 + noise * rng.standard_normal(depth.shape)
        if holes:
            depth[rng.uniform(size=depth.shape) < holes] = 0.0
        depth = np.where(np.isfinite(depth), depth, 0.0).astype(np.float32)
        grey = v["data"]
        rgb = np.stack([grey, 255 - grey, (grey // 2) + 17 * i], axis=-1).astype(np.uint8)
        factor = bitmap_factor if i == 1 else 1
        if factor != 1:
            rgb = np.repeat(np.repeat(rgb, factor, axis=0), factor, axis=1)
        h, w = depth.shape
        sx, sy = np.float32(w) / np.float32(rgb.shape[1]), np.float32(h) / np.float32(rgb.shape[0])
        K = v["K"].astype(np.float32).copy()
        if factor != 1:  # the camera of the bitmap: the depth map's is its scaled one (fusion.cc:223-226)
            K[[0, 2]] /= sx
            K[[4, 5]] /= sy
        P, inv_P, inv_R = capi.fusion_matrices(K, v["R"], v["T"], sx, sy)
        images.append({"used": True, "depth": depth, "normal": t["normal"].astype(np.float32), "rgb": np.ascontiguousarray(rgb),
                       "P": P, "inv_P": inv_P, "inv_R": inv_R, "scale": np.array([sx, sy], dtype=np.float32)})
    return images


def all_others(n):
    """Every image lists all others, the next index first: the children of a pixel include the current image again."""
    return [[(i + k) % n for k in range(1, n)] for i in range(n)]


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (images, overlap, options) of a named case."""
    kind, sizes, options, noise, holes, factor = CASES[name]
    return make_images(kind, list(sizes), noise, holes, factor), all_others(len(sizes)), dict(options)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's result of a named case (sequential schedule), computed once and left unchanged."""
    images, overlap, options = case(name)
    return ref.fuse(images, overlap, options)


def same_result(got, want):
    """points, colours, normals, visibility of capi against the restatement's dict: equal on the bits."""
    points, colours, normals, vis = got[:4]
    return (points.shape == want["points"][:, :3].shape and points.tobytes() == want["points"][:, :3].tobytes()
            and normals.tobytes() == np.ascontiguousarray(want["points"][:, 3:]).tobytes()
            and colours.tobytes() == want["colours"].tobytes() and [list(v) for v in vis] == want["visibility"])
