"""Named scenes for the global bundle adjustment's edge tests: cameras shared by some of the images, the
constant-tvec masks, the exits, the block edges of the device's tiles and gaps in the image and camera lists.
comparisons() is the list of (name, scene, options) that tests/test_bundle_adjustment_edges_gpu.py compares with the
restatement under the strict rule; tests/test_bundle_adjustment_edges_cpu.py holds what the restatement alone must satisfy
on the same list (as local_bundle_scenes.comparisons() does for the local bundle)."""
import functools

import numpy as np

from tests.bundle_adjustment_ref import NUM_PARAMS, make_scene

GROUP_OPTIONS = dict(max_num_iterations=5, refine_extra_params=0)  # a group's distortion is ill-posed on most of these
EXIT_TOLERANCE_OPTIONS = dict(gradient_tolerance=1e-10, max_num_iterations=30)
# the first seeds 530 + P + 1000 j that the restatement calls clear (531 and 785 are not stable under the conditioning probe)
POINT_SEEDS = {1: 1531, 2: 532, 255: 1785, 256: 786, 257: 787}
NF_IMAGES = 42
NF_257_SEED = 627  # the first seed from 622 on that the restatement calls clear (622 .. 626 are not stable under the probe)


def groups():
    """Two to four cameras, each shared by several images but not by all: camera runs of length >= 2 inside a track."""
    g = dict(n_points=300, shared=True, arc=1.5)
    s = {600: make_scene(600, n_images=6, models=(2, 4), **g), 601: make_scene(601, n_images=7, models=(0, 3, 6), **g),
         602: make_scene(602, n_images=9, models=(8, 1), **g), 603: make_scene(603, n_images=8, models=(5, 7, 9, 10), **g),
         604: make_scene(604, n_images=6, n_points=200, models=(2, 2), shared=True, arc=1.0)}
    out = [("groups_%d" % k, s[k], GROUP_OPTIONS) for k in sorted(s)]
    for k in (602, 604):  # the two whose distortion is well-posed
        out.append(("groups_%d_extra" % k, s[k], dict(GROUP_OPTIONS, refine_extra_params=1)))
    return out


MASKED_IMAGE = 3


def masks():
    out = []
    for m in range(2, 8):
        s = make_scene(510 + m, n_images=6, n_points=100)
        s["image_constant_tvec"][MASKED_IMAGE] = m
        out.append(("mask_%d" % m, s, dict(max_num_iterations=10)))
    return out


def exits():
    s = make_scene(520, n_points=100)
    return [("exit_function_tolerance", s, dict(EXIT_TOLERANCE_OPTIONS, function_tolerance=1e-3)),
            ("exit_parameter_tolerance", s, dict(EXIT_TOLERANCE_OPTIONS, parameter_tolerance=1e-4)),
            ("exit_cg_cap_3", s, dict(max_num_iterations=6, max_linear_solver_iterations=3)),
            ("exit_cg_cap_1", s, dict(max_num_iterations=6, max_linear_solver_iterations=1)),
            ("exit_cg_past_two_resets", make_scene(521, n_images=12, n_points=150, models=(6,), arc=1.2),
             dict(max_num_iterations=6, gradient_tolerance=1e-8))]


def nf_scene(seed, models):
    return make_scene(seed, n_images=NF_IMAGES, n_points=150, models=models, shared=True, arc=1.5, min_track=3, max_track=8)


def edges():
    run = dict(max_num_iterations=10)
    out = [("points_%d" % P, make_scene(POINT_SEEDS[P], n_points=P), run) for P in (1, 2, 255, 256, 257)]
    t4 = dict(min_track=4, max_track=4)
    out.append(("observations_256", make_scene(540, n_points=64, **t4), run))
    out.append(("observations_512", make_scene(541, n_points=128, **t4), run))
    out.append(("image_observations_64", make_scene(543, n_images=4, n_points=64, **t4), run))
    out.append(("image_observations_65", make_scene(544, n_images=4, n_points=65, **t4), run))
    # the device's f columns: 6 per image (fixed width) and the cameras' free parameters, here their focal lengths
    out.append(("nf_255", nf_scene(621, (0, 1)), GROUP_OPTIONS))
    out.append(("nf_256", nf_scene(620, (4, 4)), GROUP_OPTIONS))
    out.append(("nf_257", nf_scene(NF_257_SEED, (1, 1, 0)), GROUP_OPTIONS))
    return out


NF_EXPECTED = {"nf_255": 255, "nf_256": 256, "nf_257": 257}
GAP_IMAGE, GAP_CAMERA = 2, 1
GAP_QVEC, GAP_TVEC, GAP_PARAMS = [2.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [300.0, 1.0, 2.0]


def with_gaps(scene):
    """The scene with an image without observations inserted at GAP_IMAGE and a SIMPLE_PINHOLE camera that no image uses at
    GAP_CAMERA: an empty segment before live ones in the image and the camera lists."""
    poff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in scene["camera_model_ids"]])])
    icam = scene["image_camera"].astype(np.int64)
    icam = icam + (icam >= GAP_CAMERA)
    oimg = scene["obs_image"].astype(np.int64)
    out = dict(scene)
    out.update(camera_model_ids=np.insert(scene["camera_model_ids"], GAP_CAMERA, 0).astype(np.int32),
               camera_params=np.insert(scene["camera_params"], poff[GAP_CAMERA], GAP_PARAMS),
               image_camera=np.insert(icam, GAP_IMAGE, 0).astype(np.uint32),
               qvec=np.insert(scene["qvec"], GAP_IMAGE, GAP_QVEC, axis=0), tvec=np.insert(scene["tvec"], GAP_IMAGE, GAP_TVEC, axis=0),
               image_constant_pose=np.insert(scene["image_constant_pose"], GAP_IMAGE, 0).astype(np.uint8),
               image_constant_tvec=np.insert(scene["image_constant_tvec"], GAP_IMAGE, 0).astype(np.uint8),
               obs_image=(oimg + (oimg >= GAP_IMAGE)).astype(np.uint32))
    return out


def without_gaps(out, scene):
    """The blocks of a run on with_gaps(scene) that belong to `scene`, in its order."""
    poff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in scene["camera_model_ids"]])])
    at = poff[GAP_CAMERA]
    return {"qvec": np.delete(out["qvec"], GAP_IMAGE, axis=0), "tvec": np.delete(out["tvec"], GAP_IMAGE, axis=0), "xyz": out["xyz"],
            "camera_params": np.delete(out["camera_params"], np.arange(at, at + len(GAP_PARAMS)))}


def gaps():
    name, s, opt = groups()[0]
    return [("gaps_in_groups_600", with_gaps(s), opt)]


def failure_scene():
    """An arithmetic infinity in the initial cost: image 2 at the identity pose observes a point in its plane z = 0."""
    s = make_scene(550, n_points=20)
    img = 2
    toff = s["track_offsets"].astype(np.int64)
    p = next(p for p in range(20) if img in s["obs_image"][toff[p]:toff[p + 1]])
    s["qvec"][img], s["tvec"][img], s["xyz"][p] = [1.0, 0.0, 0.0, 0.0], 0.0, [1.0, 1.0, 0.0]
    return s


KINDS = (("groups", groups), ("masks", masks), ("exits", exits), ("edges", edges), ("gaps", gaps))


@functools.lru_cache(maxsize=None)
def of_kind(kind):
    return tuple(dict(KINDS)[kind]())


def comparisons():
    """(name, scene, options) of every comparison of the device with the restatement under the strict rule.  Built once
    and shared: nothing may change a scene of this list."""
    return tuple(entry for kind, _ in KINDS for entry in of_kind(kind))


def permuted_images_and_cameras(scene, seed):
    """The same problem with its images and cameras listed in another order.  Returns the scene, the image permutation ip
    (new image r is old image ip[r]) and the camera permutation cp."""
    rng = np.random.default_rng(seed)
    N, C = len(scene["image_camera"]), len(scene["camera_model_ids"])
    ip, cp = rng.permutation(N), rng.permutation(C)
    iinv, cinv = np.empty(N, np.int64), np.empty(C, np.int64)
    iinv[ip], cinv[cp] = np.arange(N), np.arange(C)
    poff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in scene["camera_model_ids"]])])
    out = dict(scene, camera_model_ids=scene["camera_model_ids"][cp],
               camera_params=np.concatenate([scene["camera_params"][poff[c]:poff[c + 1]] for c in cp]),
               image_camera=cinv[scene["image_camera"][ip]].astype(np.uint32), qvec=scene["qvec"][ip], tvec=scene["tvec"][ip],
               image_constant_pose=scene["image_constant_pose"][ip], image_constant_tvec=scene["image_constant_tvec"][ip],
               obs_image=iinv[scene["obs_image"]].astype(np.uint32))
    return out, ip, cp


def camera_blocks(params, models, cp):
    """camera_params of cameras `models` re-listed in the order cp."""
    poff = np.concatenate([[0], np.cumsum([NUM_PARAMS[m] for m in models])])
    return np.concatenate([params[poff[c]:poff[c + 1]] for c in cp])
