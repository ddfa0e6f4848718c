"""Scenes for the local bundle adjustment tests and the list of comparisons the GPU file makes with the
restatement; the CPU file computes the restatement's verdict on the same list (as point_filter_scenes.comparisons() does)."""
import numpy as np

from tests.bundle_adjustment_ref import make_scene

SOFT_L1, CAUCHY, TRIVIAL = 1, 2, 0


def local_scene(seed, n_config=6, n_outside=0, n_points=60, models=(2,), shared=True, min_track=2, max_track=None, noise=0.5,
                const_point_frac=0.0, arc=0.5, single_tracks=0):
    """A problem shaped like the mapper's: n_config images with the gauge of AdjustLocalBundle (the last one constant-pose,
    tvec[0] of the one before it constant; with two images the second is constant and tvec[0] of the first), then n_outside
    constant-pose images with constant cameras of their own.  single_tracks: that many points keep one observation only."""
    n_img = n_config + n_outside
    s = make_scene(seed, n_images=n_img, n_points=n_points, models=models, shared=shared, noise=noise, min_track=min_track,
                   max_track=max_track, const_point_frac=const_point_frac, gauge=False, arc=arc)
    cpose, cmask = np.zeros(n_img, np.uint8), np.zeros(n_img, np.uint8)
    cpose[n_config - 1] = 1
    cmask[n_config - 2] = 1
    cpose[n_config:] = 1
    C = len(s["camera_model_ids"])
    cconst = np.zeros(C, np.uint8)
    if n_outside and not shared:
        cconst[n_config:] = 1
    s.update(image_constant_pose=cpose, image_constant_tvec=cmask, camera_constant=cconst)
    if single_tracks:
        toff = np.asarray(s["track_offsets"], np.int64)
        keep = np.ones(toff[-1], bool)
        for p in range(single_tracks):
            keep[toff[p] + 1:toff[p + 1]] = False
        s["track_offsets"] = np.concatenate([[0], np.cumsum([keep[toff[p]:toff[p + 1]].sum() for p in range(len(toff) - 1)])]).astype(np.uint32)
        s["obs_image"], s["obs_xy"] = s["obs_image"][keep], s["obs_xy"][keep]
    return s


def reduced_dim_scene(over):
    """Per-image FULL_OPENCV cameras with the principal point free: 12 free parameters, 18 columns per variable-pose image.
    over = False: 5 variable-pose images (90) + the tvec[0]-fixed image (17) + a constant-pose FULL_OPENCV image (12) + three
    constant-pose images with SIMPLE_PINHOLE cameras of their own (3 + 3 + 3) = 128 columns.  (SIMPLE_PINHOLE, because with the
    principal point free a SIMPLE_RADIAL camera frees 4 parameters: f, cx, cy, k.)
    over = True: 6 variable-pose images (108) + the tvec[0]-fixed image (17) + one constant-pose SIMPLE_RADIAL camera (4) = 129."""
    models = [6] * 7 + [0, 0, 0] if not over else [6] * 7 + [2]
    n_var = 5 if not over else 6
    n_img = len(models)
    s = make_scene(77, n_images=n_img, n_points=90, models=tuple(models), shared=False, noise=0.3, min_track=3, gauge=False, arc=0.9)
    cpose, cmask = np.zeros(n_img, np.uint8), np.zeros(n_img, np.uint8)
    cmask[n_var] = 1
    cpose[n_var + 1:] = 1
    s.update(image_constant_pose=cpose, image_constant_tvec=cmask, camera_constant=np.zeros(n_img, np.uint8))
    return s


REDUCED_DIM_OPTIONS = dict(refine_principal_point=1, max_num_iterations=3)

MODEL_NAMES = ["SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE", "FULL_OPENCV", "FOV",
               "SIMPLE_RADIAL_FISHEYE", "RADIAL_FISHEYE", "THIN_PRISM_FISHEYE"]


def comparisons():
    """(name, scene, options) of every comparison of the device with the restatement.  gradient_tolerance is lowered so that
    the runs take steps (the default 10 ends most of these small problems at iteration 0)."""
    out = []
    run = dict(gradient_tolerance=1e-3, max_num_iterations=6)
    for n_config in (2, 3, 6):
        for n_outside in (0, 4):
            out.append(("config%d_outside%d" % (n_config, n_outside),
                        local_scene(10 + n_config + n_outside, n_config, n_outside, n_points=40, max_track=n_config + n_outside), run))
    for n_points in (1, 7, 8, 9, 63, 64, 65, 255, 257):  # the tile of 8 staged points, a wave, the workgroup's stride of 256
        out.append(("points%d" % n_points, local_scene(30 + n_points, 3, 0, n_points=n_points), run))
    out.append(("tracks_1_2_3", local_scene(50, 3, 0, n_points=30, min_track=2, max_track=3, single_tracks=6), run))
    out.append(("tracks_16_17", local_scene(51, 3, 14, n_points=24, min_track=16, max_track=17, arc=1.2), run))
    for m in range(11):  # every model shared by all images, its distortion free
        out.append(("shared_" + MODEL_NAMES[m], local_scene(60 + m, 6, 0, n_points=60, models=(m,), arc=1.0), run))
    out.append(("per_image_focal", local_scene(80, 6, 0, n_points=60, models=(2, 0, 3), shared=False, arc=1.0),
                dict(run, refine_extra_params=0)))
    for name, kind in (("trivial", TRIVIAL), ("soft_l1", SOFT_L1), ("cauchy", CAUCHY)):
        out.append(("loss_" + name, local_scene(90, 4, 2, n_points=50, noise=1.5), dict(run, loss_function_type=kind)))
    for name, kind in (("trivial", TRIVIAL), ("soft_l1", SOFT_L1), ("cauchy", CAUCHY)):  # a second scene per loss, per-image cameras
        out.append(("loss_%s_per_image" % name, local_scene(95, 5, 3, n_points=70, models=(2, 0, 3), shared=False, noise=1.0, arc=1.0),
                    dict(run, loss_function_type=kind, refine_extra_params=0, max_num_iterations=3 if kind == TRIVIAL else 6)))
    # (the trivial loss converges quadratically: by the sixth iteration cost change and model change are both rounding and
    # the acceptance test has no margin, which is what makes loss_trivial above not clear; three iterations stay clear)
    s = local_scene(91, 4, 0, n_points=40)
    s["point_constant"] = np.ones(40, np.uint8)
    out.append(("no_variable_point", s, run))
    s = local_scene(92, 4, 0, n_points=40)
    s["image_constant_pose"] = np.ones(4, np.uint8)
    s["camera_constant"] = np.ones(1, np.uint8)
    out.append(("no_variable_camera_side", s, run))
    out.append(("constant_points_mixed", local_scene(93, 5, 3, n_points=50, const_point_frac=0.4), run))
    out.append(("default_options", local_scene(94, 6, 4, n_points=80, noise=2.0), {}))
    # cameras shared by some of the images, outside ones among them: image i has camera i % len(models), none is constant
    out.append(("groups_2_cameras", local_scene(96, 6, 3, n_points=60, models=(2, 4), arc=1.0), dict(run, refine_extra_params=0)))
    out.append(("groups_3_cameras", local_scene(96, 7, 2, n_points=60, models=(0, 3, 1), arc=1.0), dict(run, refine_extra_params=0)))
    return out
