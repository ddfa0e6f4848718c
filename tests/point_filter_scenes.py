"""Scenes of the point-filter tests, shared by the CPU file (which holds every scene to the cap on unclear points)
and the GPU file: cameras on an arc looking at a cloud, tracks of chosen lengths, then planted trouble -- gross outliers, points
among and behind the cameras (observations of negative depth, some tracks with only a few of them), a far low-parallax group."""
import ctypes
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import bundle_adjustment_ref as ba
from tests import point_filter_ref as ref

P3, P4 = ([-0.5, -0.5, 1.0], [0, 1]), ([-0.6, -0.5, 1.0], [0, 1])  # the reference tests' points 3 and 4
WIDTH, HEIGHT = 640, 480  # bundle_adjustment_ref.DEFAULT_PARAMS: principal point (320, 240)


# The largest relative change of a clear point's error, or of one of the two means, when every input of a scene moves by one
# ulp: ref.error_sensitivity over every scene the GPU file compares (scenes() and around_the_cut()), under every pass mask that
# sets errors (2, 8, 2 | 4, 15), 3 seeded directions each.  Measured 4.35e-12 (the 1 024-observation scene under
# DSM_FILTER_MEAN_ERROR alone: nothing has been removed, so the points among the cameras are still there, whose shallow depths
# turn an ulp of a pose into many ulps of a pixel); with the other passes in front the worst is 3.72e-13.  Held to this bound
# by test_point_filter_cpu.py::test_error_sensitivity_constant; the GPU file allows 16 x for the device's atan / tan / acos
# and its unpinned orders.
ERROR_SENSITIVITY = 4.5e-12
ERROR_SENSITIVITY_PASSES = (2, 8, 2 | 4, 15)
ERROR_TOLERANCE = 16 * ERROR_SENSITIVITY


def unit_scene(num_images, points):
    """GenerateReconstruction (src/base/reconstruction_test.cc:43-66): one PINHOLE camera f = 1 at 1 x 1 (principal point
    0.5, 0.5), identity poses, every point2D at the origin.  points: (xyz, [image indices of the track])."""
    lens = [len(t) for _, t in points]
    return {"camera_model_ids": [1], "camera_params": [1.0, 1.0, 0.5, 0.5], "camera_width": [1], "camera_height": [1],
            "image_camera": np.zeros(num_images, np.uint32), "qvec": np.tile([1.0, 0, 0, 0], (num_images, 1)),
            "tvec": np.zeros((num_images, 3)), "xyz": np.array([x for x, _ in points], np.float64).reshape(-1, 3),
            "track_offsets": np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
            "obs_image": np.array([i for _, t in points for i in t], np.uint32), "obs_xy": np.zeros((sum(lens), 2))}


def reproject(s, points, rng, noise=0.5):
    """The observations of `points` recomputed from the scene's poses and intrinsics (behind a camera: left where they are)."""
    toff = s["track_offsets"]
    idx = np.concatenate([np.arange(int(toff[p]), int(toff[p + 1])) for p in points] + [np.zeros(0, np.int64)]).astype(np.int64)
    if not len(idx):
        return
    cams = ref.camera_list(s)
    R, _ = ref.image_poses(s["qvec"], s["tvec"])
    opoint = np.repeat(np.arange(len(toff) - 1), np.diff(toff.astype(np.int64)))
    for o in idx:
        i = int(s["obs_image"][o])
        pc = R[i].reshape(3, 3) @ s["xyz"][opoint[o]] + s["tvec"][i]
        if pc[2] < 0.1:
            continue
        m, pr, _, _ = cams[int(s["image_camera"][i])]
        x, y = ref.world_to_image(m, pr, np.array([pc[0] / pc[2]]), np.array([pc[1] / pc[2]]))
        s["obs_xy"][o] = [x[0] + noise * rng.normal(), y[0] + noise * rng.normal()]


def build(seed, n_images=12, lengths=None, n_points=120, models=(2,), max_track=8, outliers=0.08, near=0.08, far=0.08):
    """lengths: the track length of every point (None: n_points lengths drawn from 2 .. max_track).  outliers: the share of
    observations moved by tens of pixels; near: the share of points moved among the cameras (mixed depth signs); far: the
    share moved to a distance where no pair of views reaches the default 1.5 degrees."""
    rng = np.random.default_rng([seed, 0xF117])
    if lengths is None:
        lengths = rng.integers(2, min(max_track, n_images) + 1, n_points)
    lengths = np.asarray(lengths, np.int64)
    P = len(lengths)
    cam_models = list(models)
    icam = (np.arange(n_images) % len(cam_models)).astype(np.uint32)
    params = [np.array(ba.DEFAULT_PARAMS[m], np.float64) for m in cam_models]
    qs, ts = [], []
    for i in range(n_images):
        ang = 0.5 * (i / max(1, n_images - 1) - 0.5)
        pos = np.array([8.0 * np.sin(ang), 0.3 * rng.normal(), -8.0 * np.cos(ang)])
        R, t = ba._look_at(pos, rng.normal(scale=0.2, size=3))
        qs.append(ba.rot_to_quat(R) * rng.uniform(0.5, 2.0))  # not normalised: the filters normalise
        ts.append(t)
    oimg = np.concatenate([np.sort(rng.choice(n_images, size=int(L), replace=False)) for L in lengths] + [np.zeros(0, np.int64)])
    toff = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint32)
    s = {"camera_model_ids": np.array(cam_models, np.int32), "camera_params": np.concatenate(params),
         "camera_width": np.full(len(cam_models), WIDTH), "camera_height": np.full(len(cam_models), HEIGHT),
         "image_camera": icam, "qvec": np.array(qs), "tvec": np.array(ts), "point_ids": (rng.permutation(P) * 7 + 3).astype(np.uint64),
         "xyz": rng.uniform(-2.0, 2.0, (P, 3)), "track_offsets": toff, "obs_image": oimg.astype(np.uint32),
         "obs_xy": np.tile([100.0, 100.0], (len(oimg), 1))}
    kind = rng.random(P)
    for p in np.nonzero(kind < near)[0]:
        s["xyz"][p] = [rng.uniform(-5.0, 5.0), rng.uniform(-1.0, 1.0), rng.uniform(-9.5, -6.5)]
    for p in np.nonzero(kind > 1.0 - far)[0]:
        s["xyz"][p] = [rng.uniform(-50.0, 50.0), rng.uniform(-50.0, 50.0), rng.uniform(3000.0, 5000.0)]
    reproject(s, range(P), rng)
    s["xyz"] = s["xyz"] + rng.normal(scale=0.01, size=s["xyz"].shape) * (kind[:, None] <= 1.0 - far)
    bad = np.nonzero(rng.random(len(oimg)) < outliers)[0]
    s["obs_xy"][bad] += rng.uniform(20.0, 80.0, (len(bad), 2)) * rng.choice([-1.0, 1.0], (len(bad), 2))
    return s


def edge_lengths(seed, n_filler=40):
    """Every track length at which the code takes another path: 0 .. 3, around the lane / wave cut, one 300-view track."""
    rng = np.random.default_rng([seed, 0xED6E])
    c = ref.LANE_CUT
    special = [0, 1, 2, 3, c - 1, c, c + 1, 300, 0, 1, 2, 3, c - 1, c, c + 1, 40]
    L = np.concatenate([special, rng.integers(2, 9, n_filler)])
    return rng.permutation(L)


def with_observations(seed, n_obs, **kw):
    """A scene of exactly n_obs observations (the last track is cut short): the compaction scans n_obs + 1 flags."""
    rng = np.random.default_rng([seed, 0x0B5])
    lengths = []
    while sum(lengths) < n_obs:
        lengths.append(int(rng.integers(2, 9)))
    lengths[-1] -= sum(lengths) - n_obs
    return build(seed, lengths=lengths, **kw)


GRID_PASSES = (1, 2, 4, 8, 2 | 4, 15)  # what the GPU file runs on the "edge" and "models" scenes; the others run 15


def selections(s):
    """The selections the GPU file runs on the "models" scene: name -> keyword arguments of filter_points3D."""
    rng = np.random.default_rng(8)
    P, N = len(s["xyz"]), len(s["image_camera"])
    psel = rng.random(P) < 0.5
    isel = np.zeros(N, bool)
    isel[[3, 11]] = True
    return {"p": dict(point_selected=psel), "i": dict(image_selected=isel), "pi": dict(point_selected=psel, image_selected=isel),
            "none": dict(point_selected=np.zeros(P, bool))}


def comparisons():
    """Every (name, scene, passes, selection keywords) the GPU file compares with the restatement: the CPU file holds each of
    them to the cap on unclear points first."""
    every = scenes()
    a, b, _ = around_the_cut()
    out = [(n, every[n], m, {}) for n in ("edge", "models") for m in GRID_PASSES]
    out += [(n, s, 15, {}) for n, s in every.items() if n.startswith("obs")]
    out += [("models", every["models"], 15, kw) for kw in selections(every["models"]).values()]
    out += [("models", every["models"], 1, {}), ("cut_a", a, 15, {}), ("cut_b", b, 15, {})]
    return out


def scenes():
    """name -> scene: what the GPU file runs and the CPU file holds to the cap on unclear points."""
    out = {"edge": build(1, n_images=320, lengths=edge_lengths(1)),
           "models": build(2, n_images=22, n_points=150, models=tuple(range(11)))}
    for k, n_obs in enumerate((ref.SCAN_BLOCK - 2, ref.SCAN_BLOCK - 1, ref.SCAN_BLOCK, 3 * ref.SCAN_BLOCK + 77)):
        out["obs%d" % n_obs] = with_observations(10 + k, n_obs)
    return out


def around_the_cut(seed=5):
    """Two scenes whose tracks are the same after pass 1: A's tracks of LANE_CUT observations take the lane path; B gives every
    one of them a further observation, in an image that looks away from the cloud (negative depth: pass 1 removes it), so B's
    tracks take the wave path.  Returns (A, B, the number of points)."""
    c = ref.LANE_CUT
    a = build(seed, n_images=40, lengths=[c] * 32, near=0.0, far=0.25)
    b = {k: np.array(v, copy=True) for k, v in a.items()}
    cloud = a["xyz"][np.abs(a["xyz"][:, 2]) < 10].mean(0)
    pos = np.array([0.0, 0.0, -8.0])
    R, t = ba._look_at(pos, pos - (cloud - pos))  # the extra image: at a camera's place, facing the other way
    b["qvec"] = np.vstack([a["qvec"], ba.rot_to_quat(R)])
    b["tvec"] = np.vstack([a["tvec"], t])
    b["image_camera"] = np.append(a["image_camera"], 0).astype(np.uint32)
    extra = len(a["image_camera"])
    P = len(a["xyz"])
    oimg = np.concatenate([np.append(a["obs_image"][c * p:c * (p + 1)], extra) for p in range(P)])
    oxy = np.concatenate([np.vstack([a["obs_xy"][c * p:c * (p + 1)], [[320.0, 240.0]]]) for p in range(P)])
    b.update(obs_image=oimg.astype(np.uint32), obs_xy=oxy, track_offsets=(np.arange(P + 1) * (c + 1)).astype(np.uint32))
    return a, b, P


def check_refusals(ctx):
    s = unit_scene(2, [P3, P4])
    ok = ctx.filter_points3D(s, passes=2, max_reproj_error=0.09)
    assert ok["point_keep"].tolist() == [True, False]

    def bad(text, **change):
        t = dict(s)
        kw = {k[1:]: v for k, v in change.items() if k.startswith("_")}
        t.update({k: v for k, v in change.items() if not k.startswith("_")})
        with pytest.raises(capi.DsmError) as e:
            ctx.filter_points3D(t, **kw)
        assert "dsm_filter_points3D" in str(e.value) and text in str(e.value), str(e.value)

    bad("start at 0", track_offsets=[1, 2, 4])
    bad("ascend", track_offsets=[0, 3, 2])
    bad("out of range", obs_image=[0, 1, 0, 2])
    bad("out of range", image_camera=[0, 1])
    bad("unknown camera model", camera_model_ids=[11], camera_params=[])
    bad("non-finite", xyz=[[np.nan, 0, 1], [0, 0, 1]])
    bad("non-finite", obs_xy=[[0, 0], [0, np.inf], [0, 0], [0, 0]])
    bad("non-finite", tvec=[[0, 0, 0], [0, np.nan, 0]])
    bad("non-finite", qvec=[[1, 0, 0, 0], [np.inf, 0, 0, 0]])
    bad("non-finite", camera_params=[1.0, np.nan, 0.5, 0.5])
    bad("zero qvec", qvec=[[1, 0, 0, 0], [0, 0, 0, 0]])
    bad("unregistered", image_registered=[1, 0])
    bad("passes", _passes=0)
    bad("passes", _passes=16)
    for key in ("max_reproj_error", "min_tri_angle", "min_focal_length_ratio", "max_focal_length_ratio", "max_extra_param"):
        bad("threshold", **{"_" + key: -1.0})
        bad("threshold", **{"_" + key: math.inf})
        bad("threshold", **{"_" + key: math.nan})
    L = ctx._L
    o = capi.default_point_filter_options()
    z = np.zeros(4, np.uint32)
    assert L.dsm_filter_points3D(ctx._h, 0, None, 0, None, None, None, None, 0, None, None, None, None, None, None, ctypes.byref(o),
                                 *([None] * 7)) != 0 and b"NULL" in L.dsm_last_error(ctx._h)
    assert L.dsm_filter_points3D(ctx._h, 0, None, 0, None, None, None, None, 1, None, z.ctypes.data, None, None, None, None,
                                 ctypes.byref(o), *([None] * 7)) != 0 and b"NULL" in L.dsm_last_error(ctx._h)
    assert ctx.filter_points3D(s, passes=2, max_reproj_error=0.09)["point_keep"].tolist() == [True, False]  # the context is still usable
