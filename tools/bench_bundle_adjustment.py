#!/usr/bin/env python3
"""Global bundle adjustment (dsm_bundle_adjust) on one MI355X over a seeded synthetic merged scene: a camera
sequence of --images images sharing one SIMPLE_RADIAL camera, about --points points each seen by 2..10 consecutive images
(6 on average), observations with 0.5 px noise, started from perturbed poses, points and focal length.  The gauge is the
reference's: image 0 constant pose, tvec[0] of image 1 constant.

    python tools/bench_bundle_adjustment.py [--images 10000] [--points 1000000] [--reps 3] [--cpu-points 3000] [--out profiles/r10_bundle_adjustment.json]

Records the median call (HIP events inside the call) split into set-up, Jacobian, CG and candidate phases, the LM and CG
iteration counts, and the modelled bytes one implicit S p reads per observation over the CG phase's time per S p (the CG
phase includes the per-radius preparation and the no-op launches past the CG stop, so this is a lower bound of the achieved
rate).  Separately: the numpy restatement (tests/bundle_adjustment_ref.py) on the prefix of --cpu-points points, with the
device's result on that prefix."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402
from dagsfm_amd.synthetic import world_to_image  # noqa: E402
from tests import bundle_adjustment_ref as ref  # noqa: E402


def sequence_scene(n_images, n_points, seed=2026, noise=0.5):
    rng = np.random.default_rng(seed)
    step = 0.5
    # camera i at (i * step, small jitter, 0), looking down +z with a small yaw
    yaw = rng.normal(scale=0.02, size=n_images)
    R = np.zeros((n_images, 3, 3))
    R[:, 0, 0] = np.cos(yaw)
    R[:, 0, 2] = -np.sin(yaw)
    R[:, 1, 1] = 1.0
    R[:, 2, 0] = np.sin(yaw)
    R[:, 2, 2] = np.cos(yaw)
    pos = np.stack([np.arange(n_images) * step, rng.normal(scale=0.05, size=n_images), np.zeros(n_images)], 1)
    t = -np.einsum("nij,nj->ni", R, pos)
    q = np.array([ref.rot_to_quat(r) for r in R]) if n_images <= 2000 else _rot_to_quat_batch(R)
    L = rng.integers(2, 11, n_points)
    first = np.minimum(rng.integers(0, n_images, n_points), n_images - L)
    order = np.argsort(first, kind="stable")  # points in sequence order: a prefix covers the first images
    first, L = first[order], L[order]
    X = np.stack([(first + L / 2.0) * step + rng.uniform(-1.0, 1.0, n_points), rng.uniform(-3.0, 3.0, n_points),
                  rng.uniform(8.0, 15.0, n_points)], 1)
    toff = np.concatenate([[0], np.cumsum(L)]).astype(np.uint32)
    pt = np.repeat(np.arange(n_points), L)
    img = (np.repeat(first, L) + (np.arange(len(pt)) - np.repeat(toff[:-1], L))).astype(np.uint32)
    params = np.array([800.0, 500.0, 375.0, 0.01])
    pc = np.einsum("nij,nj->ni", R[img], X[pt]) + t[img]
    x, y = world_to_image(2, params, pc[:, 0] / pc[:, 2], pc[:, 1] / pc[:, 2])
    oxy = np.stack([x, y], 1) + rng.normal(scale=noise, size=(len(pt), 2))
    qp = ref.quat_plus(q, rng.normal(scale=0.001, size=(n_images, 3)))
    # the centres stay put up to noise: t = -R' c (a rotation about the world origin would move cameras 4 km out by metres)
    tp = -np.einsum("nij,nj->ni", ref.quat_matrix(qp), pos + rng.normal(scale=0.01, size=pos.shape))
    qp[0], tp[0] = q[0], t[0]
    tp[1, 0] = t[1, 0]
    Xp = X + rng.normal(scale=0.01, size=X.shape)
    pp = params.copy()
    pp[0] *= 1.005
    cpose = np.zeros(n_images, np.uint8)
    cpose[0] = 1
    cmask = np.zeros(n_images, np.uint8)
    cmask[1] = 1
    return {"camera_model_ids": np.array([2], np.int32), "camera_params": pp, "image_camera": np.zeros(n_images, np.uint32),
            "qvec": qp, "tvec": tp, "image_constant_pose": cpose, "image_constant_tvec": cmask,
            "point_ids": np.arange(n_points, dtype=np.uint64), "xyz": Xp, "point_constant": np.zeros(n_points, np.uint8),
            "track_offsets": toff, "obs_image": img, "obs_xy": oxy}


def _rot_to_quat_batch(R):
    w = np.sqrt(np.maximum(1e-12, 1.0 + R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2])) / 2.0
    return np.stack([w, (R[:, 2, 1] - R[:, 1, 2]) / (4 * w), (R[:, 0, 2] - R[:, 2, 0]) / (4 * w), (R[:, 1, 0] - R[:, 0, 1]) / (4 * w)], 1)


def prefix(scene, n_points):
    toff = scene["track_offsets"]
    n = int(toff[n_points])
    used = np.unique(scene["obs_image"][:n])
    remap = np.full(len(scene["qvec"]), -1, np.int64)
    remap[used] = np.arange(len(used))
    out = dict(scene)
    out.update(image_camera=scene["image_camera"][used], qvec=scene["qvec"][used], tvec=scene["tvec"][used],
               image_constant_pose=scene["image_constant_pose"][used], image_constant_tvec=scene["image_constant_tvec"][used],
               point_ids=scene["point_ids"][:n_points], xyz=scene["xyz"][:n_points], point_constant=scene["point_constant"][:n_points],
               track_offsets=toff[:n_points + 1], obs_image=remap[scene["obs_image"][:n]].astype(np.uint32), obs_xy=scene["obs_xy"][:n])
    out["image_constant_pose"] = out["image_constant_pose"].copy()
    out["image_constant_pose"][0] = 1  # the prefix's own gauge
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-points", type=int, default=3000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    t0 = time.perf_counter()
    scene = sequence_scene(a.images, a.points)
    gen_s = time.perf_counter() - t0
    n_obs = len(scene["obs_image"])
    ctx = capi.Context(0)
    opt = capi.default_bundle_adjustment_options()
    runs = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        out = ctx.bundle_adjust(scene, opt)
        runs.append((out["report"].as_dict(), time.perf_counter() - t0, out))
    reps = sorted(runs, key=lambda r: r[0]["total_ms"])
    rep, wall, out = reps[len(reps) // 2]
    k = 2  # free camera parameters (f, k)
    bytes_per_obs = 376 + 32 * k  # one S p: F p per observation, E^T y per track, F^T (y - E z) per image
    cg_it = rep["total_cg_iterations"]
    n_sp = cg_it + cg_it // 10
    res = {"metric": "global bundle adjustment, device ms per call (measured)", "images": a.images, "points": a.points,
           "observations": n_obs, "camera": "SIMPLE_RADIAL, shared", "scene_generation_s": gen_s,
           "total_ms": rep["total_ms"], "setup_ms": rep["setup_ms"], "jacobian_ms": rep["jacobian_ms"], "cg_ms": rep["cg_ms"],
           "candidate_ms": rep["candidate_ms"], "call_wall_s": wall, "total_ms_all_reps": [r[0]["total_ms"] for r in runs],
           "lm_iterations": rep["num_iterations"], "successful_steps": rep["num_successful_steps"], "cg_iterations": cg_it,
           "cg_phase_ms_per_cg_iteration": rep["cg_ms"] / cg_it if cg_it else None,
           "modelled_bytes_per_observation_per_Sp": bytes_per_obs,
           "achieved_bytes_per_s_lower_bound": (bytes_per_obs * n_obs * n_sp) / (rep["cg_ms"] * 1e-3) if cg_it else None,
           "report": rep,
           "byte_identical_repeats": len({r[2]["xyz"].tobytes() + r[2]["qvec"].tobytes() for r in runs}) == 1}
    if a.cpu_points > 0:
        sub = prefix(scene, a.cpu_points)
        t0 = time.perf_counter()
        exp = ref.bundle_adjust(sub, {})
        cdt = time.perf_counter() - t0
        dev = ctx.bundle_adjust(sub, opt)
        res["cpu_restatement"] = {"method": "tests/bundle_adjustment_ref.py: numpy + scipy.sparse, dense Schur complement",
                                  "points": a.cpu_points, "images": len(sub["qvec"]), "observations": len(sub["obs_image"]),
                                  "seconds": cdt, "device_ms_same_prefix": dev["report"].total_ms,
                                  "same_iterations": dev["report"].num_iterations == exp["report"]["num_iterations"],
                                  "final_cost_device": dev["report"].final_cost, "final_cost_restatement": exp["report"]["final_cost"],
                                  "min_margins": [exp["report"]["min_rho_margin"], exp["report"]["min_cg_margin"],
                                                  exp["report"]["min_gradient_margin"]]}
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
