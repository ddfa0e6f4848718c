#!/usr/bin/env python3
"""The point and observation filters (dsm_filter_points3D) on one MI355X, on two scenes:

  sequence   the 10 000-image sequence of tools/bench_retriangulation.py after its re-triangulation: the existing tracks, the
             continued observations and the new points as one reconstruction
  ba         the scene of profiles/r10_bundle_adjustment.json (tools/bench_bundle_adjustment.sequence_scene)

    python tools/bench_point_filter.py [--images 10000] [--points 1000000] [--reps 5] [--cpu-points 3000] [--skip-sequence]
                                       [--out profiles/r14_point_filter.json]

Per scene and per pass mask (2 | 4 = FilterAllPoints3D, 1 = the prelude of AdjustGlobalBundle, 8 = the RMSE lines): the median
of --reps calls after one warm-up, by the call's device time (HIP events inside the call) with its split, the call's wall
time, what each pass removed, the lane- and wave-path counts and the pairs evaluated.  Beside it: the numpy restatement's
time on the first --cpu-points points of the `ba` scene with the device on the same sub-scene, and the ratio of the filter's
device time to dsm_bundle_adjust's on the same scene, read from the committed profiles/r10_bundle_adjustment.json.  No
pass / fail time: the stage has no predecessor to compare with."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from dagsfm_amd import capi  # noqa: E402
from tests import point_filter_ref as ref  # noqa: E402
from tests import retriangulation_ref as rt  # noqa: E402
import bench_bundle_adjustment as bba  # noqa: E402
import bench_retriangulation as brt  # noqa: E402

PASSES = (("filter_all_points3D", 2 | 4), ("negative_depth", 1), ("mean_reprojection_error", 8))


def after_retriangulation(ctx, images, clusters=100, overlap=50, points_per_image=120):
    """bench_retriangulation's scene and call, then the merged reconstruction as the dict of bundle_adjust (tracks of two
    observations or more, as the solve takes them)."""
    scene, _ = rt.make_scene(n_images=images, n_points=images * points_per_image // 4, track=(2, 6), noise=0.3, wrong=0.1,
                             existing=0.3, sequence=True, seed=2026)
    seps = [int(scene["image_ids"][i]) for i in brt.separators(images, clusters, overlap)]
    out = ctx.retriangulate(scene, seps)
    off = np.asarray(scene["points2D_offsets"], np.int64)
    img_of = np.repeat(np.arange(images), np.diff(off))
    index_of_image = {int(v): i for i, v in enumerate(scene["image_ids"])}
    row_of_point = {int(v): i for i, v in enumerate(scene["point3D_ids"])}
    p3 = np.asarray(scene["points2D_point3D"], np.int64)
    have = np.nonzero(p3 >= 0)[0]
    pt = [p3[have]]
    ob = [have]
    P0 = len(scene["point3D_ids"])
    row_of_point.update({int(v): P0 + k for k, v in enumerate(out["new_point_ids"])})  # Continue may extend a point of this call
    cont = np.asarray(out["continued_obs"], np.int64).reshape(-1, 2)
    if len(cont):
        pt.append(np.array([row_of_point[int(v)] for v in out["continued_point_ids"]], np.int64))
        ob.append(off[[index_of_image[int(v)] for v in cont[:, 0]]] + cont[:, 1])
    new = np.asarray(out["new_track_obs"], np.int64).reshape(-1, 2)
    noff = np.asarray(out["new_track_offsets"], np.int64)
    if len(new):
        pt.append(P0 + np.repeat(np.arange(len(noff) - 1), np.diff(noff)))
        ob.append(off[[index_of_image[int(v)] for v in new[:, 0]]] + new[:, 1])
    pt, ob = np.concatenate(pt), np.concatenate(ob)
    order = np.argsort(pt, kind="stable")
    pt, ob = pt[order], ob[order]
    xyz = np.vstack([np.asarray(scene["point3D_xyz"], float).reshape(-1, 3), np.asarray(out["new_xyz"], float).reshape(-1, 3)])
    counts = np.bincount(pt, minlength=len(xyz))
    keep = counts[pt] >= 2
    pt, ob = pt[keep], ob[keep]
    used = np.nonzero(counts >= 2)[0]
    cam = scene["cameras"][0]
    return {"camera_model_ids": [cam.model_id], "camera_params": list(cam.params)[:capi.CAMERA_MODEL_NUM_PARAMS[cam.model_id]],
            "camera_width": [cam.width], "camera_height": [cam.height], "image_camera": np.zeros(images, np.uint32),
            "qvec": np.asarray(scene["qvec"], float), "tvec": np.asarray(scene["tvec"], float), "xyz": xyz[used],
            "point_ids": used.astype(np.uint64), "track_offsets": np.concatenate([[0], np.cumsum(counts[used])]).astype(np.uint32),
            "obs_image": img_of[ob].astype(np.uint32), "obs_xy": np.asarray(scene["points2D_xy"], float).reshape(-1, 2)[ob]}


def measure(ctx, scene, reps):
    out = {}
    for name, passes in PASSES:
        ctx.filter_points3D(scene, passes=passes)  # warm-up
        runs = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = ctx.filter_points3D(scene, passes=passes)
            runs.append((r["report"].as_dict(), time.perf_counter() - t0, r))
        order = sorted(range(reps), key=lambda k: runs[k][0]["device_ms"])
        rep, wall, _ = runs[order[reps // 2]]
        keys = ("point_keep", "obs_keep", "point_error", "kept_obs")
        out[name] = {"passes": passes, "device_ms": rep["device_ms"], "call_wall_s": wall,
                     "split_ms": {k: rep[k] for k in ("setup_ms", "upload_ms", "residuals_ms", "tracks_ms", "angles_ms", "compaction_ms",
                                                      "download_ms")},
                     "device_ms_all_reps": [r[0]["device_ms"] for r in runs], "num_filtered": rep["num_filtered"],
                     "points_deleted": rep["points_deleted"], "observations_deleted": rep["observations_deleted"],
                     "lane_path_tracks": rep["lane_path_tracks"], "wave_path_tracks": rep["wave_path_tracks"],
                     "pairs_evaluated": rep["pairs_evaluated"], "mean_reprojection_error": rep["mean_reprojection_error"],
                     "mean_point_error": rep["mean_point_error"],
                     "byte_identical_repeats": all(all(r[2][k].tobytes() == runs[0][2][k].tobytes() for k in keys) for r in runs)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu-points", type=int, default=3000)
    ap.add_argument("--skip-sequence", action="store_true")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"metric": "point and observation filters, device ms per call (measured: median of %d after one warm-up)" % a.reps,
           "scenes": {}}
    scene = bba.sequence_scene(a.images, a.points)
    entry = {"images": a.images, "points": len(scene["xyz"]), "observations": len(scene["obs_image"]), "runs": measure(ctx, scene, a.reps)}
    r10 = os.path.join(ROOT, "profiles", "r10_bundle_adjustment.json")
    if os.path.exists(r10):
        ba = json.load(open(r10))
        if ba.get("images") == a.images and ba.get("points") == a.points:
            entry["bundle_adjust_total_ms_from_r10_record"] = ba["total_ms"]
            entry["filter_device_ms_over_bundle_adjust_ms"] = {k: v["device_ms"] / ba["total_ms"] for k, v in entry["runs"].items()}
    if a.cpu_points > 0:
        sub = bba.prefix(scene, min(a.cpu_points, len(scene["xyz"])))
        t0 = time.perf_counter()
        exp = ref.filter_points3D(sub, passes=15)
        cdt = time.perf_counter() - t0
        dev = ctx.filter_points3D(sub, passes=15)
        entry["cpu_restatement"] = {"method": "tests/point_filter_ref.py: sequential numpy, passes 1 | 2 | 4 | 8", "points": len(sub["xyz"]),
                                    "observations": len(sub["obs_image"]), "seconds": cdt,
                                    "device_ms_same_sub_scene": dev["report"].device_ms,
                                    "same_point_keep": bool((dev["point_keep"] == exp["point_keep"]).all()),
                                    "unclear_points": int((~ref.clear_points(exp)).sum())}
    res["scenes"]["ba"] = entry
    if not a.skip_sequence:
        t0 = time.perf_counter()
        seq = after_retriangulation(ctx, a.images)
        res["scenes"]["sequence"] = {"images": a.images, "points": len(seq["xyz"]), "observations": len(seq["obs_image"]),
                                     "scene_generation_and_retriangulation_s": time.perf_counter() - t0, "runs": measure(ctx, seq, a.reps)}
    res["not_measured"] = "the lane / wave cut (PF_LANE_CUT = 16) was chosen by reasoning, not by a sweep; no counters were collected"
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
