#!/usr/bin/env python3
"""Times dsm_warp_images on a batch of 4000 x 3000 RGB images: one algebraic source model (OPENCV) and one
fisheye one (OPENCV_FISHEYE), each warped into its own undistorted camera, as image_undistorter does.

Before anything is timed, a 130 x 33 case of each model must agree with tests/undistortion_ref.py byte for byte (images) and
double for double (the map of source points).  Per model: the HIP-event time of the warp kernel per image
(dsm_get_undistortion_time, the median of --repeat calls after a warm-up), the bytes the kernel has to move (every source byte
read once, every target byte written once) over that time against the 6.29 TB/s a float4 copy reaches on the MI355X, the
upload and download times of the same call, and dsm_undistort_cameras' border scan.  For comparison the same images through the
numpy restatement: its rate is measured on a 96 x 72 camera of the same model and EXTRAPOLATED to 4000 x 3000 by the pixel
count, labelled as such (the restatement calls the oracle once per pixel; it is a checker, not an implementation anybody runs).
Reads nothing from the reference.

  python tools/bench_undistortion.py [--size 4000x3000] [--images 4] [--repeat 5] [--out profiles/r22_undistortion.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dagsfm_amd import capi  # noqa: E402
from tests import oracle_lib  # noqa: E402
from tests import undistortion_ref as ref  # noqa: E402
from tests import undistortion_scenes as scenes  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s of a float4 copy on the MI355X (measured; the HBM3E specification is 8.0e12)
MODELS = (("OPENCV", 4), ("OPENCV_FISHEYE", 5))


def check(ctx, orc, model_id):
    source = scenes.camera(model_id, 130, 33)
    target = ctx.undistort_cameras([source])[0]
    assert bytes(target) == bytes(ref.undistort_camera(orc, source)), "the undistorted camera differs from the restatement's"
    images = scenes.stack(130, 33, 2, 3)
    got = ctx.warp_images(source, target, images, return_map=True)
    want = ref.warp_images(orc, source, target, images)
    g, w = got["source_xy"], want["source_xy"]
    assert ((g.view(np.uint64) == w.view(np.uint64)) | (np.isnan(g) & np.isnan(w))).all(), "the map differs from the restatement's"
    assert (got["images"] == want["images"]).all(), "the bytes differ from the restatement's"


def big_images(width, height, n):
    """n RGB images of one 512 x 512 texture tiled over the frame, shifted per image and channel (integer arithmetic only)."""
    t = scenes.grey(512, 512, 3)
    tile = np.tile(t, ((height + 511) // 512 + 1, (width + 511) // 512 + 1))
    out = np.empty((n, height, width, 3), np.uint8)
    for i in range(n):
        for c in range(3):
            dy, dx = 37 * i + 11 * c, 53 * i + 7 * c
            out[i, :, :, c] = tile[dy:dy + height, dx:dx + width]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="4000x3000")
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_undistortion.json"))
    args = ap.parse_args()
    width, height = map(int, args.size.split("x"))
    orc = oracle_lib.load()
    ctx = capi.Context(0)
    info = ctx.device_info()
    images = big_images(width, height, args.images)
    out = {"tool": "tools/bench_undistortion.py", "size": args.size, "images_per_batch": args.images, "channels": 3,
           "device": {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units},
           "copy_rate_bytes_per_s": COPY_RATE, "models": []}
    for name, model_id in MODELS:
        check(ctx, orc, model_id)
        source = scenes.camera(model_id, width, height)
        target = ctx.undistort_cameras([source])[0]
        scan_ms = ctx.undistortion_time()["border_scan"]
        dst = np.zeros_like(images)
        ctx.warp_images(source, target, images, out=dst)  # warm-up: allocations, code object
        kernel, upload, download, wall = [], [], [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            r = ctx.warp_images(source, target, images, out=dst)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = ctx.undistortion_time()
            kernel.append(t["warp_kernel"])
            upload.append(t["warp_upload"])
            download.append(t["warp_download"])
        k_ms = float(np.median(kernel)) / args.images
        moved = 2.0 * width * height * 3  # bytes per image: the source read once, the target written once
        # the restatement on a small camera of the same model, extrapolated by the pixel count
        sw, sh = 96, 72
        s_source = scenes.camera(model_id, sw, sh)
        s_target = ctx.undistort_cameras([s_source])[0]
        s_images = scenes.stack(sw, sh, 1, 3)
        t0 = time.perf_counter()
        ref.warp_images(orc, s_source, s_target, s_images)
        ref_s = time.perf_counter() - t0
        row = {"model": name, "undistorted_size": "%dx%d" % (target.width, target.height), "rescale_owed": bool(r["needs_rescale"]),
               "nonzero_fraction": float((dst != 0).mean()), "border_scan_ms": scan_ms,
               "warp_kernel_ms_per_image": k_ms, "warp_kernel_ms_all_batches": kernel,
               "upload_ms_per_image": float(np.median(upload)) / args.images, "download_ms_per_image": float(np.median(download)) / args.images,
               "wall_ms_per_image_host_pointers": float(np.median(wall)) / args.images,
               "bytes_moved_per_image": moved, "achieved_bytes_per_s": moved / (k_ms * 1e-3),
               "fraction_of_copy_rate": moved / (k_ms * 1e-3) / COPY_RATE,
               "numpy_restatement": {"measured_on": "%dx%d" % (sw, sh), "seconds": ref_s,
                                     "EXTRAPOLATED_seconds_per_image_at_full_size": ref_s * (width * height) / (sw * sh),
                                     "note": "extrapolated by the pixel count from the small camera; one oracle call per pixel"}}
        out["models"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
