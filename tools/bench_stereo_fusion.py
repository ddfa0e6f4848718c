#!/usr/bin/env python3
"""First measurements of dsm_fuse_stereo: the slanted and the step scene of tests/patch_match_scenes.py, by
default 1600 x 1200 with 10 images, truth maps with 0.2 % depth noise, every image listing all others, at the reference's
default options.  Per scene: one warm-up call, then the median of --repeats calls (host clock around dsm_fuse_stereo, which
returns with the points on the host) with the stage times, the rounds per image, the traversals per pixel and the points per
second; against libdsm_stereo_fusion_host.so, the same header on ONE CPU thread of the same box (the reference is
single-threaded, and no earlier commit has this stage), whose points must equal the device's on the bits; and, with
--serial-size, the check build's serial lane (DSM_FUSION_SERIAL) at that smaller size against both.  Before timing, a
37 x 23 case is held to tests/stereo_fusion_ref.py bit for bit, so that what is timed is what is specified.

    python tools/bench_stereo_fusion.py [--size 1600x1200] [--images 10] [--repeats 3] [--scenes slanted,step]
                                        [--serial-size 200x150] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagsfm_amd import capi  # noqa: E402
from tests import stereo_fusion_cases as cases  # noqa: E402


def device_call(ctx, args, n_images):
    arr, offs, idx, _ = args
    n = ctypes.c_uint64(0)
    o = capi.default_stereo_fusion_options()
    t0 = time.perf_counter()
    rc = ctx._L.dsm_fuse_stereo(ctx._h, ctypes.byref(o), n_images, ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, ctypes.byref(n))
    wall = time.perf_counter() - t0
    if rc != 0:
        ctx._fail("dsm_fuse_stereo", rc)
    return wall, int(n.value)


def device_points(ctx, n):
    rec = np.zeros(max(n, 1), dtype=capi.FUSED_POINT_DTYPE)
    voff = np.zeros(n + 1, dtype=np.uint64)
    ctx._chk(ctx._L.dsm_get_fused_points(ctx._h, rec.ctypes.data, len(rec), voff.ctypes.data, None, 0))
    vimg = np.zeros(max(int(voff[-1]), 1), dtype=np.uint32)
    ctx._chk(ctx._L.dsm_get_fused_points(ctx._h, None, 0, None, vimg.ctypes.data, len(vimg)))
    return rec[:n], voff, vimg[:int(voff[-1])]


def host_call(args, n_images):
    L = capi.fusion_host_lib()
    arr, offs, idx, _ = args
    n, trav = ctypes.c_uint64(0), ctypes.c_uint64(0)
    t0 = time.perf_counter()
    rc = L.dsm_fusion_host_run(None, n_images, ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, ctypes.byref(n), ctypes.byref(trav), None)
    wall = time.perf_counter() - t0
    assert rc == 0, rc
    n = int(n.value)
    rec = np.zeros(max(n, 1), dtype=capi.FUSED_POINT_DTYPE)
    bits = np.zeros((max(n, 1), (n_images + 31) // 32), dtype=np.uint32)
    L.dsm_fusion_host_get(rec.ctypes.data, bits.ctypes.data, None)
    return wall, rec[:n], bits[:n], int(trav.value)


def same_points(rec, voff, vimg, host_rec, host_bits, n_images):
    if len(rec) != len(host_rec) or rec.tobytes() != host_rec.tobytes():
        return False
    bits = np.zeros_like(host_bits)
    owner = np.repeat(np.arange(len(rec)), np.diff(voff).astype(np.int64))
    np.bitwise_or.at(bits, (owner, vimg // 32), (np.uint32(1) << (vimg % 32).astype(np.uint32)))
    return bool((bits == host_bits).all())


def measure(ctx, kind, w, h, n_images, repeats, with_host=True):
    images = cases.make_images(kind, [(w, h)] * n_images, noise=0.002, seed=4)
    overlap = cases.all_others(n_images)
    args = capi._fusion_call_arguments(images, overlap)
    device_call(ctx, args, n_images)  # warm-up: code objects, buffers
    walls = []
    for _ in range(repeats):
        wall, n = device_call(ctx, args, n_images)
        walls.append(wall)
    ms = ctx.stereo_fusion_time()
    pos, rounds = ctx.stereo_fusion_rounds(n_images)
    wall = statistics.median(walls)
    pixels = float(w) * h * n_images
    row = {"scene": kind, "size": [w, h], "images": n_images, "points": n, "call_s_median": wall, "call_s": walls, "stage_ms_last_call": ms,
           "rounds_per_image_in_fusion_order": [int(rounds[i]) for i in np.argsort(pos)], "traversals_per_pixel": ms["traversals"] / pixels,
           "points_per_s": n / wall, "pixels_per_s": pixels / wall}
    if with_host:
        host_wall, host_rec, host_bits, host_trav = host_call(args, n_images)
        rec, voff, vimg = device_points(ctx, n)
        row.update({"host_one_thread_s": host_wall, "host_traversals_per_pixel": host_trav / pixels, "speedup_over_host_one_thread": host_wall / wall,
                    "equal_to_host_build": same_points(rec, voff, vimg, host_rec, host_bits, n_images)})
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", default="1600x1200")
    ap.add_argument("--images", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--scenes", default="slanted,step")
    ap.add_argument("--serial-size", default=None, help="WxH at which the check build's serial lane is timed as well")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    ctx = capi.Context(0, check=False)
    images, overlap, options = cases.case("slanted")
    assert cases.same_result(ctx.stereo_fusion(images, overlap, **options), cases.expected("slanted")), "bench parity"
    result = {"options": "defaults", "depth_noise": 0.002, "rows": [], "serial": []}
    for kind in a.scenes.split(","):
        row = measure(ctx, kind, w, h, a.images, a.repeats)
        result["rows"].append(row)
        print(json.dumps(row), flush=True)
    if a.serial_size:
        sw, sh = (int(v) for v in a.serial_size.split("x"))
        check = capi.Context(0, check=True)
        for kind in a.scenes.split(","):
            row = measure(ctx, kind, sw, sh, a.images, a.repeats)
            check.set_debug_option("DSM_FUSION_SERIAL", "1")
            args = capi._fusion_call_arguments(cases.make_images(kind, [(sw, sh)] * a.images, noise=0.002, seed=4), cases.all_others(a.images))
            arr, offs, idx, _ = args
            n = ctypes.c_uint64(0)
            t0 = time.perf_counter()
            rc = check._L.dsm_fuse_stereo(check._handle, None, a.images, ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, ctypes.byref(n))
            row["serial_lane_s"] = time.perf_counter() - t0
            assert rc == 0 and int(n.value) == row["points"], (rc, int(n.value), row["points"])
            row["speedup_over_serial_lane"] = row["serial_lane_s"] / row["call_s_median"]
            result["serial"].append(row)
            print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
