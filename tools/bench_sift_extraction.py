#!/usr/bin/env python3
"""Times dsm_extract_sift on texture of tests/sift_scenes.py at 640 x 480, 1600 x 1200 and 3200 x 2400 (the
reference's max_image_size) with the default options.

Before anything is timed, one small size is extracted on the device and by the numpy restatement (tests/sift_ref.py) and the two
must agree bit for bit.  Per size: the wall time per image (host pointers in, features out, the median of --repeat calls after a
warm-up), the HIP-event time of every stage (dsm_get_sift_time), and for the smoothing of the levels the achieved bytes/s --
every pass counted as one read and one write of the level, 2 passes per level, S + 2 levels per octave -- against the HBM figure
the runtime reports (2 x memory clock x bus width).  Reads nothing from the reference.  If profiles/sift_vlfeat_host_times.json
exists (written by `tools/make_sift_golden.py --time W H --json`, the SSE2 build of VLFeat on one core of the host THAT tool ran
on), its times are copied in for comparison, labelled as another host's.

  python tools/bench_sift_extraction.py [--sizes 640x480,1600x1200,3200x2400] [--repeat 5] [--out profiles/r16_sift_extraction.json]
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
from tests import sift_ref, sift_scenes  # noqa: E402


def smoothing_bytes(width, height, options):
    total = 0
    for oc in range(options.first_octave, options.first_octave + options.num_octaves):
        w = width >> oc if oc >= 0 else width << -oc
        h = height >> oc if oc >= 0 else height << -oc
        if w < 2 or h < 2:
            break
        total += (options.octave_resolution + 2) * 2 * (2 * 4 * w * h)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1600x1200,3200x2400")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--check-size", default="160x120")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_sift_extraction.json"))
    args = ap.parse_args()
    ctx = capi.Context(0)
    o = capi.default_sift_options()
    cw, ch = map(int, args.check_size.split("x"))
    image = sift_scenes.texture(cw, ch, 1)
    kp, ds = ctx.extract_sift(image, o)
    rkp, rds = sift_ref.extract(image)
    assert kp.shape == rkp.shape and (kp.view(np.uint32) == rkp.view(np.uint32)).all() and (ds == rds).all(), "device and restatement differ"
    info = ctx.device_info()
    peak = 2.0 * info.memory_clock_khz * 1e3 * info.memory_bus_bits / 8 if info.memory_clock_khz > 0 and info.memory_bus_bits > 0 else None
    out = {"tool": "tools/bench_sift_extraction.py", "options": "defaults (4 octaves from -1, 3 levels, 2 orientations, L1_ROOT)",
           "device": {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units,
                      "hbm_peak_bytes_per_s": peak},
           "check": {"size": args.check_size, "features": int(len(kp)), "bit_exact_vs_restatement": True}, "sizes": []}
    for size in args.sizes.split(","):
        w, h = map(int, size.split("x"))
        image = sift_scenes.texture(w, h, 1)
        ctx.extract_sift(image, o)  # warm-up: allocations
        walls, stages = [], []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            kp, ds = ctx.extract_sift(image, o)
            walls.append((time.perf_counter() - t0) * 1e3)
            stages.append(ctx.sift_time())
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        nbytes = smoothing_bytes(w, h, o)
        bw = nbytes / (med["smoothing"] * 1e-3) if med["smoothing"] > 0 else None
        row = {"size": size, "features": int(len(kp)), "wall_ms_per_image": float(np.median(walls)), "wall_ms_all": walls,
               "stage_ms": med, "device_ms": float(sum(med.values())), "smoothing_bytes": nbytes, "smoothing_bytes_per_s": bw,
               "smoothing_fraction_of_hbm_peak": (bw / peak if bw and peak else None)}
        out["sizes"].append(row)
        print(json.dumps(row))
    host = os.path.join(ROOT, "profiles", "sift_vlfeat_host_times.json")
    if os.path.exists(host):
        out["vlfeat_on_one_core_of_ANOTHER_host"] = json.load(open(host))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
