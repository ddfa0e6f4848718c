#!/usr/bin/env python3
"""Times dsm_extract_covariant_sift on texture of tests/sift_scenes.py at 640 x 480, 1600 x 1200 and 3200 x 2400
with the default options (domain-size pooling on, 10 scales).

Before anything is timed, one golden case (tests/golden/covdet_vlfeat_v1.npz, VLFeat's own output) is extracted on the device
and must agree bit for bit: keypoint rows, (o, s), scores, raw descriptors and bytes.  Per size: the wall time per image (host
pointers in, features out, the median of --repeat calls after a warm-up), the HIP-event time of every stage
(dsm_get_covariant_sift_time) and the descriptor stage's time per (feature, pooling scale); next to it dsm_extract_sift's time
per descriptor from profiles/r16_sift_extraction.json where that file exists.  Reads nothing from the reference.  If
profiles/covdet_vlfeat_host_times.json exists (written by `tools/make_covdet_golden.py --time W H --json`: the SSE2 build of
VLFeat on one core of the host THAT tool ran on), its times are copied in for comparison, labelled as another host's.

  python tools/bench_covariant_sift.py [--sizes 640x480,1600x1200,3200x2400] [--repeat 5] [--out profiles/r21_covariant_sift.json]

--affine times dsm_extract_covariant_sift_affine with estimate_affine_shape = 1 on the same sizes instead: the
check case comes from tests/golden/covdet_vlfeat_affine_v1.npz, the median is over 3 calls unless --repeat is given, every row
also holds the rounds of the shape adaptation, the features active in each round (dsm_get_affine_shape_stats) and the host's
share of a call (wall time minus the summed HIP-event times), and the output is profiles/r27_affine_shape.json.  The other
host's times are those of `tools/make_covdet_affine_golden.py --time W H --json` (profiles/covdet_vlfeat_affine_host_times.json).
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
from tests import covariant_sift_ref as ref  # noqa: E402
from tests import sift_scenes  # noqa: E402


def check(ctx, name, affine=False):
    if affine:
        from tests import affine_sift_ref
        case = affine_sift_ref.golden()[name]
        want = affine_sift_ref.expected(case, name)
    else:
        case = ref.golden()[name]
        want = ref.expected(case, name)
    o = capi.default_covariant_sift_options(**case["options"])
    kp, desc = (ctx.extract_covariant_sift_affine if affine else ctx.extract_covariant_sift)(case["image"], o)
    raw = ctx.covariant_sift_raw(num_scales=int(case["counts"][5]))
    same = lambda a, b: a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)).all()
    assert same(kp, want["keypoints"]) and same(raw["octave_scale"], want["os"]) and same(raw["scores"], want["scores"]), "features differ from VLFeat's"
    assert same(ref.digest(raw["raw"]), want["digests"]), "raw descriptors differ from VLFeat's"
    assert same(desc, ref.describe(raw["raw"], case["options"]["domain_size_pooling"], ref.L1_ROOT)), "descriptor bytes differ"
    return len(kp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1600x1200,3200x2400")
    ap.add_argument("--repeat", type=int, default=None, help="timed calls per size (default 5, 3 with --affine)")
    ap.add_argument("--affine", action="store_true", help="estimate_affine_shape = 1 through dsm_extract_covariant_sift_affine")
    ap.add_argument("--check-case", default="tex200x150")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    repeat = args.repeat if args.repeat else (3 if args.affine else 5)
    out_path = args.out or os.path.join(ROOT, "profiles", "r27_affine_shape.json" if args.affine else "r21_covariant_sift.json")
    ctx = capi.Context(0)
    o = capi.default_covariant_sift_options(estimate_affine_shape=1 if args.affine else 0)
    extract = ctx.extract_covariant_sift_affine if args.affine else ctx.extract_covariant_sift
    n = check(ctx, args.check_case, args.affine)
    info = ctx.device_info()
    out = {"tool": "tools/bench_covariant_sift.py" + (" --affine" if args.affine else ""),
           "options": ("estimate_affine_shape = 1, otherwise " if args.affine else "") + "defaults (octaves from -1, 3 levels, domain-size pooling over 10 scales, L1_ROOT, at most 8192 features)",
           "device": {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units},
           "check": {"case": args.check_case, "features": int(n), "bit_exact_vs_vlfeat_golden": True}, "sizes": []}
    for size in args.sizes.split(","):
        w, h = map(int, size.split("x"))
        image = sift_scenes.texture(w, h, 1)
        extract(image, o)  # warm-up: allocations
        walls, stages = [], []
        for _ in range(repeat):
            t0 = time.perf_counter()
            kp, ds = extract(image, o)
            walls.append((time.perf_counter() - t0) * 1e3)
            stages.append(ctx.covariant_sift_time())
        med = {k: float(np.median([s[k] for s in stages])) for k in stages[0]}
        items = len(kp) * o.dsp_num_scales
        row = {"size": size, "features": int(len(kp)), "items": int(items), "wall_ms_per_image": float(np.median(walls)), "wall_ms_all": walls,
               "stage_ms": med, "device_ms": float(sum(med.values())),
               "descriptor_us_per_feature_scale": (med["descriptors"] * 1e3 / items if items else None)}
        if args.affine:
            st = ctx.affine_shape_stats()
            row["affine_shape"] = {"rounds": st["rounds"], "active": st["active"], "exits": st["exits"], "launched_patches": int(sum(st["active"])),
                                   "moment_us_per_patch": med["orientations"] * 1e3 / max(1, sum(st["active"]))}
            row["host_ms_per_image"] = row["wall_ms_per_image"] - row["device_ms"]  # every stage's host half, the copies and the syncs
        out["sizes"].append(row)
        print(json.dumps(row))
    r16 = os.path.join(ROOT, "profiles", "r16_sift_extraction.json")
    if os.path.exists(r16):
        out["dsm_extract_sift_descriptor_us_per_descriptor"] = {
            s["size"]: s["stage_ms"]["descriptors"] * 1e3 / s["features"] for s in json.load(open(r16))["sizes"] if s["features"]}
    host = os.path.join(ROOT, "profiles", "covdet_vlfeat_affine_host_times.json" if args.affine else "covdet_vlfeat_host_times.json")
    if os.path.exists(host):
        out["vlfeat_on_one_core_of_ANOTHER_host"] = json.load(open(host))
    with open(out_path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
