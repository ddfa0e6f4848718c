#!/usr/bin/env python3
"""Regenerates tests/golden/sift_vlfeat_v1.npz and sift_vlfeat_v2.npz: the cases of tests/sift_scenes.py (cases() and
cases_v2()) run through the reference's VLFeat.

Needs the reference tree (default /root/reference, or --reference DIR); nothing of it is copied into the repository.  The
driver tools/sift_golden_driver.c is compiled against lib/VLFeat/{sift,imopv,imopv_sse2,generic,host,mathop,mathop_sse2,random}.c
in a temporary directory, twice: with SSE2 as the reference's CMake builds it (-DVL_DISABLE_AVX -DVL_DISABLE_OPENMP), and with
-DVL_DISABLE_SSE2 added.  Both builds must write identical bytes for every case, or the tool fails.

The file holds, per case NAME: NAME/image (uint8), NAME/options (float64: num_octaves, octave_resolution, first_octave, upright,
peak_threshold, edge_threshold), NAME/ints (int32 [n, 4]: o, ix, iy, is), NAME/floats (float32 [n, 4]: x, y, s, sigma),
NAME/num_angles (int32 [n]), NAME/angles (float64 [n, 4]) and NAME/descriptors (float32 [sum num_angles, 128], VLFeat's order).
The archive is written with fixed time stamps, so a second run gives the same bytes.

  python tools/make_sift_golden.py            # rewrite both golden files, print the counts
  python tools/make_sift_golden.py --check    # regenerate in memory and compare with the committed files
  python tools/make_sift_golden.py --time W H [--json]  # wall time of the SSE2 build on one core for texture(W, H); --json records
                                                        # it for tools/bench_sift_extraction.py
"""
import argparse
import io
import os
import struct
import subprocess
import sys
import tempfile
import time
import zipfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import sift_scenes  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "sift_vlfeat_v1.npz")
GOLDEN_V2 = os.path.join(ROOT, "tests", "golden", "sift_vlfeat_v2.npz")
VL_SOURCES = ["sift", "imopv", "imopv_sse2", "generic", "host", "mathop", "mathop_sse2", "random"]
OPTION_KEYS = ("num_octaves", "octave_resolution", "first_octave", "upright", "peak_threshold", "edge_threshold")


def build(reference, out_dir, sse2):
    vl = os.path.join(reference, "lib", "VLFeat")
    if not os.path.isdir(vl):
        raise SystemExit("no reference tree at %s" % reference)
    exe = os.path.join(out_dir, "driver_sse2" if sse2 else "driver_plain")
    cmd = ["gcc", "-O2", "-msse2", "-DVL_DISABLE_AVX", "-DVL_DISABLE_OPENMP"] + ([] if sse2 else ["-DVL_DISABLE_SSE2"])
    cmd += ["-I", vl, "-o", exe, os.path.join(ROOT, "tools", "sift_golden_driver.c")]
    cmd += [os.path.join(vl, s + ".c") for s in VL_SOURCES] + ["-lm", "-lpthread"]
    subprocess.check_call(cmd)
    return exe


def run(exe, work, image, options):
    h, w = image.shape
    req, res = os.path.join(work, "request.bin"), os.path.join(work, "result.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<8i", w, h, options["num_octaves"], options["octave_resolution"], options["first_octave"],
                            options["upright"], 0, 0))
        f.write(struct.pack("<2d", options["peak_threshold"], options["edge_threshold"]))
        f.write(np.ascontiguousarray(image, np.uint8).tobytes())
    t0 = time.perf_counter()
    subprocess.check_call([exe, req, res])
    dt = time.perf_counter() - t0
    return open(res, "rb").read(), dt


def parse(blob):
    n = struct.unpack_from("<i", blob, 0)[0]
    at = 8
    ints, flts, nang, angles, desc = [], [], [], [], []
    for _ in range(n):
        ints.append(np.frombuffer(blob, "<i4", 4, at))
        flts.append(np.frombuffer(blob, "<f4", 4, at + 16))
        k = struct.unpack_from("<i", blob, at + 32)[0]
        nang.append(k)
        angles.append(np.frombuffer(blob, "<f8", 4, at + 40))
        at += 72
        desc.append(np.frombuffer(blob, "<f4", 128 * k, at).reshape(k, 128))
        at += 512 * k
    assert at == len(blob)
    z = lambda dt, shape: np.zeros(shape, dt)
    return {"ints": np.array(ints, np.int32) if n else z(np.int32, (0, 4)), "floats": np.array(flts, np.float32) if n else z(np.float32, (0, 4)),
            "num_angles": np.array(nang, np.int32), "angles": np.array(angles, np.float64) if n else z(np.float64, (0, 4)),
            "descriptors": np.concatenate(desc).astype(np.float32) if n and sum(nang) else z(np.float32, (0, 128))}


def generate(reference, cases):
    arrays, counts = {}, []
    with tempfile.TemporaryDirectory() as work:
        exe_sse2, exe_plain = build(reference, work, True), build(reference, work, False)
        for name, image, options in cases:
            a, _ = run(exe_sse2, work, image, options)
            b, _ = run(exe_plain, work, image, options)
            assert a == b, "the SSE2 and the plain build of VLFeat disagree on case %s" % name
            rec = parse(a)
            arrays[name + "/image"] = np.ascontiguousarray(image, np.uint8)
            arrays[name + "/options"] = np.array([options[k] for k in OPTION_KEYS], np.float64)
            for k, v in rec.items():
                arrays[name + "/" + k] = v
            octs = sorted(set(rec["ints"][:, 0].tolist()))
            levels = sorted(set(map(tuple, rec["ints"][:, [0, 3]].tolist())))
            most = int(rec["num_angles"].max()) if len(rec["ints"]) else 0
            counts.append("  %-14s %4d keypoints, %4d descriptors, octaves %s, %d DoG levels, at most %d orientations" % (
                name, len(rec["ints"]), len(rec["descriptors"]), octs, len(levels), most))
    return arrays, counts


def archive(arrays):
    """An .npz with fixed time stamps (numpy.savez stamps the current time)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0))
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, b.getvalue())
    return buf.getvalue()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--time", nargs=2, type=int, metavar=("W", "H"))
    ap.add_argument("--json", action="store_true", help="with --time: record the time in profiles/sift_vlfeat_host_times.json")
    ap.add_argument("--peaks", action="store_true", help="list the keypoint count of texture(64, 48, 2) over peak thresholds")
    args = ap.parse_args()
    if args.time:
        with tempfile.TemporaryDirectory() as work:
            exe = build(args.reference, work, True)
            image = sift_scenes.texture(args.time[0], args.time[1], 1)
            blob, dt = run(exe, work, image, sift_scenes.DEFAULTS)
            nkeys = struct.unpack_from("<i", blob, 0)[0]
            print("%d x %d: %d keypoints, %.3f s wall (process start and file I/O included)" % (args.time[0], args.time[1], nkeys, dt))
            if args.json:
                import json
                path = os.path.join(ROOT, "profiles", "sift_vlfeat_host_times.json")
                rec = json.load(open(path)) if os.path.exists(path) else {
                    "what": "wall time of tools/sift_golden_driver.c (VLFeat, SSE2 build, one core, all orientations and descriptors, "
                            "process start and file I/O included) on the host that ran tools/make_sift_golden.py -- not the GPU host"}
                rec["%dx%d" % tuple(args.time)] = {"wall_s": round(dt, 3), "keypoints": nkeys}
                with open(path, "w") as f:
                    json.dump(rec, f, indent=1, sort_keys=True)
                    f.write("\n")
        return
    if args.peaks:
        with tempfile.TemporaryDirectory() as work:
            exe = build(args.reference, work, True)
            for t in [0.030 + 0.0005 * k for k in range(21)]:
                blob, _ = run(exe, work, sift_scenes.texture(64, 48, 2), dict(sift_scenes.DEFAULTS, peak_threshold=t))
                print(t, struct.unpack_from("<i", blob, 0)[0])
        return
    all_same = True
    for path, cases in ((GOLDEN, sift_scenes.cases()), (GOLDEN_V2, sift_scenes.cases_v2())):
        arrays, counts = generate(args.reference, cases)
        data = archive(arrays)
        print(os.path.relpath(path, ROOT))
        print("\n".join(counts))
        print("%d bytes" % len(data))
        if args.check:
            same = os.path.exists(path) and open(path, "rb").read() == data
            print("identical to the committed file" if same else "DIFFERENT from the committed file")
            all_same = all_same and same
            continue
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(data)
    if args.check:
        sys.exit(0 if all_same else 1)


if __name__ == "__main__":
    main()
