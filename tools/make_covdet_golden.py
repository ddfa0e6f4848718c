#!/usr/bin/env python3
"""Regenerates tests/golden/covdet_vlfeat_v1.npz: the cases of tests/covariant_sift_scenes.py run through the reference's
VLFeat (covdet + scalespace + vl_sift_calc_raw_descriptor) in COLMAP's call sequence.

Needs the reference tree (default /root/reference, or --reference DIR); nothing of it is copied into the repository.  The
driver tools/covdet_golden_driver.cc is compiled against lib/VLFeat/{covdet,scalespace,sift,imopv,imopv_sse2,generic,host,
mathop,mathop_sse2,random}.c in a temporary directory, twice: with SSE2 as the reference's CMake builds it (-DVL_DISABLE_AVX
-DVL_DISABLE_OPENMP), and with -DVL_DISABLE_SSE2 added.  Both builds must write identical bytes for every case (the wall
time in the header apart), or the tool fails.

The file holds, per case NAME: NAME/image (uint8), NAME/options (float64, covariant_sift_scenes.OPTION_KEYS), NAME/counts
(int32: detected, VLFeat's suppression counter, after the suppression, after the orientations, kept by the cut, pooling
scales), and for each stage in (detected, suppressed, oriented, sorted): NAME/<stage>_frames (float32 [n, 6]: x, y, a11, a12,
a21, a22), NAME/<stage>_os (int32 [n, 2]), NAME/<stage>_scores (float32 [n, 3]: peak, edge, orientation); NAME/sorted_index
(int32 [n]: the place in `oriented` of every sorted feature) and VLFeat's raw descriptors of the kept features, before the
pooling and in VLFeat's bin order: NAME/raw (float32 [kept, scales, 128]) for covariant_sift_scenes.FLOAT_CASES, NAME/digests
(uint8 [kept, 32], one SHA-256 per feature) for the others.  The archive is written with fixed time stamps.

The coverage conditions the cases must meet are asserted before the file is written (check_coverage).

  python tools/make_covdet_golden.py            # rewrite the golden file, print the counts
  python tools/make_covdet_golden.py --check    # regenerate in memory and compare with the committed file
  python tools/make_covdet_golden.py --time W H [--json]  # the SSE2 build's time on one core for texture(W, H); --json records
                                                          # it for tools/bench_covariant_sift.py
"""
import argparse
import os
import platform
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import covariant_sift_ref, covariant_sift_scenes, sift_scenes  # noqa: E402
from make_sift_golden import archive  # noqa: E402

GOLDEN = covariant_sift_ref.GOLDEN
VL_SOURCES = ["covdet", "scalespace", "sift", "imopv", "imopv_sse2", "generic", "host", "mathop", "mathop_sse2", "random"]
HEADER = 8 * 4 + 8
HOST_TIMES = os.path.join(ROOT, "profiles", "covdet_vlfeat_host_times.json")


def build(reference, out_dir, sse2):
    vl = os.path.join(reference, "lib", "VLFeat")
    if not os.path.isdir(vl):
        raise SystemExit("no reference tree at %s" % reference)
    flags = ["-O2", "-msse2", "-DVL_DISABLE_AVX", "-DVL_DISABLE_OPENMP"] + ([] if sse2 else ["-DVL_DISABLE_SSE2"])
    tag = "sse2" if sse2 else "plain"
    objs = []
    for s in VL_SOURCES:
        objs.append(os.path.join(out_dir, "%s_%s.o" % (s, tag)))
        subprocess.check_call(["gcc"] + flags + ["-I", vl, "-c", os.path.join(vl, s + ".c"), "-o", objs[-1]])
    exe = os.path.join(out_dir, "driver_" + tag)
    subprocess.check_call(["g++", "-O2", "-std=c++14"] + flags + ["-I", vl, "-o", exe, os.path.join(ROOT, "tools", "covdet_golden_driver.cc")] + objs
                          + ["-lm", "-lpthread"])
    return exe


def run(exe, work, image, o, extra=()):
    """One run of the driver; `extra` are further arguments (tools/make_covdet_affine_golden.py passes the third one)."""
    h, w = image.shape
    req, res = os.path.join(work, "request.bin"), os.path.join(work, "result.bin")
    with open(req, "wb") as f:
        f.write(struct.pack("<8i", w, h, o["octave_resolution"], o["first_octave"], o["max_num_features"], o["upright"],
                            o["domain_size_pooling"], o["dsp_num_scales"]))
        f.write(struct.pack("<4d", o["peak_threshold"], o["edge_threshold"], o["dsp_min_scale"], o["dsp_max_scale"]))
        f.write(np.ascontiguousarray(image, np.uint8).tobytes())
    subprocess.check_call([exe, req, res] + list(extra))
    return open(res, "rb").read()


def parse(blob, as_floats):
    counts = np.frombuffer(blob, "<i4", 8, 0)
    seconds = struct.unpack_from("<d", blob, 32)[0]
    at = HEADER
    rec = {"counts": counts[:6].astype(np.int32)}
    for stage, n in zip(covariant_sift_ref.STAGES, (counts[0], counts[2], counts[3], counts[3])):
        words = np.frombuffer(blob, "<i4", 12 * int(n), at).reshape(int(n), 12)
        at += 48 * int(n)
        rec[stage + "_frames"] = words[:, 0:6].copy().view(np.float32)
        rec[stage + "_os"] = words[:, 6:8].astype(np.int32)
        rec[stage + "_scores"] = words[:, 8:11].copy().view(np.float32)
        if stage == "sorted":
            rec["sorted_index"] = words[:, 11].astype(np.int32)
    kept, scales = int(counts[4]), int(counts[5])
    raw = np.frombuffer(blob, "<f4", kept * scales * 128, at).reshape(kept, scales, 128)
    assert at + raw.nbytes == len(blob)
    if as_floats:
        rec["raw"] = raw.astype(np.float32)
    else:
        rec["digests"] = covariant_sift_ref.digest(raw)
    return rec, seconds


def summary(name, image, o, rec):
    """(the line the tool prints, the facts check_coverage reads)"""
    c = rec["counts"]
    kept = int(c[4])
    h, w = image.shape
    octs = sorted(set(rec["sorted_os"][:kept, 0].tolist()))
    idx = rec["sorted_index"]
    # the copies of one detection share (x, y, o, s, peak score)
    keys = [tuple(rec["oriented_frames"][i, :2].tolist()) + tuple(rec["oriented_os"][i].tolist()) for i in range(len(idx))]
    most = max([keys.count(k) for k in set(keys)] or [0])
    scales = covariant_sift_ref.scale_list(o["domain_size_pooling"], o["dsp_min_scale"], o["dsp_max_scale"], o["dsp_num_scales"])
    padded = sum(covariant_sift_ref.patch_is_padded(rec["sorted_frames"][i], s, w, h, o["first_octave"], o["octave_resolution"])
                 for i in range(kept) for s in scales)
    groups = []
    for os_ in rec["sorted_os"].tolist():
        if groups and groups[-1][0] == tuple(os_):
            groups[-1][1] += 1
        else:
            groups.append([tuple(os_), 1])
    facts = dict(detected=int(c[0]), suppressed=int(c[1]), oriented=int(c[3]), kept=kept, octaves=octs, most=most, padded=padded,
                 patches=kept * len(scales), groups=groups)
    line = "  %-14s detected %4d, suppressed %3d, oriented %4d, kept %4d, octaves %s, at most %d orientations, %d of %d patches padded" % (
        name, c[0], c[1], c[3], kept, octs, most, padded, kept * len(scales))
    return line, facts


def check_coverage(facts):
    """The conditions the stored cases must meet between them."""
    f = list(facts.values())
    assert any(x["suppressed"] >= 1 for x in f), "no case with a suppressed feature"
    assert any(x["most"] == 4 for x in f), "no case with a feature of exactly four orientations"
    assert any(x["patches"] and x["padded"] == x["patches"] for x in f), "no case where every patch takes the padded path"
    assert any(x["padded"] < x["patches"] for x in f), "no case where some patches are not padded"
    assert any(len(x["octaves"]) >= 3 for x in f), "no case with features in three octaves"
    assert facts["checker17"]["kept"] == 4 and facts["checker17"]["patches"] == 40
    assert facts["flat40x30"]["detected"] == 0
    # the three cuts on `mid` (covariant_sift_scenes.MAXF_*), from the group counts of the full run
    full, S = facts["mid"], covariant_sift_scenes
    totals = np.cumsum([n for _, n in full["groups"]]).tolist()
    stopped = facts["maxf_octaves"]
    assert min(stopped["octaves"]) > min(full["octaves"]) and stopped["detected"] >= S.MAXF_BETWEEN_OCTAVES, "the detection loop did not stop early"
    assert facts["maxf_inside"]["detected"] == full["detected"] and facts["maxf_groups"]["detected"] == full["detected"]
    assert S.MAXF_BETWEEN_GROUPS in totals[:-1] and facts["maxf_groups"]["kept"] == S.MAXF_BETWEEN_GROUPS + 1, \
        "MAXF_BETWEEN_GROUPS must be a running total of the group counts %s" % totals
    nxt = [t for t in totals if t > S.MAXF_INSIDE_GROUP]
    assert S.MAXF_INSIDE_GROUP not in totals and len(nxt) >= 2 and facts["maxf_inside"]["kept"] == nxt[0] + 1, \
        "MAXF_INSIDE_GROUP must fall inside a group that is not the last (running totals %s)" % totals


def generate(reference):
    arrays, lines, facts = {}, [], {}
    with tempfile.TemporaryDirectory() as work:
        exe_sse2, exe_plain = build(reference, work, True), build(reference, work, False)
        for name, image, o in covariant_sift_scenes.cases():
            a, b = run(exe_sse2, work, image, o), run(exe_plain, work, image, o)
            assert a[:32] == b[:32] and a[HEADER:] == b[HEADER:], "the SSE2 and the plain build of VLFeat disagree on case %s" % name
            rec, _ = parse(a, name in covariant_sift_scenes.FLOAT_CASES)
            arrays[name + "/image"] = np.ascontiguousarray(image, np.uint8)
            arrays[name + "/options"] = np.array([o[k] for k in covariant_sift_scenes.OPTION_KEYS], np.float64)
            for k, v in rec.items():
                arrays[name + "/" + k] = v
            line, facts[name] = summary(name, image, o, rec)
            lines.append(line)
            if name == "mid":
                lines.append("      (o, s) groups of mid in sorted order: %s" % " ".join("%d,%d:%d" % (g[0][0], g[0][1], g[1]) for g in facts[name]["groups"]))
    return arrays, lines, facts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default="/root/reference")
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--no-coverage", action="store_true", help="write or print even where check_coverage fails (while choosing scenes)")
    ap.add_argument("--time", nargs=2, type=int, metavar=("W", "H"))
    ap.add_argument("--json", action="store_true", help="with --time: record the time in profiles/covdet_vlfeat_host_times.json")
    args = ap.parse_args()
    if args.time:
        with tempfile.TemporaryDirectory() as work:
            exe = build(args.reference, work, True)
            image = sift_scenes.texture(args.time[0], args.time[1], 1)
            rec, seconds = parse(run(exe, work, image, covariant_sift_scenes.DEFAULTS), False)
            c = rec["counts"]
            print("%d x %d: %d detected, %d oriented, %d kept x %d scales, %.3f s (detection, orientations, descriptors; one core)" % (
                args.time[0], args.time[1], c[0], c[3], c[4], c[5], seconds))
            if args.json:
                import json
                out = json.load(open(HOST_TIMES)) if os.path.exists(HOST_TIMES) else {
                    "what": "time of tools/covdet_golden_driver.cc (VLFeat, SSE2 build, one core: detection, orientations and the raw "
                            "descriptors of every pooling scale, default options; no file I/O) on the host that ran "
                            "tools/make_covdet_golden.py -- not the GPU host"}
                out["host"] = platform.processor() or platform.machine()
                out["%dx%d" % tuple(args.time)] = {"seconds": round(seconds, 3), "detected": int(c[0]), "features": int(c[4]), "scales": int(c[5])}
                with open(HOST_TIMES, "w") as f:
                    json.dump(out, f, indent=1, sort_keys=True)
                    f.write("\n")
        return
    arrays, lines, facts = generate(args.reference)
    print(os.path.relpath(GOLDEN, ROOT))
    print("\n".join(lines))
    if not args.no_coverage:
        check_coverage(facts)
    data = archive(arrays)
    print("%d bytes" % len(data))
    if args.check:
        same = os.path.exists(GOLDEN) and open(GOLDEN, "rb").read() == data
        print("identical to the committed file" if same else "DIFFERENT from the committed file")
        sys.exit(0 if same else 1)
    with open(GOLDEN, "wb") as f:
        f.write(data)


if __name__ == "__main__":
    main()
