#!/usr/bin/env python3
"""Regenerates tests/golden/covdet_vlfeat_affine_v1.npz: the cases of tests/affine_sift_scenes.py (estimate_affine_shape = 1)
run through the reference's VLFeat in COLMAP's call sequence, where vl_covdet_extract_affine_shape stands in the place of
vl_covdet_extract_orientations (sift.cc:467-473).

Needs the reference tree (default /root/reference, or --reference DIR); nothing of it is copied into the repository.  The
driver, its two builds (SSE2 as the reference's CMake builds it, and -DVL_DISABLE_SSE2) and the archive are those of
tools/make_covdet_golden.py; the driver is run with its third argument.  Both builds must write identical bytes for every
case (the wall time in the header apart), or the tool fails.

The file holds, per case NAME: NAME/image (uint8), NAME/options (float64, affine_sift_scenes.OPTION_KEYS), NAME/counts (int32:
detected, VLFeat's suppression counter, after the suppression, after the adaptation, kept by the cut, pooling scales), and for
the stages `adapted` (after vl_covdet_extract_affine_shape) and `sorted` (after COLMAP's std::sort): NAME/<stage>_frames
(float32 [n, 6]: x, y, a11, a12, a21, a22), NAME/<stage>_os (int32 [n, 2]), NAME/<stage>_scores (float32 [n, 3]: peak, edge,
orientation); NAME/sorted_index (int32 [n]: the place in `adapted` of every sorted feature) and VLFeat's raw descriptors of the
kept features as in covdet_vlfeat_v1.npz: NAME/raw for affine_sift_scenes.FLOAT_CASES, NAME/digests for the others.  The
detection lists are those of covdet_vlfeat_v1.npz (affine_sift_scenes.V1_CASE) and are not stored again; the tool asserts that
they are the same.

  python tools/make_covdet_affine_golden.py            # rewrite the golden file, print the counts
  python tools/make_covdet_affine_golden.py --check    # regenerate in memory and compare with the committed file
  python tools/make_covdet_affine_golden.py --time W H [--json]  # the SSE2 build's time on one core for texture(W, H); --json
                                                                 # records it for tools/bench_covariant_sift.py --affine
"""
import argparse
import os
import platform
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import affine_sift_ref, affine_sift_scenes, covariant_sift_ref, sift_scenes  # noqa: E402
import make_covdet_golden as base  # noqa: E402
from make_covdet_golden import archive, build  # noqa: E402

GOLDEN = affine_sift_ref.GOLDEN
SIZE_BOUND = 578734  # tests/test_covariant_sift_cpu.py: the largest golden file before covdet_vlfeat_v1.npz
HOST_TIMES = os.path.join(ROOT, "profiles", "covdet_vlfeat_affine_host_times.json")


def run(exe, work, image, o):
    return base.run(exe, work, image, o, extra=["affine"])


def parse(blob, as_floats):
    """base.parse, keeping what this file stores: the third list is the adapted one."""
    rec, seconds = base.parse(blob, as_floats)
    out = {"counts": rec["counts"], "sorted_index": rec["sorted_index"]}
    for k in ("frames", "os", "scores"):
        out["adapted_" + k] = rec["oriented_" + k]
        out["sorted_" + k] = rec["sorted_" + k]
    for k in ("raw", "digests"):
        if k in rec:
            out[k] = rec[k]
    return out, seconds, rec


def summary(name, image, o, rec):
    c = rec["counts"]
    kept = int(c[4])
    h, w = image.shape
    octs = sorted(set(rec["sorted_os"][:kept, 0].tolist()))
    f = rec["sorted_frames"][:kept]
    aniso = int(((f[:, 3] != 0) | (f[:, 2] != f[:, 5])).sum())
    scales = covariant_sift_ref.scale_list(o["domain_size_pooling"], o["dsp_min_scale"], o["dsp_max_scale"], o["dsp_num_scales"])
    padded = sum(covariant_sift_ref.patch_is_padded(rec["sorted_frames"][i], s, w, h, o["first_octave"], o["octave_resolution"])
                 for i in range(kept) for s in scales)
    groups = []
    for os_ in rec["sorted_os"].tolist():
        if groups and groups[-1][0] == tuple(os_):
            groups[-1][1] += 1
        else:
            groups.append([tuple(os_), 1])
    facts = dict(detected=int(c[0]), adapted=int(c[3]), kept=kept, octaves=octs, anisotropic=aniso, padded=padded, patches=kept * len(scales),
                 groups=groups)
    line = "  %-14s detected %4d, adapted %4d, kept %4d, octaves %s, %d anisotropic, %d of %d patches padded" % (
        name, c[0], c[3], kept, octs, aniso, padded, kept * len(scales))
    return line, facts


def check_coverage(facts):
    """The conditions the stored cases must meet between them."""
    f = list(facts.values())
    assert any(x["anisotropic"] >= 1 for x in f), "no case with a frame the adaptation changed"
    assert facts["upright"]["anisotropic"] == 0
    assert any(0 < x["padded"] < x["patches"] for x in f), "no case with padded and unpadded patches"
    assert any(len(x["octaves"]) >= 3 for x in f), "no case with features in three octaves"
    assert facts["checker17"]["kept"] == 1 and facts["flat40x30"]["detected"] == 0
    # the three cuts on `mid` (affine_sift_scenes.MAXF_*), from the group counts of the full run
    full, S = facts["mid"], affine_sift_scenes
    assert full["kept"] == 100
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
    v1 = covariant_sift_ref.golden()
    with tempfile.TemporaryDirectory() as work:
        exe_sse2, exe_plain = build(reference, work, True), build(reference, work, False)
        for name, image, o in affine_sift_scenes.cases():
            a, b = run(exe_sse2, work, image, o), run(exe_plain, work, image, o)
            assert a[:32] == b[:32] and a[base.HEADER:] == b[base.HEADER:], "the SSE2 and the plain build of VLFeat disagree on case %s" % name
            rec, _, full = parse(a, name in affine_sift_scenes.FLOAT_CASES)
            old = v1[affine_sift_scenes.V1_CASE[name]]
            for stage in ("detected", "suppressed"):  # the detection does not see the option
                for k in ("frames", "os", "scores"):
                    assert full["%s_%s" % (stage, k)].tobytes() == old["%s_%s" % (stage, k)].tobytes(), (name, stage, k)
            arrays[name + "/image"] = np.ascontiguousarray(image, np.uint8)
            arrays[name + "/options"] = np.array([o[k] for k in affine_sift_scenes.OPTION_KEYS], np.float64)
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
    ap.add_argument("--json", action="store_true", help="with --time: record the time in profiles/covdet_vlfeat_affine_host_times.json")
    args = ap.parse_args()
    if args.time:
        with tempfile.TemporaryDirectory() as work:
            exe = build(args.reference, work, True)
            image = sift_scenes.texture(args.time[0], args.time[1], 1)
            o = dict(affine_sift_scenes.cases()[0][2])
            rec, seconds, _ = parse(run(exe, work, image, o), False)
            c = rec["counts"]
            print("%d x %d: %d detected, %d adapted, %d kept x %d scales, %.3f s (detection, shape adaptation, descriptors; one core)" % (
                args.time[0], args.time[1], c[0], c[3], c[4], c[5], seconds))
            if args.json:
                import json
                out = json.load(open(HOST_TIMES)) if os.path.exists(HOST_TIMES) else {
                    "what": "time of tools/covdet_golden_driver.cc with its third argument (VLFeat, SSE2 build, one core: detection, "
                            "vl_covdet_extract_affine_shape and the raw descriptors of every pooling scale, default options with "
                            "estimate_affine_shape = 1; no file I/O) on the host that ran tools/make_covdet_affine_golden.py -- not the GPU host"}
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
    assert len(data) <= SIZE_BOUND, "the golden file is above %d bytes" % SIZE_BOUND
    if args.check:
        same = os.path.exists(GOLDEN) and open(GOLDEN, "rb").read() == data
        print("identical to the committed file" if same else "DIFFERENT from the committed file")
        sys.exit(0 if same else 1)
    with open(GOLDEN, "wb") as f:
        f.write(data)


if __name__ == "__main__":
    main()
