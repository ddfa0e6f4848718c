#!/usr/bin/env python3
"""Times the vocabulary training on one MI355X: dsm_retrieval_quantize at 2^18 and 2^21 descriptors with the
reference's defaults (65 536 words, branching 256, 11 iterations), dsm_retrieval_train_embedding on the same descriptors and
the words that came out, and -- where oracle/_ref/libflann_ref.so exists -- the reference's own single-threaded
VisualIndex::Quantize at 2^18 on this machine's CPU, whose words the device's must equal.

Before anything is timed, a case of tests/vocabulary_build_scenes.py must agree with tests/vocabulary_build_ref.py.  Per size:
the wall time of the call (host pointers in, words out; the median of --repeat calls after a warm-up, with the spread), the
per-stage times of dsm_get_vocabulary_build_time, descriptors per second, and the share of the wall time spent in the
sequential pieces the host keeps (the swap partition with its copies, the root's float chains, the draws).

  python tools/bench_vocabulary.py [--sizes 18,21] [--repeat 3] [--out profiles/r23_vocabulary_build.json]
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dagsfm_amd import capi  # noqa: E402
from tests import flann_ref  # noqa: E402
from tests import vocabulary_build_ref as ref  # noqa: E402
from tests import vocabulary_build_scenes as scenes  # noqa: E402


def check(ctx):
    d, nw, b, it, seed = scenes.CASES["batch_edges_1000_300_8"]
    ref.srand(seed)
    rec = ref.Recorder()
    want = ref.quantize(d, nw, b, it, rand=rec)[0]
    # (the same draws replayed, not rand() again: a process's first HIP calls may draw from rand() themselves)
    got = ctx.retrieval_quantize(d, capi.default_vocabulary_build_options(num_visual_words=nw, branching=b, num_iterations=it),
                                 rand=ref.Replay(rec.draws))
    assert got.shape == want.shape and (got == want).all(), "the device's words differ from the restatement's"


def descriptors(n, seed):
    """n descriptors around 4096 modes, generated in pieces (tests/vocabulary_build_scenes.py modes() at once would hold n x 128
    doubles)."""
    rng = np.random.default_rng(seed)
    centres = rng.integers(0, 160, (4096, 128)).astype(np.float32)
    out = np.empty((n, 128), np.uint8)
    for s in range(0, n, 65536):
        k = min(65536, n - s)
        which = rng.integers(0, 4096, k)
        out[s:s + k] = np.clip(np.rint(centres[which] + rng.normal(0.0, 14.0, (k, 128)).astype(np.float32)), 0, 255).astype(np.uint8)
    return out


def reference_cpu(desc, args):
    lib = flann_ref.load()
    cpu_words = np.zeros((args.words, 128), np.uint8)
    lib.flann_ref_seed(7)
    t0 = time.perf_counter()
    count = lib.flann_ref_quantize(desc.ctypes.data, len(desc), args.words, args.branching, args.iterations, cpu_words.ctypes.data)
    return {"seconds": time.perf_counter() - t0, "words_returned": int(count), "words_sha256": hashlib.sha256(cpu_words[:count].tobytes()).hexdigest()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="18,21")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--branching", type=int, default=256)
    ap.add_argument("--iterations", type=int, default=11)
    ap.add_argument("--workgroup-node-max", type=int, default=0)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--cpu-only", action="store_true", help="only the reference's Quantize at 2^18 on this host's CPU (no GPU needed)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_vocabulary_build.json"))
    args = ap.parse_args()
    if args.cpu_only:
        print(json.dumps({"descriptors": 1 << 18, "reference_cpu_single_thread": reference_cpu(descriptors(1 << 18, 18), args)}))
        return
    ctx = capi.Context(0)
    info = ctx.device_info()
    check(ctx)
    o = capi.default_vocabulary_build_options(num_visual_words=args.words, branching=args.branching, num_iterations=args.iterations,
                                              workgroup_node_max=args.workgroup_node_max)
    projection = np.linalg.qr(np.random.default_rng(5).normal(size=(128, 128)))[0][:64].astype(np.float32)
    out = {"tool": "tools/bench_vocabulary.py", "options": {"num_visual_words": args.words, "branching": args.branching,
                                                             "num_iterations": args.iterations, "workgroup_node_max": args.workgroup_node_max},
           "device": {"name": info.name.decode(), "arch": info.arch.decode(), "compute_units": info.compute_units}, "sizes": []}
    for log2 in [int(s) for s in args.sizes.split(",")]:
        n = 1 << log2
        desc = descriptors(n, log2)
        words = None
        wall, stages, embed_wall, embed_ms = [], [], [], []
        for rep in range(args.repeat + 1):  # the first call is the warm-up (code object, first allocations)
            ref.srand(7)
            t0 = time.perf_counter()
            words = ctx.retrieval_quantize(desc, o)
            t1 = time.perf_counter()
            st = ctx.vocabulary_build_time()
            thr, has = ctx.retrieval_train_embedding(desc, words, projection)
            t2 = time.perf_counter()
            if rep:
                wall.append((t1 - t0) * 1e3)
                stages.append(st)
                embed_wall.append((t2 - t1) * 1e3)
                embed_ms.append(ctx.vocabulary_build_time()["embedding"])
        nodes = len(ctx.vocabulary_tree()[0])
        med = float(np.median(wall))
        stage_med = {k: float(np.median([s[k] for s in stages])) for k in capi.VOCABULARY_BUILD_STAGES[:5]}
        device_ms = stage_med["seeding"] + stage_med["assignment"] + stage_med["centre_update"]
        row = {"descriptors": n, "words_returned": int(len(words)), "words_sha256": hashlib.sha256(words.tobytes()).hexdigest(), "tree_nodes": nodes,
               "quantize_wall_ms": {"median": med, "min": float(min(wall)), "max": float(max(wall)), "all": wall},
               "quantize_stage_ms": stage_med, "descriptors_per_s": n / (med * 1e-3),
               "host_sequential_share": {"partition": stage_med["partition"] / med,
                                         "other_host_and_launch_gaps": max(0.0, med - device_ms - stage_med["statistics"] - stage_med["partition"]) / med},
               "embedding_wall_ms": {"median": float(np.median(embed_wall)), "min": float(min(embed_wall)), "max": float(max(embed_wall))},
               "embedding_device_ms": float(np.median(embed_ms)), "words_with_embedding": int(has.sum())}
        if log2 == 18 and not args.no_cpu and flann_ref.load() is not None:
            row["reference_cpu_single_thread"] = reference_cpu(desc, args)
            assert row["reference_cpu_single_thread"]["words_sha256"] == row["words_sha256"], "the device's words differ from the reference's"
        out["sizes"].append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
