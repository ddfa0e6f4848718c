#!/usr/bin/env python3
"""Global rotation averaging (dsm_view_graph_rotation_averaging; GlobalRotationAveraging) on one MI355X over the
view graphs of tools/bench_view_graph.py: the configs[3] shape (10 000 images, 200 neighbours, 2 % corrupted, noise 0.002) and a
sequence graph (10 000 images, +-4 neighbours).

    python tools/bench_rotation_averaging.py [--images 10000] [--out profiles/r07_rotation_averaging.json] [--cpu-images 1000]

Records the device time (HIP events inside the call, after one warm-up call), iteration counts, CG iterations and the largest
final CG residual per graph; separately the CPU time of the numpy restatement (tests/rotation_averaging_ref.py: dense Cholesky,
one thread of numpy/LAPACK -- not the reference build) on the first --cpu-images images of each graph, with the device's
orientation gap to it on that sub-graph."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402
from tools.bench_view_graph import build  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=10000)
    ap.add_argument("--cpu-images", type=int, default=1000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    res = {"metric": "global rotation averaging, device ms per call", "graphs": []}
    for name, k in (("configs3_knn200", 200), ("sequence_pm4", 8)):
        pairs, q, bad = build(a.images, k, 0.02 if k == 200 else 0.0, 0.002, 0)
        ctx.rotation_averaging(pairs, q)  # warm-up
        t0 = time.perf_counter()
        out = ctx.rotation_averaging(pairs, q)
        wall = time.perf_counter() - t0
        r = out["report"].as_dict()
        g = {"graph": name, "images": a.images, "edges": int(len(pairs)), "corrupted": int(bad.sum()), "device_ms": r["device_ms"],
             "call_wall_s": wall, "report": r, "corrupted_filtered": int((out["edge_state"][bad] == 2).sum())}
        if a.cpu_images > 0:
            from tests import rotation_averaging_ref as ref
            sel = (pairs[:, 0] < a.cpu_images) & (pairs[:, 1] < a.cpu_images)
            sp, sq = pairs[sel], q[sel]
            t0 = time.perf_counter()
            exp = ref.rotation_averaging(sp, sq)
            cdt = time.perf_counter() - t0
            dev = ctx.rotation_averaging(sp, sq)
            gap = float(ref.angle_between(dev["orientations"], exp["orientations"]).max())
            g["cpu_restatement"] = {"method": "tests/rotation_averaging_ref.py: numpy, dense Cholesky of the grounded Laplacian",
                                    "images": a.cpu_images, "edges": int(sel.sum()), "seconds": cdt,
                                    "device_ms_same_subgraph": dev["report"].device_ms, "orientation_gap_rad": gap,
                                    "same_decisions": bool(np.array_equal(dev["edge_state"], exp["edge_state"]))}
        res["graphs"].append(g)
        print(json.dumps(g), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
