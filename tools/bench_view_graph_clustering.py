#!/usr/bin/env python3
"""View-graph clustering (dsm_view_graph_cluster, SPECTRAL; ClusteringScenes) on one MI355X over the view graphs
of tools/bench_view_graph.py with seeded inlier counts (15..500) as weights: the configs[3] shape (10 000 images, 200
neighbours, about 1 M edges) and a sequence graph (10 000 images, +-4 neighbours); num_images_ub = 100, so k = 100 clusters
and a block of 200 vectors.

    python tools/bench_view_graph_clustering.py [--images 10000] [--cpu-images 2000] [--out profiles/r08_view_graph_clustering.json]

Records the device time (HIP events inside the call, after one warm-up call), the eigen-solver and k-means iteration counts,
the worst final eigen-residual and the eigen-gap per graph; separately the CPU time of the numpy restatement
(tests/view_graph_clustering_ref.py: dense eigh, numpy/LAPACK -- not the reference build) on the first --cpu-images images of
each graph (k = cpu_images / 100), with the device's result on that sub-graph compared to it."""
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
    ap.add_argument("--cpu-images", type=int, default=2000)
    ap.add_argument("--graphs", default="configs3_knn200,sequence_pm4")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    ctx = capi.Context(0)
    opts = capi.default_clustering_options()
    res = {"metric": "view-graph clustering (SPECTRAL), device ms per call", "graphs": []}
    for name, k in (("configs3_knn200", 200), ("sequence_pm4", 8)):
        if name not in a.graphs.split(","):
            continue
        pairs, _, _ = build(a.images, k, 0.0, 0.0, 0)
        w = np.random.default_rng(1).integers(15, 501, len(pairs)).astype(np.int32)
        ctx.cluster_view_graph(pairs, w, options=opts)  # warm-up
        t0 = time.perf_counter()
        out = ctx.cluster_view_graph(pairs, w, options=opts)
        wall = time.perf_counter() - t0
        r = out["report"].as_dict()
        g = {"graph": name, "images": a.images, "edges": int(len(pairs)), "device_ms": r["device_ms"], "call_wall_s": wall,
             "report": r, "cluster_sizes": [int(len(c)) for c in out["clusters"]]}
        if a.cpu_images > 0:
            from tests import view_graph_clustering_ref as ref
            sel = (pairs[:, 0] < a.cpu_images) & (pairs[:, 1] < a.cpu_images)
            sp, sw = pairs[sel], w[sel]
            t0 = time.perf_counter()
            exp = ref.cluster(sp, sw)
            cdt = time.perf_counter() - t0
            dev = ctx.cluster_view_graph(sp, sw, options=opts)
            kk = exp["k"]
            g["cpu_restatement"] = {"method": "tests/view_graph_clustering_ref.py: numpy, dense eigh of L, k-means++ / Lloyd",
                                    "images": a.cpu_images, "edges": int(sel.sum()), "k": kk, "seconds": cdt,
                                    "device_ms_same_subgraph": dev["report"].device_ms,
                                    "device_eigen_iterations_same_subgraph": dev["report"].eigen_iterations,
                                    "min_decision_margin": ref.min_margin(exp),
                                    "subspace_sine": ref.principal_sine(dev["eigenvectors"], exp["subspace"]),
                                    "eigen_gap": float(exp["eigenvalues"][kk] - exp["eigenvalues"][kk - 1]),
                                    "same_labels": bool(np.array_equal(dev["labels"], exp["labels"])),
                                    "same_edge_clusters": bool(np.array_equal(dev["edge_cluster"], exp["edge_cluster"]))}
        res["graphs"].append(g)
        print(json.dumps({k2: v for k2, v in g.items() if k2 != "cluster_sizes"}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
