#!/usr/bin/env python3
"""The NONLINEAR global rotation estimator (dsm_view_graph_rotation_averaging_nonlinear) on one MI355X over random
view graphs of 1 000 x 20, 10 000 x 20 and 50 000 x 30 (images x neighbours), 1 % corrupted edges, noise 0.003: first from
zero, as Run() starts it, then from the result of the robust estimator (dsm_view_graph_rotation_averaging).

    python tools/bench_nonlinear_rotation.py [--sizes 1000x20,10000x20,50000x30] [--out profiles/r20_nonlinear_rotation.json]

Both starts are first checked against the numpy restatement (tests/nonlinear_rotation_ref.py) on the smallest size: the same
termination, iteration count and accept / reject sequence, R_v R_v0^T within 1e-8 rad; where that fails the figures are still
printed, marked, and the tool exits non-zero.  Records per graph and
start the wall time of the call (after one warm-up call), device_ms (HIP events inside the call), LM and CG iteration counts and
the kernel launches per LM iteration; the restatement's CPU time on the smallest size stands beside them as a reported figure
only (numpy, a dense solve: not the reference build).  There is no time target: nothing comparable existed before."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dagsfm_amd import capi  # noqa: E402


def build(n_img, deg, seed=0, noise=0.003, corrupt=0.01):
    """n_img images, each joined to `deg` random others (the graph of tests/test_rotation_averaging._edges_random, vectorised)"""
    rng = np.random.default_rng(seed)
    a = np.repeat(np.arange(n_img), deg)
    b = rng.integers(0, n_img, len(a))
    ok = a != b
    e = np.unique(np.stack([np.minimum(a, b)[ok], np.maximum(a, b)[ok]], 1), axis=0)
    q = rng.normal(size=(n_img, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)

    def mul(x, y):
        return np.stack([x[:, 0] * y[:, 0] - x[:, 1] * y[:, 1] - x[:, 2] * y[:, 2] - x[:, 3] * y[:, 3],
                         x[:, 0] * y[:, 1] + x[:, 1] * y[:, 0] + x[:, 2] * y[:, 3] - x[:, 3] * y[:, 2],
                         x[:, 0] * y[:, 2] - x[:, 1] * y[:, 3] + x[:, 2] * y[:, 0] + x[:, 3] * y[:, 1],
                         x[:, 0] * y[:, 3] + x[:, 1] * y[:, 2] - x[:, 2] * y[:, 1] + x[:, 3] * y[:, 0]], 1)

    rel = mul(q[e[:, 1]], q[e[:, 0]] * np.array([1.0, -1.0, -1.0, -1.0]))
    rel += rng.normal(scale=noise, size=rel.shape)
    bad = rng.random(len(e)) < corrupt
    rel[bad] = rng.normal(size=(int(bad.sum()), 4))
    rel /= np.linalg.norm(rel, axis=1, keepdims=True)
    o = rng.permutation(len(e))
    return e[o].astype(np.uint32), rel[o], bad[o]


def check_against_restatement(ctx, pairs, q, initial):
    from tests import nonlinear_rotation_ref as nl
    from tests import rotation_averaging_ref as ra
    t0 = time.perf_counter()
    exp = nl.rotation_averaging_nonlinear(pairs, q, initial=initial)
    cpu_s = time.perf_counter() - t0
    dev = ctx.rotation_averaging_nonlinear(pairs, q, initial=initial)
    rd, re = dev["report"], exp["report"]
    gap = float(ra.angle_between(nl.relative_to_first(dev["orientations"]), nl.relative_to_first(exp["orientations"])).max())
    same = (rd.termination == re["termination"] and rd.num_iterations == re["num_iterations"]
            and list(dev["trace"][1:, 4].astype(int)) == exp["accepted"] and np.array_equal(dev["edge_state"], exp["edge_state"]))
    return {"method": "tests/nonlinear_rotation_ref.py: numpy, sparse Jacobian, dense solve", "seconds": cpu_s,
            "relative_orientation_gap_rad": gap, "same_decisions": bool(same), "ok": bool(same and gap < 1e-8)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000x20,10000x20,50000x30")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split("x")) for s in a.sizes.split(",")]
    ctx = capi.Context(0)
    res = {"metric": "NONLINEAR global rotation estimator, ms per call", "graphs": []}
    for k, (n_img, deg) in enumerate(sizes):
        pairs, q, bad = build(n_img, deg, seed=k)
        ctx.rotation_averaging(pairs, q)  # warm-up
        t0 = time.perf_counter()
        rob = ctx.rotation_averaging(pairs, q)
        rob_ms = (time.perf_counter() - t0) * 1e3
        for start, initial in (("zero", None), ("robust", rob)):
            g = {"images": n_img, "neighbours": deg, "edges": int(len(pairs)), "corrupted": int(bad.sum()), "start": start}
            if k == 0:
                g["cpu_restatement"] = check_against_restatement(ctx, pairs, q, initial)
            ctx.rotation_averaging_nonlinear(pairs, q, initial=initial)  # warm-up
            t0 = time.perf_counter()
            out = ctx.rotation_averaging_nonlinear(pairs, q, initial=initial)
            g["call_ms"] = (time.perf_counter() - t0) * 1e3
            r = out["report"].as_dict()
            g.update(device_ms=r["device_ms"], lm_iterations=r["num_iterations"], cg_iterations=r["total_cg_iterations"],
                     launches_per_lm_iteration=r["num_kernel_launches"] / max(1, r["num_iterations"]),
                     corrupted_filtered=int((out["edge_state"][bad] == 2).sum()), report=r)
            if start == "robust":
                g["robust_call_ms"] = rob_ms
            res["graphs"].append(g)
            print(json.dumps(g), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    if not all(g["cpu_restatement"]["ok"] for g in res["graphs"] if "cpu_restatement" in g):
        raise SystemExit("the device does not reproduce the restatement on the smallest size: the figures above are not to be used")


if __name__ == "__main__":
    main()
