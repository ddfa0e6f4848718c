#!/usr/bin/env python3
"""First measurements of dsm_select_source_images: a synthetic sparse model, by default 2 000 images on a ring
around the points and 175 000 points whose tracks of 2 .. 18 images are drawn from a window of neighbouring images -- about
10^7 items (pairs of track elements).  One warm-up call, then the median of --repeats calls (host clock around the call, which
returns with the lists on the host) with the stage times of the last one; against libdsm_source_selection_host.so, the same
header on ONE CPU thread of the same box (the reference is single-threaded, and no earlier commit has this stage).  The lists,
the depth ranges and the pair table of the two must agree byte for byte: exit status 3 otherwise.  Before timing, the `gate`
fixture is held to tests/source_selection_ref.py bit for bit, so that what is timed is what is specified.

    python tools/bench_source_selection.py [--images 2000] [--points 175000] [--max-track 18] [--window 60] [--repeats 20]
                                           [--out profiles/source_selection_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dagsfm_amd import capi  # noqa: E402
from tests import source_selection_fixtures as fx  # noqa: E402


def make_model(n_images, n_points, max_track, window, seed=28):
    rng = np.random.default_rng(seed)
    ang = 2 * np.pi * np.arange(n_images) / n_images
    C = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), 0.5 * rng.normal(size=n_images)], axis=1)
    z = -C / np.linalg.norm(C, axis=1, keepdims=True)
    x = np.cross(z, [0.0, 0.0, 1.0])
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    R = np.stack([x, np.cross(z, x), z], axis=1)  # [n][3][3], rows x, y, z
    T = -np.einsum("nij,nj->ni", R, C)
    xyz = rng.normal(size=(n_points, 3)) * [2.0, 2.0, 1.0]
    lengths = rng.integers(2, max_track + 1, n_points)
    offs = np.zeros(n_points + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths)
    centre = rng.integers(0, n_images, n_points)
    idx = np.empty(int(offs[-1]), dtype=np.uint32)
    for p in range(n_points):  # distinct images of the window around the point's centre image
        pick = rng.choice(window, size=lengths[p], replace=False) - window // 2
        idx[int(offs[p]):int(offs[p + 1])] = (centre[p] + pick) % n_images
    return R.reshape(-1, 9).astype(np.float32), T.astype(np.float32), xyz.astype(np.float32), offs, idx


def same(a, b):
    if a["sources"] != b["sources"] or a["depth_ranges"].tobytes() != b["depth_ranges"].tobytes():
        return False
    return all(x.tobytes() == y.tobytes() for x, y in zip(a["pairs"], b["pairs"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--points", type=int, default=175000)
    ap.add_argument("--max-track", type=int, default=18)
    ap.add_argument("--window", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_selection_bench.json"))
    a = ap.parse_args()
    assert 2 <= a.max_track <= a.window <= a.images
    ctx = capi.Context(0, check=False)
    m = fx.model("gate")
    assert fx.same(ctx.select_source_images(m["R"], m["T"], m["xyz"], m["tracks"]), fx.reference("gate")) is None, "bench parity"

    R, T, xyz, offs, idx = make_model(a.images, a.points, a.max_track, a.window)
    ctx.select_source_images(R, T, xyz, (offs, idx))  # warm-up: code objects, buffers
    walls = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        dev = ctx.select_source_images(R, T, xyz, (offs, idx))
        walls.append(time.perf_counter() - t0)
    ms = ctx.source_selection_time()
    t0 = time.perf_counter()
    host = capi.selection_host(R, T, xyz, (offs, idx))
    host_wall = time.perf_counter() - t0
    wall = statistics.median(walls)
    stages = {k: ms[k] for k in capi.SOURCE_SELECTION_STAGES[:6]}
    row = {"images": a.images, "points": a.points, "track_elements": int(offs[-1]), "items": int(ms["items_count"]), "pairs": int(ms["pairs"]),
           "nan_items": int(ms["nan_items"]), "list_entries": sum(len(s) for s in dev["sources"]), "call_s_median": wall, "call_s_min": min(walls), "call_s_max": max(walls), "call_s": walls,
           "stage_ms_last_call": stages, "dominant_stage": max(stages, key=stages.get), "device_stages_s": sum(stages.values()) / 1e3,
           "items_per_s": ms["items_count"] / wall, "host_one_thread_s": host_wall, "speedup_over_host_one_thread": host_wall / wall,
           "equal_to_host_build": same(dev, host) and host["stats"]["items"] == int(ms["items_count"])}
    print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(row, f, indent=1)
    if not row["equal_to_host_build"]:
        sys.exit(3)


if __name__ == "__main__":
    main()
