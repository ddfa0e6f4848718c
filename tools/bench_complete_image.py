#!/usr/bin/env python3
"""First measurements of dsm_complete_images (IncrementalTriangulator::CompleteImage on the device).

The scene is tools/bench_track_update.py's (cameras on a line, a corridor of points, every point seen by 3 .. 7 consecutive
images, a third of the observations stripped, some points split) with a tenth of the points taken out whole, so the images have
something to create.  The last-registered 1, 16 and 256 images are completed (fewer where the scene has fewer): one warm-up,
then the median of `--repeats` calls -- the call, the host set-up, the device window, the estimates that run ahead and the
ordered commit pass -- with the items, the trials and the new points, and beside it the check build's serial form
(DSM_COMPLETE_IMAGE_SERIAL=1: every estimate on the commit lane), whose result must be the same bytes; exit status 3 otherwise.
Times are host clocks around synchronised phases (the report's), not kernel times."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from dagsfm_amd import capi  # noqa: E402
import bench_track_update  # noqa: E402


def measure(ctx, s, ids, repeats):
    from tests import complete_image_scenes as scenes
    first = ctx.complete_images(s, ids)  # warm-up, and the result that is compared
    wall, reps = [], []
    for _ in range(repeats):
        t = time.perf_counter()
        r = ctx.complete_images(s, ids)["report"]
        wall.append((time.perf_counter() - t) * 1e3)
        reps.append(r)
    med = lambda f: round(statistics.median(f(r) for r in reps), 3)
    rep = first["report"]
    row = {"call_ms": round(statistics.median(wall), 3), "setup_ms": med(lambda r: r.steps.setup_ms), "device_ms": med(lambda r: r.device_ms),
           "graph_ms": med(lambda r: r.steps.graph_ms), "estimate_ms": med(lambda r: r.estimate_ms), "commit_ms": med(lambda r: r.commit_ms),
           "download_ms": med(lambda r: r.steps.download_ms), "rounds": int(rep.num_rounds), "items": int(rep.num_items),
           "estimated_ahead": int(rep.num_estimated_ahead), "serial_items": int(rep.num_serial_items),
           "complete_trials": int(rep.complete_trials), "ransac_trials": int(rep.ransac_trials), "new_points": int(rep.num_new_points),
           "new_observations": int(rep.num_new_observations), "completed_observations": int(rep.num_completed_observations)}
    return row, scenes.result_bytes(first)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=400)
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--without", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--counts", default="1,16,256")
    ap.add_argument("--no-serial", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    from tests import complete_image_scenes as scenes
    t0 = time.time()
    s = scenes.without_points(bench_track_update.make_scene(a.images, a.points, a.seed), a.without, a.seed)
    out = {"images": a.images, "points3D": int(len(s["point3D_ids"])), "points2D": int(s["points2D_offsets"][-1]),
           "track_elements": int(s["track_offsets"][-1]), "pairs": int(len(s["pairs"])), "matches": int(s["match_offsets"][-1]),
           "scene_s": round(time.time() - t0, 2), "completed_images": {}}
    print(json.dumps({k: v for k, v in out.items() if k != "completed_images"}), flush=True)
    counts = sorted({min(int(x), a.images) for x in a.counts.split(",")})
    lists = {n: [int(i) for i in s["image_ids"][::-1][:n]] for n in counts}  # the last registered first
    product = capi.Context(0, check=False)
    base = {}
    for n in counts:
        out["completed_images"][str(n)], base[n] = measure(product, s, lists[n], a.repeats)
    status = 0
    if not a.no_serial:
        # the binding forwards the process's DSM_* variables to a context before every call: the switch goes through the environment,
        # after the product's calls (a check-only switch on a product context is an error)
        os.environ["DSM_COMPLETE_IMAGE_SERIAL"] = "1"
        serial = capi.Context(0, check=True)
        for n in counts:
            srow, sbytes = measure(serial, s, lists[n], a.repeats)
            out["completed_images"][str(n)]["serial_form"] = {k: srow[k] for k in ("call_ms", "device_ms", "estimate_ms", "commit_ms", "serial_items")}
            if sbytes != base[n] or srow["estimated_ahead"] != 0:
                print("MISMATCH: the serial form's result for %d images is not the product's bytes" % n, flush=True)
                status = 3
        del os.environ["DSM_COMPLETE_IMAGE_SERIAL"]
    for n in counts:
        print(json.dumps({n: out["completed_images"][str(n)]}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(status)


if __name__ == "__main__":
    main()
