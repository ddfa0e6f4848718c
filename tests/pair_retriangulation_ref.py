"""Sequential numpy restatement of re-triangulating the under-reconstructed image pairs:
IncrementalTriangulator::Retriangulate (src/sfm/incremental_triangulator.cc:289-390) over the pairs in ascending
(min image id, max image id), with the correspondences of FindCorrespondencesBetweenImages
(src/base/correspondence_graph.cc:223-248), Continue under re_max_angle_error and Create on two views.

It is one loop over the sorted pairs that writes every change straight into the feature -> point state, with no notion of the
device's candidates or rounds.  num_tri_corrs is recounted from the state at every pair's turn.  The graph, the camera test,
LORANSAC and the angular residual are those of tests/retriangulation_ref.py, and the margins are recorded as there."""
import math

import numpy as np

from tests.retriangulation_ref import (COSINE_EDGE, DBL_MAX, DEG, Margins, Scene, bogus, build_graph, default_options,
                                       is_two_view, loransac, make_scene, residual_cos)

NOT_UNDER_RECONSTRUCTED, CLOSED_BY_ITS_TURN, UNREGISTERED, TRIALS_EXHAUSTED, BOGUS_CAMERA, PROCESSED = range(6)
RE_DEFAULTS = dict(re_max_angle_error=5.0, re_min_ratio=0.2, re_max_trials=1)

__all__ = ["retriangulate_pairs", "min_margin", "fold", "make_scene", "default_pair_options"]


def default_pair_options(**kw):
    o = default_options()
    o.update(RE_DEFAULTS)
    o.update(kw)
    return o


class _Trials:
    trials = 0


def pair_correspondences(sc, corrs, a, b):
    """FindCorrespondencesBetweenImages(image a, image b): (point2D of a, point2D of b) in ascending point2D index of a."""
    out = []
    for i in range(sc.nfeat(a)):
        for c in corrs.get((a, i), []):
            if c[0] == b:
                out.append((i, c[1]))
    return out


def retriangulate_pairs(scene, options=None, re_num_trials=None, to_world=None, next_point3D_id=0):
    """The sequential loop.  Returns a dict shaped like capi.Context.retriangulate_pairs's (lists instead of arrays;
    continued and touched as (image id, point2D, point id)), plus counts (the correspondences per case), margins, bogus_margin."""
    o = default_pair_options(**(options or {}))
    sc = Scene(scene, to_world)
    s = scene
    mg = Margins()
    cam_bogus = [bogus(c, o, mg) for c in s["cameras"]]
    N = len(s["image_ids"])
    img_bogus = [cam_bogus[sc.cam_of_id[int(s["image_camera_ids"][i])]] for i in range(N)]
    corrs = build_graph(sc)
    pids = [int(x) for x in np.asarray(s["point3D_ids"], np.uint64)]
    xyz_of = dict(zip(pids, [list(map(float, x)) for x in np.asarray(s["point3D_xyz"], np.float64).reshape(-1, 3)]))
    next_id = next_point3D_id or ((max(pids) + 1) if pids else 1)
    pt_of = {}  # (image index, point2D) -> point id
    p3 = np.asarray(s["points2D_point3D"], np.int64)
    for i in range(N):
        for k in range(sc.nfeat(i)):
            if p3[sc.off[i] + k] >= 0:
                pt_of[(i, k)] = pids[p3[sc.off[i] + k]]
    before = dict(pt_of)
    pairs = np.asarray(s["pairs"], np.int64).reshape(-1, 2)
    K = len(pairs)
    trials = [0] * K if re_num_trials is None else [int(x) for x in re_num_trials]
    re_max = o["re_max_angle_error"] * DEG

    def oriented(k):  # (image1, image2) as image indices: image1 has the smaller id
        id1, id2 = sorted(int(x) for x in pairs[k])
        return sc.img_of_id[id1], sc.img_of_id[id2]

    kept = {k: pair_correspondences(sc, corrs, *oriented(k)) for k in range(K)}

    def num_tri(k):
        a, b = oriented(k)
        return sum(1 for i, j in kept[k] if (a, i) in pt_of and pt_of[(a, i)] == pt_of.get((b, j)))

    open_at_start = [bool(kept[k]) and num_tri(k) / float(len(kept[k])) < o["re_min_ratio"] for k in range(K)]
    status = [NOT_UNDER_RECONSTRUCTED] * K
    counts = dict(both=0, continue_tried=0, continue_taken=0, two_view_skipped=0, create_tried=0, create_taken=0)
    out = dict(new_point_ids=[], new_xyz=[], new_tracks=[], continued=[], num_tris=0)
    for k in sorted(range(K), key=lambda k: tuple(sorted(int(x) for x in pairs[k]))):
        a, b = oriented(k)
        if not kept[k]:
            continue
        if num_tri(k) / float(len(kept[k])) >= o["re_min_ratio"]:
            status[k] = CLOSED_BY_ITS_TURN if open_at_start[k] else NOT_UNDER_RECONSTRUCTED
            continue
        if not s["registered"][a] or not s["registered"][b]:
            status[k] = UNREGISTERED
            continue
        if trials[k] >= o["re_max_trials"]:
            status[k] = TRIALS_EXHAUSTED
            continue
        trials[k] += 1
        if img_bogus[a] or img_bogus[b]:
            status[k] = BOGUS_CAMERA
            continue
        status[k] = PROCESSED
        for i, j in kept[k]:
            f1, f2 = (a, i), (b, j)
            if f1 in pt_of and f2 in pt_of:
                counts["both"] += 1
            elif f1 in pt_of or f2 in pt_of:  # Continue of the feature without a point onto the other's
                g, p = (f2, pt_of[f1]) if f1 in pt_of else (f1, pt_of[f2])
                counts["continue_tried"] += 1
                r, d = residual_cos(sc.uv(*g), sc.pose[g[0]][0], xyz_of[p])
                err = math.sqrt(r) if r == r else math.nan
                if not d <= COSINE_EDGE:
                    mg.cont = 0.0
                if err < DBL_MAX:
                    mg.cont = min(mg.cont, abs(err - re_max) / re_max)
                    if err <= re_max:
                        pt_of[g] = p
                        counts["continue_taken"] += 1
                        out["continued"].append((int(s["image_ids"][g[0]]), g[1], p))
                        out["num_tris"] += 1
            elif o["ignore_two_view_tracks"] and is_two_view(corrs, f1):
                counts["two_view_skipped"] += 1
            else:  # Create over {f1, f2}
                counts["create_tried"] += 1
                X, mask = loransac([sc.pose[f[0]] + (sc.uv(*f),) for f in (f1, f2)], o, mg, _Trials())
                if X is not None:
                    assert all(mask)
                    pt_of[f1] = pt_of[f2] = next_id
                    xyz_of[next_id] = X
                    counts["create_taken"] += 1
                    out["new_point_ids"].append(next_id)
                    out["new_xyz"].append(X)
                    out["new_tracks"].append([(int(s["image_ids"][f[0]]), f[1]) for f in (f1, f2)])
                    out["num_tris"] += 2
                    next_id += 1
    order = sorted(range(N), key=lambda i: int(s["image_ids"][i]))
    out["touched"] = [(int(s["image_ids"][i]), k, pt_of[(i, k)]) for i in order for k in range(sc.nfeat(i))
                      if (i, k) in pt_of and before.get((i, k)) != pt_of[(i, k)]]
    out.update(pair_num_total_corrs=[len(kept[k]) for k in range(K)], pair_num_tri_corrs=[num_tri(k) for k in range(K)],
               pair_status=status, re_num_trials=trials, counts=counts, margins=mg, bogus_margin=mg.bogus)
    return out


def min_margin(out):
    return out["margins"].min()


def fold(scene, touched, new_point_ids, new_xyz):
    """The scene with a call's results added: the new points appended, every touched point2D on its point.
    touched: (image id, point2D, point id) triples."""
    s = dict(scene)
    ids = np.concatenate([np.asarray(scene["point3D_ids"], np.uint64), np.asarray(new_point_ids, np.uint64)])
    xyz = np.concatenate([np.asarray(scene["point3D_xyz"], np.float64).reshape(-1, 3), np.asarray(new_xyz, np.float64).reshape(-1, 3)])
    index = {int(p): q for q, p in enumerate(ids)}
    img = {int(i): k for k, i in enumerate(scene["image_ids"])}
    p3 = np.array(scene["points2D_point3D"], np.int32, copy=True)
    for image_id, k, pid in touched:
        p3[int(scene["points2D_offsets"][img[int(image_id)]]) + int(k)] = index[int(pid)]
    s.update(point3D_ids=ids, point3D_xyz=xyz, points2D_point3D=p3)
    return s
