"""Sequential restatement of IncrementalTriangulator::CompleteImage (src/sfm/incremental_triangulator.cc:119-229), what
dsm_complete_images is compared with.

The state and Complete's walk are tests/track_update_ref.py's (State, complete, sq_error); the correspondence graph,
IsTwoViewObservation, the sampler, ComputeNumTrials, TriangulatePoint, TriangulateMultiViewPoint, the depth test and the
triangulation angle are tests/retriangulation_ref.py's.  Added here: the reprojection residual of EstimateTriangulation
(CalculateSquaredReprojectionError, the projection-matrix overload, projection.cc:138-157: the row dot products in
retriangulation.hip's rt_row order, inv = 1 / z, inv * x, inv * y, DBL_MAX below a depth of epsilon, then WorldToImage), LORANSAC
over it with an explicit min_num_trials, and the loop over an image's point2Ds with the RANSAC option the reference carries from
one point2D to the next: tri_options lives outside the loop and min_num_trials = C(n, 2) is assigned only where the list holds
n <= 15 entries, so a longer list runs with what the last shorter one of the same image left (0 if there was none).

Every decision that rounding could flip records its relative margin, as rt.Margins does: the residual against max_error^2,
equal-count support sums, the angle, the depths; Complete's error and depth margins and the bogus ratios are the State's."""
import math

import numpy as np

from tests import point_filter_ref as pf
from tests import retriangulation_ref as rt
from tests import track_update_ref as tu

MERGE, COMPLETE = tu.MERGE, tu.COMPLETE
EPS, DBL_MAX, DBL_MIN = rt.EPS, rt.DBL_MAX, rt.DBL_MIN
EXHAUSTIVE = 15  # kExhaustiveSamplingThreshold


def default_options(**kw):
    o = tu.default_options(min_angle=1.5, ignore_two_view_tracks=1, ransac_confidence=0.9999, ransac_max_num_trials=10000,
                           max_transitivity=1)
    o.update(kw)
    return o


def check_options(o):
    if o["max_transitivity"] != 1:
        raise ValueError("max_transitivity other than 1")
    if o["ransac_max_num_trials"] < 1 or not 0 < o["ransac_confidence"] < 1:
        raise ValueError("ransac option out of range")
    if not o["min_angle"] >= 0 or not math.isfinite(o["min_angle"]):
        raise ValueError("min_angle out of range")
    for key in ("complete_max_reproj_error", "merge_max_reproj_error"):
        if not o[key] >= 0 or not math.isfinite(o[key]):
            raise ValueError(key + " out of range")


def angle_ok(a, min_angle, mg):
    """rt.angle_ok; min_angle 0 is allowed here and has no margin to record (the device's division gives infinity)"""
    return rt.angle_ok(a, min_angle, mg) if min_angle > 0 else a >= min_angle


def reproj_residual(view, X, mg=None):
    """view: (P, C, uv, camera tuple of State.cam, xy).  mg: an rt.Margins that takes the depth margin."""
    P, _, _, cam, xy = view
    z = rt.row(P, 2, X)
    if mg is not None:
        mg.depth = min(mg.depth, pf.margin(float(z), EPS))
    if z < EPS:
        return DBL_MAX
    x, y = rt.row(P, 0, X), rt.row(P, 1, X)
    inv = 1.0 / z
    px, py = pf.world_to_image(cam[0], cam[1], np.float64(inv * x), np.float64(inv * y))
    dx, dy = np.float64(px) - xy[0], np.float64(py) - xy[1]
    return float(dx * dx + dy * dy)


def loransac_reproj(views, o, mg, min_trials):
    """LORANSAC<TriangulationEstimator x 2, InlierSupportMeasurer, CombinationSampler> with REPROJECTION_ERROR residuals over
    views [(P, C, uv, cam, xy)] and RANSACOptions::min_num_trials = min_trials.  Returns (X or None, mask, num_trials)."""
    n = len(views)
    max_res = o["complete_max_reproj_error"] * o["complete_max_reproj_error"]
    min_ang = o["min_angle"] * rt.DEG
    allc = n * (n - 1) // 2
    max_trials = min(o["ransac_max_num_trials"], allc)

    def support(X):
        c, s = 0, 0.0
        for vw in views:
            r = reproj_residual(vw, X, mg)
            if r != DBL_MAX:
                mg.residual = min(mg.residual, pf.margin(r, max_res))
            if r <= max_res:
                c += 1
                s += r
        return c, s

    def better(c1, s1, c2, s2):
        if c1 > c2:
            return True
        if c1 == c2 and c1 > 0 and s2 != DBL_MAX:  # a tie of two models without an inlier cannot change the outcome
            mg.support = min(mg.support, abs(s1 - s2) / max(max(s1, s2), DBL_MIN))
        return c1 == c2 and s1 < s2

    best_c, best_s, best_X = 0, DBL_MAX, None
    dyn = max_trials
    abort = False
    sampler = rt.combinations(n, max_trials)
    t = 0
    while t < max_trials:
        if abort:
            t += 1
            break
        a, b = sampler[t]
        va, vb = views[a], views[b]
        X = rt.triangulate_point(va[0], vb[0], va[2], vb[2])
        ok = rt.depth_ok(va[0], X, mg) and rt.depth_ok(vb[0], X, mg) and angle_ok(rt.tri_angle(va[1], vb[1], X), min_ang, mg)
        if ok:
            c, s = support(X)
            if better(c, s, best_c, best_s):
                best_c, best_s, best_X = c, s, X
                if c > 2:
                    inl = [vw for vw in views if reproj_residual(vw, X) <= max_res]
                    XL = rt.triangulate_multi([vw[0] for vw in inl], [vw[2] for vw in inl])
                    good = all(rt.depth_ok(vw[0], XL, mg) for vw in inl)
                    if good:
                        good = any(angle_ok(rt.tri_angle(inl[i][1], inl[j][1], XL), min_ang, mg) for i in range(len(inl)) for j in range(i))
                    if good:
                        lc, ls = support(XL)
                        if better(lc, ls, best_c, best_s):
                            best_c, best_s, best_X = lc, ls, XL
                dyn = rt.num_trials(best_c, n, o["ransac_confidence"])
            if t >= dyn and t >= min_trials:
                abort = True
        t += 1
    if best_c < 2:
        return None, None, t
    return best_X, [reproj_residual(vw, best_X) <= max_res for vw in views], t


class Record:
    """what the CompleteImage calls of one run did"""

    def __init__(self):
        self.mg = rt.Margins()
        self.ransac_trials = 0
        self.new_points = 0
        self.new_observations = 0
        self.completed_observations = 0
        self.items = []  # (image index, point2D_idx, list length, min_num_trials used, trials) per estimate


def view_of(st, f):
    i, k = f
    P, C = st.sc.pose[i]
    return (P, C, st.sc.uv(i, k), st.cam[i], st.sc.xy[st.sc.off[i] + k])


def complete_image(st, i, rec):
    """CompleteImage of image index i on the State; returns num_tris."""
    o = st.o
    if not st.reg[i] or st.cam_bogus[i]:
        return 0
    num_tris = 0
    min_num_trials = 0  # tri_options.ransac_options.min_num_trials: set up per image, carried across its point2Ds
    for k in range(st.sc.nfeat(i)):
        f = (i, k)
        if f in st.f2p:
            c = st.complete(st.f2p[f])
            num_tris += c
            rec.completed_observations += c
            continue
        if o["ignore_two_view_tracks"] and rt.is_two_view(st.corrs, f):
            continue
        found = [c for c in st.corrs.get(f, []) if st.reg[c[0]] and not st.cam_bogus[c[0]]]
        if not found or any(c in st.f2p for c in found):
            continue
        lst = found + [f]
        if len(lst) <= EXHAUSTIVE:
            min_num_trials = len(lst) * (len(lst) - 1) // 2
        X, mask, trials = loransac_reproj([view_of(st, c) for c in lst], o, rec.mg, min_num_trials)
        rec.ransac_trials += trials
        rec.items.append((i, k, len(lst), min_num_trials, trials))
        if X is None:
            continue
        track = [c for c, m in zip(lst, mask) if m]
        pid = st.next_id  # AddPoint3D
        st.next_id += 1
        st.points[pid] = [np.array(X, np.float64), track]
        for c in track:
            st.f2p[c] = pid
        st.modified.add(pid)
        num_tris += len(track)
        rec.new_points += 1
        rec.new_observations += len(track)
    return num_tris


def complete_images(scene, image_ids, steps=(), selected=None, next_point3D_id=0, to_world=None, **options):
    """The steps of track_update_ref.update_tracks, then CompleteImage of every listed image in the given order, over one
    State.  Returns update_tracks's dict plus image_num_tris, ransac_trials, the counts and the margins (error, depth, bogus of
    the State; residual, support, angle and the estimates' depth)."""
    o = default_options(**options)
    check_options(o)
    image_ids = [int(i) for i in np.asarray(image_ids, np.int64).reshape(-1)]
    if len(set(image_ids)) != len(image_ids):
        raise ValueError("a repeated image id")
    if selected is not None:
        selected = [int(s) for s in np.asarray(selected, np.uint64).reshape(-1)]
        if len(set(selected)) != len(selected):
            raise ValueError("a repeated selected id")
    st = tu.State(scene, next_point3D_id, **o)
    if to_world is not None:
        st.sc.to_world = to_world
    if any(i not in st.sc.img_of_id for i in image_ids):
        raise ValueError("an unknown image id")
    if selected is not None and any(s not in st.points for s in selected):
        raise ValueError("a selected id that is no point")
    counts = [st.step(int(k), selected) for k in steps]
    rec = Record()
    tris = [complete_image(st, st.sc.img_of_id[i], rec) for i in image_ids]
    ids = sorted(st.points)
    toff, obs = [0], []
    for p in ids:
        for i, k in st.points[p][1]:
            obs.append((st.image_ids[i], k))
        toff.append(len(obs))
    mg = dict(st.mg)
    mg.update(residual=rec.mg.residual, support=rec.mg.support, angle=rec.mg.angle, estimate_depth=rec.mg.depth)
    return {"point_ids": np.array(ids, np.uint64), "xyz": np.array([st.points[p][0] for p in ids], np.float64).reshape(-1, 3),
            "track_offsets": np.array(toff, np.uint64), "track_obs": np.array(obs, np.uint32).reshape(-1, 2),
            "modified": np.array(sorted(st.modified), np.uint64), "step_counts": np.array(counts, np.uint64),
            "image_num_tris": np.array(tris, np.uint64), "complete_trials": st.complete_trials, "merge_trials": st.merge_trials,
            "ransac_trials": rec.ransac_trials, "num_new_points": rec.new_points, "num_new_observations": rec.new_observations,
            "num_completed_observations": rec.completed_observations, "items": rec.items, "margins": mg}


def min_margin(out):
    return min(out["margins"].values())
