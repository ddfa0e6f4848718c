"""Sequential restatement of dsm_find_initial_pairs: the reference's nested loops walked literally.

  IncrementalMapper::FindInitialImagePair / FindFirstInitialImage / FindSecondInitialImage   src/sfm/incremental_mapper.cc:146-200, 791-930
  IncrementalMapper::EstimateInitialTwoViewGeometry                                          :1121-1176
  TwoViewGeometry::EstimateRelativePose                                                       src/estimators/two_view_geometry.cc:169-230
  IncrementalMapper::RegisterInitialImagePair (the triangulation)                             :289-339
  CorrespondenceGraph::AddCorrespondences / FindCorrespondencesBetweenImages                  src/base/correspondence_graph.cc

The correspondence graph is a dict, init_image_pairs_ a set.  Where the reference iterates an unordered map or sorts unstably
the rulings of DESIGN.md 29 apply (ties to the smaller image id).  EstimateCalibrated is the oracle's
(oracle.estimate_two_view_geometry on cameras copied with the prior flag set, a fresh stream seeded with pair_seed(id1, id2,
user_seed)); the pose of a CALIBRATED / UNCALIBRATED geometry is the oracle's PoseFromEssentialMatrix, of a planar one the
oracle's own (qvec, tvec); TriangulatePoint and ImageToWorld are the oracle's; the angles, Median, the acceptance tests and
the point gates are scalar Python floats in the device's operation order.  acos is math.acos unless another one is passed (the
CPU test passes the host build's correctly rounded acos where it asks for equal bits)."""
import math

import numpy as np

from dagsfm_amd import capi

EPS = 2.220446049250313e-16
DEG = 0.0174532925199432954743716805978692718781530857086181640625  # DegToRad, util/math.h:198-200
NO_IMAGE = 0xFFFFFFFF


def default_options(**kw):
    o = dict(init_min_num_inliers=100, init_max_error=4.0, init_max_forward_motion=0.95, init_min_tri_angle=16.0, init_max_reg_trials=2,
             user_seed=0)
    o.update({k: v for k, v in kw.items() if k != "speculation_window"})
    return o


class Margins:
    def __init__(self):
        self.tri_angle = self.forward = self.point_angle = self.point_depth = math.inf

    def acceptance(self):
        return min(self.tri_angle, self.forward)

    def points(self):
        return min(self.point_angle, self.point_depth)


# ------------------------------------------------------------------ the exact pieces, in the device's operation order
def quat_to_R(q):
    """NormalizeQuaternion + Eigen's toRotationMatrix (pose.cc:75-91), row-major."""
    q0, q1, q2, q3 = (float(v) for v in q)
    nq = math.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w, x, y, z = (1.0, q1, q2, q3) if nq == 0 else (q0 / nq, q1 / nq, q2 / nq, q3 / nq)
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]


def compose_P(q, t):
    R = quat_to_R(q)
    return [R[0], R[1], R[2], float(t[0]), R[3], R[4], R[5], float(t[1]), R[6], R[7], R[8], float(t[2])]


def projection_center(q, t):
    """ProjectionCenterFromPose (pose.cc:164-171): Eigen's quaternion-vector product of the conjugate and -tvec."""
    q0, q1, q2, q3 = (float(v) for v in q)
    nq = math.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w = 1.0 if nq == 0 else q0 / nq
    qv = [-(q1 if nq == 0 else q1 / nq), -(q2 if nq == 0 else q2 / nq), -(q3 if nq == 0 else q3 / nq)]
    v = [-float(t[0]), -float(t[1]), -float(t[2])]
    uv = [qv[1] * v[2] - qv[2] * v[1], qv[2] * v[0] - qv[0] * v[2], qv[0] * v[1] - qv[1] * v[0]]
    uv = [a + a for a in uv]
    c = [qv[1] * uv[2] - qv[2] * uv[1], qv[2] * uv[0] - qv[0] * uv[2], qv[0] * uv[1] - qv[1] * uv[0]]
    return [(v[k] + w * uv[k]) + c[k] for k in range(3)]


def minus_Rt_t(R, t):
    return [-((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]) for k in range(3)]


def tri_angle(c1, c2, X, acos=math.acos):
    """CalculateTriangulationAngle = one element of CalculateTriangulationAngles (triangulation.cc:122-181)."""
    d = [c1[k] - c2[k] for k in range(3)]
    b = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    d = [X[k] - c1[k] for k in range(3)]
    r1 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    d = [X[k] - c2[k] for k in range(3)]
    r2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    den = 2.0 * math.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    q = ((r1 + r2) - b) / den
    if not -1.0 <= q <= 1.0:
        return math.nan
    a = acos(q)
    o = math.pi - a
    return o if o < a else a


def median(a):
    """Median (util/math.h:211-229)."""
    s = sorted(a)
    mid = len(s) // 2
    return (s[mid] + s[mid - 1]) / 2.0 if len(s) % 2 == 0 else s[mid]


def accept(num_inliers, tz, angle, o, mg):
    """incremental_mapper.cc:1166-1169, the && chain as it runs."""
    if not num_inliers >= o["init_min_num_inliers"]:
        return False
    az, mf, thr = abs(tz), o["init_max_forward_motion"], o["init_min_tri_angle"] * DEG
    mg.forward = min(mg.forward, abs(az - mf) / max(mf, EPS))
    if not az < mf:
        return False
    mg.tri_angle = min(mg.tri_angle, abs(angle - thr) / max(thr, EPS))
    return angle > thr


def row2(P, X):
    return P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11]


def depth_ok(P, X, mg):
    z = row2(P, X)
    mg.point_depth = min(mg.point_depth, abs(z - EPS) / max(abs(z), EPS))
    return z >= EPS


def point_gates(angle, min_angle, P1, P2, X, mg):
    mg.point_angle = min(mg.point_angle, abs(angle - min_angle) / max(min_angle, EPS))
    if not angle >= min_angle:
        return False
    return depth_ok(P1, X, mg) and depth_ok(P2, X, mg)


I34 = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]


# ------------------------------------------------------------------ the scene as the mapper sees it
class View:
    """One problem's DatabaseCache: the images of the subset, the correspondence graph of the pairs inside it."""

    def __init__(self, scene, problem):
        self.s = scene
        self.ids = [int(i) for i in problem["image_ids"]]
        inside = set(self.ids)
        n = len(self.ids)
        self.num_registrations = dict(zip(self.ids, [int(x) for x in problem.get("num_registrations", [0] * n)]))
        self.init_num_reg_trials = dict(zip(self.ids, [int(x) for x in problem.get("init_num_reg_trials", [0] * n)]))
        self.init_image_pairs = {frozenset((int(a), int(b))) for a, b in problem.get("tried_pairs", [])}
        self.seed1, self.seed2 = problem.get("seed_image1"), problem.get("seed_image2")
        self.img_of_id = {int(i): k for k, i in enumerate(scene["image_ids"])}
        cam_of = {int(c): k for k, c in enumerate(scene["camera_ids"])}
        self.camera = {i: scene["cameras"][cam_of[int(scene["image_camera_ids"][self.img_of_id[i]])]] for i in self.ids}
        self.off = np.asarray(scene["points2D_offsets"], np.int64)
        self.xy = np.asarray(scene["points2D_xy"], np.float64).reshape(-1, 2)
        # CorrespondenceGraph::AddCorrespondences per pair in load order, with its duplicate rule
        self.corrs = {}
        pairs = np.asarray(scene["pairs"], np.int64).reshape(-1, 2)
        moff = np.asarray(scene["match_offsets"], np.int64)
        m = np.asarray(scene["matches"], np.int64).reshape(-1, 2)
        for k, (id1, id2) in enumerate(pairs):
            id1, id2 = int(id1), int(id2)
            if id1 not in inside or id2 not in inside:
                continue
            for i1, i2 in m[moff[k]:moff[k + 1]]:
                c1 = self.corrs.setdefault((id1, int(i1)), [])
                c2 = self.corrs.setdefault((id2, int(i2)), [])
                if any(c[0] == id2 for c in c1) or any(c[0] == id1 for c in c2):
                    continue
                c1.append((id2, int(i2)))
                c2.append((id1, int(i1)))

    def num_points2D(self, i):
        k = self.img_of_id[i]
        return int(self.off[k + 1] - self.off[k])

    def points(self, i):
        k = self.img_of_id[i]
        return self.xy[self.off[k]:self.off[k + 1]]

    def num_correspondences(self, i):
        return sum(len(self.corrs.get((i, k), ())) for k in range(self.num_points2D(i)))

    def find_correspondences_between_images(self, id1, id2):
        return [(k, c[1]) for k in range(self.num_points2D(id1)) for c in self.corrs.get((id1, k), ()) if c[0] == id2]

    def prior(self, i):
        return bool(self.camera[i].has_prior_focal_length)


def find_first_initial_image(v, o):
    infos = []
    for i in sorted(v.ids):
        if v.num_correspondences(i) == 0:
            continue
        if v.init_num_reg_trials.get(i, 0) >= o["init_max_reg_trials"]:
            continue
        if v.num_registrations.get(i, 0) > 0:
            continue
        infos.append((not v.prior(i), -v.num_correspondences(i), i))
    return [i for _, _, i in sorted(infos)]


def find_second_initial_image(v, o, id1):
    num = {}
    for k in range(v.num_points2D(id1)):
        for c in v.corrs.get((id1, k), ()):
            if v.num_registrations.get(c[0], 0) == 0:
                num[c[0]] = num.get(c[0], 0) + 1
    infos = [(not v.prior(i), -n, i) for i, n in num.items() if n >= o["init_min_num_inliers"]]
    return [i for _, _, i in sorted(infos)]


def find_initial_image_pair(v, o, estimate):
    """FindInitialImagePair's loops; estimate(id1, id2) -> bool.  Returns (found, id1, id2, tried) with the pairs tried in
    this call in order.  Both seeds: the controller's direct RegisterInitialImagePair of that pair."""
    tried = []
    if v.seed1 is not None and v.seed2 is not None:
        tried.append((v.seed1, v.seed2))
        ok = estimate(v.seed1, v.seed2)
        return (ok, v.seed1, v.seed2, tried) if ok else (False, NO_IMAGE, NO_IMAGE, tried)
    if v.seed1 is not None or v.seed2 is not None:
        ids1 = [v.seed1 if v.seed1 is not None else v.seed2]
    else:
        ids1 = find_first_initial_image(v, o)
    for id1 in ids1:
        for id2 in find_second_initial_image(v, o, id1):
            pair = frozenset((id1, id2))
            if pair in v.init_image_pairs:
                continue
            v.init_image_pairs.add(pair)
            tried.append((id1, id2))
            if estimate(id1, id2):
                return True, id1, id2, tried
    return False, NO_IMAGE, NO_IMAGE, tried


def candidate_order(scene, problem, **kw):
    """The whole candidate list of a problem: the loops with an estimation that never succeeds."""
    return find_initial_image_pair(View(scene, problem), default_options(**kw), lambda a, b: False)[3]


# ------------------------------------------------------------------ estimation and triangulation
def forced_prior(cam):
    c = capi.copy_camera(cam)
    c.has_prior_focal_length = 1
    return c


def relative_pose_angle(R, t, uv1, uv2, oracle, acos=math.acos):
    """CheckCheirality (pose.cc:225-247) over the normalised inliers, then Median(CalculateTriangulationAngles(0, -R^T t, .))."""
    P2 = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    rt = [R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2] for i in range(3)]
    max_depth = 1000.0 * math.sqrt(rt[0] * rt[0] + rt[1] * rt[1] + rt[2] * rt[2])
    n2 = math.sqrt(R[2] * R[2] + R[5] * R[5] + R[8] * R[8])
    C1, C2 = [0.0, 0.0, 0.0], minus_Rt_t(R, t)
    angles = []
    for a, b in zip(uv1, uv2):
        X = [float(x) for x in oracle.triangulate_point(np.array(I34).reshape(3, 4), np.array(P2).reshape(3, 4), a, b)]
        d1 = (0.0 * X[0] + 0.0 * X[1] + 1.0 * X[2] + 0.0 * 1.0) * 1.0
        if not (EPS < d1 < max_depth):
            continue
        d2 = (P2[8] * X[0] + P2[9] * X[1] + P2[10] * X[2] + P2[11] * 1.0) * n2
        if not (EPS < d2 < max_depth):
            continue
        angles.append(tri_angle(C1, C2, X, acos))
    return median(angles) if angles else 0.0


def estimate_initial_two_view_geometry(v, o, id1, id2, oracle, mg, acos=math.acos):
    """EstimateInitialTwoViewGeometry.  Returns a dict: ok, tvg (the oracle's record, config resolved), inliers, qvec, tvec,
    tri_angle (EstimateRelativePose's), matches."""
    matches = v.find_correspondences_between_images(id1, id2)
    cam1, cam2 = forced_prior(v.camera[id1]), forced_prior(v.camera[id2])
    to = capi.default_two_view_options(min_num_trials=30, max_error=o["init_max_error"])
    p1, p2 = v.points(id1), v.points(id2)
    tvg, inl = oracle.estimate_two_view_geometry(cam1, p1, cam2, p2, np.array(matches, np.uint32).reshape(-1, 2), to,
                                                 capi.pair_seed(id1, id2, o["user_seed"]))
    out = dict(ok=False, tvg=tvg, inliers=inl, matches=matches, tri_angle=0.0, qvec=list(tvg.qvec), tvec=list(tvg.tvec), config=tvg.config)
    if tvg.config not in (2, 3, 4, 5, 6):  # UNDEFINED, DEGENERATE, WATERMARK (and MULTIPLE) fail
        return out
    uv1 = [oracle.image_to_world(cam1, p1[a]) for a, _ in inl]
    uv2 = [oracle.image_to_world(cam2, p2[b]) for _, b in inl]
    if tvg.config in (2, 3):
        R, t, _ = oracle.pose_from_essential(np.array(list(tvg.E)).reshape(3, 3), np.array(uv1).reshape(-1, 2), np.array(uv2).reshape(-1, 2))
        R, t = [float(x) for x in R.reshape(-1)], [float(x) for x in t]
        out["qvec"], out["tvec"] = [float(x) for x in oracle.rotation_to_quaternion(np.array(R).reshape(3, 3))], t
    else:  # PoseFromHomographyMatrix: the oracle's own choice among the decompositions, through its quaternion
        R, t = quat_to_R(tvg.qvec), [float(x) for x in tvg.tvec]
    angle = relative_pose_angle(R, t, uv1, uv2, oracle, acos)
    if tvg.config in (5, 6) and math.sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) == 0:
        out["config"], angle = 5, 0.0
    elif tvg.config == 6:
        out["config"] = 4
    if out["config"] == 5:
        angle = 0.0
    out["tri_angle"] = angle
    out["ok"] = accept(len(inl), t[2], angle, o, mg)
    return out


def triangulate(v, o, id1, id2, qvec, tvec, oracle, mg, acos=math.acos):
    """RegisterInitialImagePair's loop (:289-339): [(xyz, point2D_idx1, point2D_idx2)] in correspondence order."""
    cam1, cam2 = v.camera[id1], v.camera[id2]
    p1, p2 = v.points(id1), v.points(id2)
    P2, C1, C2 = compose_P(qvec, tvec), [0.0, 0.0, 0.0], projection_center(qvec, tvec)
    min_angle = o["init_min_tri_angle"] * DEG
    out = []
    for a, b in v.find_correspondences_between_images(id1, id2):
        X = [float(x) for x in oracle.triangulate_point(np.array(I34).reshape(3, 4), np.array(P2).reshape(3, 4),
                                                        oracle.image_to_world(cam1, p1[a]), oracle.image_to_world(cam2, p2[b]))]
        if point_gates(tri_angle(C1, C2, X, acos), min_angle, I34, P2, X, mg):
            out.append((X, a, b))
    return out


def find_initial_pairs(scene, problems, oracle, acos=math.acos, **kw):
    """The whole call, problem after problem.  Per problem a dict: found, image_id1, image_id2, tried, estimate (the record of
    the pair found, or None), records (of every pair tried), points, margins (acceptance margins over the candidates tried, point margins of the pair found),
    view."""
    o = default_options(**kw)
    results = []
    for problem in problems:
        v = View(scene, problem)
        mg = Margins()
        records = []

        def estimate(id1, id2):
            records.append(estimate_initial_two_view_geometry(v, o, id1, id2, oracle, mg, acos))
            return records[-1]["ok"]

        found, id1, id2, tried = find_initial_image_pair(v, o, estimate)
        rec = records[-1] if found else None
        points = triangulate(v, o, id1, id2, rec["qvec"], rec["tvec"], oracle, mg, acos) if found else []
        results.append(dict(found=found, image_id1=id1, image_id2=id2, tried=tried, estimate=rec, records=records, points=points,
                            margins=mg, view=v, options=o))
    return results
