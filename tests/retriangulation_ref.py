"""Sequential numpy restatement of re-triangulating the separator images:
IncrementalTriangulator::TriangulateImage for every separator in ascending id, with Find (max_transitivity 1), Continue and
Create (src/sfm/incremental_triangulator.cc:61-117, 419-586), EstimateTriangulation with LORANSAC, InlierSupportMeasurer and
CombinationSampler (src/estimators/triangulation.cc, src/optim/loransac.h:91-233), over the correspondence graph of
CorrespondenceGraph::AddCorrespondences (src/base/correspondence_graph.cc:77-161).

It walks the reference loop one feature at a time and writes every change straight into the feature -> point state, with no
notion of the device's rounds.  Every decision that rounding could flip records its margin (relative, as the device's report):
the inlier tests, equal-count support comparisons, the triangulation angle, the cheirality depths, Continue's choice and
threshold, the bogus-parameter ratios.  Scalar arithmetic follows the device's operation order; the SVD (numpy's LAPACK) and the
symmetric eigen-solver (numpy.linalg.eigh) round differently from the device's Jacobi sweeps, so parity is by tolerance."""
import itertools
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
DBL_MIN = np.finfo(np.float64).tiny
EPS = np.finfo(np.float64).eps
DEG = 0.0174532925199432954743716805978692718032360229492187
COSINE_EDGE = 1.0 - 8 * EPS  # a cosine above it may give acos NaN (an outlier) by rounding alone: margin 0
TWO_FOCAL = {1, 4, 5, 6, 7, 10}
NUM_PARAMS = [3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12]


def default_options(**kw):
    o = dict(create_max_angle_error=2.0, continue_max_angle_error=2.0, min_angle=1.5, min_focal_length_ratio=0.1,
             max_focal_length_ratio=10.0, max_extra_param=1.0, ransac_confidence=0.9999, ransac_min_inlier_ratio=0.02,
             ransac_max_num_trials=10000, ignore_two_view_tracks=1, max_transitivity=1)
    o.update(kw)
    return o


class Margins:
    def __init__(self):
        self.residual = self.support = self.angle = self.depth = self.cont = self.bogus = math.inf

    def min(self):
        return min(self.residual, self.support, self.angle, self.depth, self.cont, self.bogus)


# ------------------------------------------------------------------ sampler and trial counts
def combinations(n, draws):
    """CombinationSampler(2) over n samples: NextCombination's lexicographic order, reset to the first after the last."""
    idx = list(range(n))
    out = []
    for _ in range(draws):
        out.append((idx[0], idx[1]))
        if not next_combination(idx, 2):
            idx = list(range(n))
    return out


def next_combination(v, k):
    """NextCombination (util/math.h:141-172) on v[:k] / v[k:], in place; False after the last combination."""
    first1, last1, first2, last2 = 0, k, k, len(v)
    if first1 == last1 or first2 == last2:
        return False
    m1, m2 = last1, last2 - 1
    while True:
        m1 -= 1
        if not (m1 != first1 and v[m1] >= v[m2]):
            break
    result = m1 == first1 and v[first1] >= v[m2]
    if not result:
        while first2 != m2 and v[m1] >= v[first2]:
            first2 += 1
        first1 = m1
        v[first1], v[first2] = v[first2], v[first1]
        first1 += 1
        first2 += 1
    if first1 != last1 and first2 != last2:
        m1, m2 = last1, first2
        while m1 != first1 and m2 != last2:
            m1 -= 1
            v[m1], v[m2] = v[m2], v[m1]
            m2 += 1
        v[first1:m1] = v[first1:m1][::-1]
        v[first1:last1] = v[first1:last1][::-1]
        v[m2:last2] = v[m2:last2][::-1]
        v[first2:last2] = v[first2:last2][::-1]
    return not result


def num_trials(k, n, confidence):
    """RANSAC::ComputeNumTrials with kMinNumSamples 2, clamped to 32 bits (no inlier: never aborts)."""
    ratio = k / float(n)
    nom = 1 - confidence
    if nom <= 0:
        return 2 ** 32 - 1
    denom = 1 - ratio ** 2
    if denom <= 0:
        return 1
    v = math.log(nom) / math.log(denom) if denom != 1 else -math.inf
    v = math.ceil(v) if math.isfinite(v) else v
    if not (v >= 0) or v >= 4294967295.0:
        return 2 ** 32 - 1
    return int(v)


# ------------------------------------------------------------------ geometry
def pose_matrix(qvec, tvec):
    """[R | t] with R from the normalised quaternion (Eigen's toRotationMatrix), and the centre -R^T t."""
    q0, q1, q2, q3 = (float(x) for x in qvec)
    nq = math.sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3)
    w, x, y, z = q0 / nq, q1 / nq, q2 / nq, q3 / nq
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = [1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)]
    t = [float(v) for v in tvec]
    P = [R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]]
    C = [-((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]) for k in range(3)]
    return P, C


def row(P, r, X):
    return P[4 * r] * X[0] + P[4 * r + 1] * X[1] + P[4 * r + 2] * X[2] + P[4 * r + 3]


def residual(uv, P, X):
    """CalculateNormalizedAngularError(point2D, point3D, proj_matrix), squared."""
    return residual_cos(uv, P, X)[0]


def residual_cos(uv, P, X):
    """the squared angular error and the cosine acos was taken of"""
    u, v = uv
    r1n = math.sqrt((u * u + v * v) + 1.0)
    a0, a1, a2 = row(P, 0, X), row(P, 1, X), row(P, 2, X)
    r2n = math.sqrt((a0 * a0 + a1 * a1) + a2 * a2)
    d = ((u / r1n) * (a0 / r2n) + (v / r1n) * (a1 / r2n)) + (1.0 / r1n) * (a2 / r2n)
    e = math.acos(d) if -1.0 <= d <= 1.0 else math.nan
    return e * e, d


def depth_ok(P, X, mg):
    z = row(P, 2, X)
    mg.depth = min(mg.depth, abs(z - EPS) / max(abs(z), EPS))
    return z >= EPS


def tri_angle(c1, c2, X):
    """CalculateTriangulationAngle (triangulation.cc:122-142)."""
    b = [c1[k] - c2[k] for k in range(3)]
    p = [X[k] - c1[k] for k in range(3)]
    q = [X[k] - c2[k] for k in range(3)]
    base = (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]
    r1 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2]
    r2 = (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]
    den = 2.0 * math.sqrt(r1 * r2)
    if den == 0.0:
        return 0.0
    c = (r1 + r2 - base) / den
    a = abs(math.acos(c)) if -1.0 <= c <= 1.0 else math.nan
    return min(a, math.pi - a) if a == a else math.nan


def angle_ok(a, min_angle, mg):
    mg.angle = min(mg.angle, abs(a - min_angle) / min_angle)
    return a >= min_angle


def triangulate_point(P1, P2, uv1, uv2):
    """TriangulatePoint (triangulation.cc:39-53): the smallest right singular vector of the 4 x 4 system."""
    A = np.array([[uv1[0] * P1[8 + c] - P1[c] for c in range(4)], [uv1[1] * P1[8 + c] - P1[4 + c] for c in range(4)],
                  [uv2[0] * P2[8 + c] - P2[c] for c in range(4)], [uv2[1] * P2[8 + c] - P2[4 + c] for c in range(4)]])
    _, _, vt = np.linalg.svd(A)
    x = vt[3]
    return [float(x[0] / x[3]), float(x[1] / x[3]), float(x[2] / x[3])]


def triangulate_multi(Ps, uvs):
    """TriangulateMultiViewPoint (triangulation.cc:72-89): the eigenvector of the smallest eigenvalue of sum term^T term."""
    A = np.zeros((4, 4))
    for P, (u, v) in zip(Ps, uvs):
        n = math.sqrt((u * u + v * v) + 1.0)
        p = np.array([u / n, v / n, 1.0 / n])
        M = np.array(P).reshape(3, 4)
        T = M - np.outer(p, p @ M)
        A += T.T @ T
    w, V = np.linalg.eigh(A)
    x = V[:, int(np.argmin(w))]
    return [float(x[0] / x[3]), float(x[1] / x[3]), float(x[2] / x[3])]


# ------------------------------------------------------------------ the scene
class Scene:
    """The input of dsm_retriangulate as the restatement reads it.  to_world(camera, xy) -> normalised coordinates; the
    default handles the pinhole models only (tests pass the oracle's ImageToWorld for the others)."""

    def __init__(self, s, to_world=None):
        self.s = s
        self.to_world = to_world or pinhole_to_world
        self.cam_of_id = {int(c): k for k, c in enumerate(s["camera_ids"])}
        self.img_of_id = {int(i): k for k, i in enumerate(s["image_ids"])}
        self.off = np.asarray(s["points2D_offsets"], np.int64)
        self.xy = np.asarray(s["points2D_xy"], np.float64).reshape(-1, 2)
        self.pose = [pose_matrix(q, t) for q, t in zip(np.asarray(s["qvec"], np.float64).reshape(-1, 4),
                                                       np.asarray(s["tvec"], np.float64).reshape(-1, 3))]
        self.uv_cache = {}

    def nfeat(self, i):
        return int(self.off[i + 1] - self.off[i])

    def camera(self, i):
        return self.s["cameras"][self.cam_of_id[int(self.s["image_camera_ids"][i])]]

    def uv(self, i, k):
        key = (i, k)
        if key not in self.uv_cache:
            self.uv_cache[key] = tuple(float(x) for x in self.to_world(self.camera(i), self.xy[self.off[i] + k]))
        return self.uv_cache[key]


def pinhole_to_world(cam, xy):
    p = cam.params
    if cam.model_id == 0:
        return ((xy[0] - p[1]) / p[0], (xy[1] - p[2]) / p[0])
    if cam.model_id == 1:
        return ((xy[0] - p[2]) / p[0], (xy[1] - p[3]) / p[1])
    raise ValueError("pinhole_to_world: model %d needs a to_world" % cam.model_id)


def bogus(cam, o, mg):
    """CameraModelHasBogusParams (camera_models.h:473-528), its ratio margins recorded."""
    mid = cam.model_id
    two = mid in TWO_FOCAL
    pp = 2 if two else 1
    cx, cy = cam.params[pp], cam.params[pp + 1]
    if cx < 0 or cx > cam.width or cy < 0 or cy > cam.height:
        return True
    max_size = float(max(cam.width, cam.height))
    for i in range(2 if two else 1):
        r = cam.params[i] / max_size
        mg.bogus = min(mg.bogus, abs(r - o["min_focal_length_ratio"]) / o["min_focal_length_ratio"],
                       abs(r - o["max_focal_length_ratio"]) / o["max_focal_length_ratio"])
        if r < o["min_focal_length_ratio"] or r > o["max_focal_length_ratio"]:
            return True
    first = NUM_PARAMS[mid] if mid in (0, 1) else (4 if two else 3)
    for i in range(first, NUM_PARAMS[mid]):
        if o["max_extra_param"] > 0:
            mg.bogus = min(mg.bogus, abs(abs(cam.params[i]) - o["max_extra_param"]) / o["max_extra_param"])
        if abs(cam.params[i]) > o["max_extra_param"]:
            return True
    return False


def build_graph(sc):
    """CorrespondenceGraph::AddCorrespondences per pair in input order: corrs[(image index, point2D)] -> [(image index, point2D)]."""
    corrs = {}
    pairs = np.asarray(sc.s["pairs"], np.int64).reshape(-1, 2)
    moff = np.asarray(sc.s["match_offsets"], np.int64)
    m = np.asarray(sc.s["matches"], np.int64).reshape(-1, 2)
    for k, (id1, id2) in enumerate(pairs):
        a, b = sc.img_of_id[int(id1)], sc.img_of_id[int(id2)]
        for i1, i2 in m[moff[k]:moff[k + 1]]:
            c1 = corrs.setdefault((a, int(i1)), [])
            c2 = corrs.setdefault((b, int(i2)), [])
            if any(c[0] == b for c in c1) or any(c[0] == a for c in c2):
                continue  # duplicate
            c1.append((b, int(i2)))
            c2.append((a, int(i1)))
    return corrs


def is_two_view(corrs, f):
    c = corrs.get(f, [])
    if len(c) != 1:
        return False
    return len(corrs.get(c[0], [])) == 1


# ------------------------------------------------------------------ the estimator and LORANSAC
class Problem:
    """the margins and decisions of one (separator, point2D)"""

    def __init__(self):
        self.mg = Margins()
        self.trials = 0
        self.cont = None
        self.points = []  # (xyz, track of (image index, point2D))


def loransac(views, o, mg, rec):
    """LORANSAC<TriangulationEstimator x 2, InlierSupportMeasurer, CombinationSampler> over views [(P, C, uv)]."""
    n = len(views)
    max_res = (o["create_max_angle_error"] * DEG) * (o["create_max_angle_error"] * DEG)
    min_ang = o["min_angle"] * DEG
    allc = n * (n - 1) // 2
    max_trials = min(o["ransac_max_num_trials"], allc)
    min_trials = allc if n <= 15 else 0

    def support(X):
        c, s = 0, 0.0
        for P, C, uv in views:
            r, d = residual_cos(uv, P, X)
            mg.residual = min(mg.residual, abs(r - max_res) / max_res if d <= COSINE_EDGE else 0.0)
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
    sampler = combinations(n, max_trials)
    t = 0
    while t < max_trials:
        if abort:
            t += 1
            break
        a, b = sampler[t]
        (Pa, Ca, uva), (Pb, Cb, uvb) = views[a], views[b]
        X = triangulate_point(Pa, Pb, uva, uvb)
        ok = depth_ok(Pa, X, mg) and depth_ok(Pb, X, mg) and angle_ok(tri_angle(Ca, Cb, X), min_ang, mg)
        if ok:
            c, s = support(X)
            if better(c, s, best_c, best_s):
                best_c, best_s, best_X = c, s, X
                if c > 2:
                    inl = [vw for vw in views if residual(vw[2], vw[0], X) <= max_res]
                    XL = triangulate_multi([vw[0] for vw in inl], [vw[2] for vw in inl])
                    good = all(depth_ok(vw[0], XL, mg) for vw in inl)
                    if good:
                        good = any(angle_ok(tri_angle(inl[i][1], inl[j][1], XL), min_ang, mg) for i in range(len(inl)) for j in range(i))
                    if good:
                        lc, ls = support(XL)
                        if better(lc, ls, best_c, best_s):
                            best_c, best_s, best_X = lc, ls, XL
                dyn = num_trials(best_c, n, o["ransac_confidence"])
            if t >= dyn and t >= min_trials:
                abort = True
        t += 1
    rec.trials += t
    if best_c < 2:
        return None, None
    mask = [residual(uv, P, best_X) <= max_res for P, C, uv in views]
    return best_X, mask


# ------------------------------------------------------------------ TriangulateImage over the separators
def triangulate(scene, separators, options=None, to_world=None, next_point3D_id=0):
    """The sequential loop.  Returns a dict shaped like capi.Context.retriangulate's, plus `problems`: per processed
    (separator id, point2D) with a non-empty list, its Problem record (margins, trials, decisions)."""
    o = default_options(**(options or {}))
    sc = Scene(scene, to_world)
    s = scene
    mg_cam = Margins()
    cam_bogus = [bogus(c, o, mg_cam) for c in s["cameras"]]
    N = len(s["image_ids"])
    ok = [bool(s["registered"][i]) and not cam_bogus[sc.cam_of_id[int(s["image_camera_ids"][i])]] for i in range(N)]
    corrs = build_graph(sc)
    pids = [int(x) for x in np.asarray(s["point3D_ids"], np.uint64)]
    pxyz = [list(map(float, x)) for x in np.asarray(s["point3D_xyz"], np.float64).reshape(-1, 3)]
    next_id = next_point3D_id or ((max(pids) + 1) if pids else 1)
    pt_of = {}  # (image index, point2D) -> point id
    p3 = np.asarray(s["points2D_point3D"], np.int64)
    for i in range(N):
        for k in range(sc.nfeat(i)):
            if p3[sc.off[i] + k] >= 0:
                pt_of[(i, k)] = pids[p3[sc.off[i] + k]]
    xyz_of = dict(zip(pids, pxyz))
    cont_max = o["continue_max_angle_error"] * DEG
    out = dict(new_point_ids=[], new_xyz=[], new_tracks=[], continued=[], problems={}, num_tris_per_separator={})
    seps = sorted(int(x) for x in separators)
    for sid in seps:
        i = sc.img_of_id[sid]
        tris = 0
        if not ok[i]:
            out["num_tris_per_separator"][sid] = 0
            continue
        P, C = sc.pose[i]
        for k in range(sc.nfeat(i)):
            found = [c for c in corrs.get((i, k), []) if ok[c[0]]]
            if not found:
                continue
            rec = Problem()
            out["problems"][(sid, k)] = rec
            ref = (i, k)
            if any(c in pt_of for c in found) and ref not in pt_of:  # Continue
                best, second, target = DBL_MAX, DBL_MAX, None
                uv = sc.uv(i, k)
                for c in found:
                    if c in pt_of:
                        r, d = residual_cos(uv, P, xyz_of[pt_of[c]])
                        err = math.sqrt(r)
                        if not d <= COSINE_EDGE:
                            rec.mg.cont = 0.0
                        if err < best:
                            best, target = err, pt_of[c]
                for c in found:  # the best error on another point: the margin of the choice
                    if c in pt_of and pt_of[c] != target:
                        second = min(second, math.sqrt(residual(uv, P, xyz_of[pt_of[c]])))
                if target is not None:
                    if second != DBL_MAX and best > 0.0:
                        rec.mg.cont = min(rec.mg.cont, (second - best) / best)
                    rec.mg.cont = min(rec.mg.cont, abs(best - cont_max) / cont_max)
                    if best <= cont_max:
                        pt_of[ref] = target
                        rec.cont = target
                        out["continued"].append((sid, k, target))
                        tris += 1
            create = [c for c in found + [ref] if c not in pt_of]  # Create, with its recursion
            go = len(create) >= 2
            if go and o["ignore_two_view_tracks"] and len(create) == 2 and is_two_view(corrs, create[0]):
                go = False
            while go:
                level = [c for c in create if c not in pt_of]
                if len(level) < 2:
                    break
                views = [sc.pose[c[0]] + (sc.uv(*c),) for c in level]
                X, mask = loransac(views, o, rec.mg, rec)
                if X is None:
                    break
                track = [c for c, m in zip(level, mask) if m]
                pid = next_id
                next_id += 1
                xyz_of[pid] = X
                for c in track:
                    pt_of[c] = pid
                rec.points.append((X, track))
                out["new_point_ids"].append(pid)
                out["new_xyz"].append(X)
                out["new_tracks"].append([(int(s["image_ids"][c[0]]), c[1]) for c in track])
                tris += len(track)
                go = len(level) - len(track) >= 3
        out["num_tris_per_separator"][sid] = tris
    out["continued"] = [(sid, k, pid) for sid, k, pid in out["continued"]]
    out["num_tris"] = sum(out["num_tris_per_separator"].values())
    out["bogus_margin"] = mg_cam.bogus
    return out


def min_margin(out):
    m = out["bogus_margin"]
    for rec in out["problems"].values():
        m = min(m, rec.mg.min())
    return m


# ------------------------------------------------------------------ scenes
def random_rotation(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def look_at_qvec(center, target, rng, roll=0.0):
    """a qvec (w, x, y, z) whose camera at `center` looks at `target`."""
    z = np.asarray(target, float) - center
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])  # world -> camera rows
    c, s = math.cos(roll), math.sin(roll)
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ R
    return rot_to_quat(R), R


def rot_to_quat(R):
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        s = math.sqrt(tr + 1.0) * 2
        return np.array([0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    i = int(np.argmax(np.diag(R)))
    j, k = (i + 1) % 3, (i + 2) % 3
    s = math.sqrt(1.0 + R[i, i] - R[j, j] - R[k, k]) * 2
    q = np.zeros(4)
    q[0] = (R[k, j] - R[j, k]) / s
    q[1 + i] = 0.25 * s
    q[1 + j] = (R[j, i] + R[i, j]) / s
    q[1 + k] = (R[k, i] + R[i, k]) / s
    return q


def make_scene(n_images=8, n_points=60, track=(2, 6), noise=0.3, wrong=0.1, existing=0.0, cameras=None, seed=0, extent=2.0,
               dist=8.0, spacing=0.6, unregistered=(), shuffle_points=True, sequence=False):
    """A sequence of cameras on a line looking at a box of points.  Every ground-truth point is observed by a run of
    consecutive images (length drawn from `track`); each image's points2D are shuffled.  Matches connect every pair of images
    that share points (one verified pair each, i < j, in order); a fraction `wrong` of a pair's matches is replaced by a
    random wrong feature.  A fraction `existing` of the ground-truth points is already in the reconstruction, observed by
    all but one of its images.  sequence: every camera looks straight ahead at its own stretch of a long corridor of points
    (for long sequences), instead of all cameras at one box.  cameras: a list of Camera (cycled over the images; default SIMPLE_PINHOLE f 500, 640 x 480).
    Returns (scene dict, ground-truth xyz per new point key)."""
    from dagsfm_amd import capi
    rng = np.random.default_rng(seed)
    cams = cameras or [capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480)]
    X = rng.uniform(-extent, extent, (n_points, 3))
    centers = [np.array([(i - n_images / 2) * spacing, 0.0, -dist]) for i in range(n_images)]
    targets = [[c[0], 0.0, 0.0] if sequence else [0.0, 0.0, 0.0] for c in centers]
    poses = [look_at_qvec(c, tg, rng, roll=rng.uniform(-0.1, 0.1)) for c, tg in zip(centers, targets)]
    img_cam = [i % len(cams) for i in range(n_images)]
    obs = [[] for _ in range(n_images)]  # (point, xy)
    for p in range(n_points):
        L = int(rng.integers(track[0], track[1] + 1))
        L = min(L, n_images)
        first = int(rng.integers(0, n_images - L + 1))
        if sequence:
            X[p, 0] += 0.5 * (centers[first][0] + centers[first + L - 1][0])
        for i in range(first, first + L):
            q, R = poses[i]
            t = -R @ centers[i]
            Xc = R @ X[p] + t
            if Xc[2] <= 0.1:
                continue
            xy = world_to_image(cams[img_cam[i]], Xc[0] / Xc[2], Xc[1] / Xc[2]) + rng.normal(0, noise, 2)
            obs[i].append((p, xy))
    perm_obs = [[obs[i][j] for j in rng.permutation(len(obs[i]))] for i in range(n_images)]
    index = [{p: k for k, (p, _) in enumerate(perm_obs[i])} for i in range(n_images)]
    offs = np.concatenate([[0], np.cumsum([len(o) for o in perm_obs])]).astype(np.uint32)
    xy = np.array([x for o in perm_obs for _, x in o]).reshape(-1, 2)
    pairs, moff, matches = [], [0], []
    for i in range(n_images):
        for j in range(i + 1, min(n_images, i + track[1])):  # runs of <= track[1] images: farther pairs share nothing
            common = [p for p in index[i] if p in index[j]]
            if not common:
                continue
            m = []
            for p in sorted(common, key=lambda p: index[i][p]):
                a, b = index[i][p], index[j][p]
                if rng.random() < wrong:
                    b = int(rng.integers(0, len(perm_obs[j])))
                m.append((a, b))
            # keep the lists one-to-one (a cross-checked matcher's output)
            seen_a, seen_b, mm = set(), set(), []
            for a, b in m:
                if a in seen_a or b in seen_b:
                    continue
                seen_a.add(a)
                seen_b.add(b)
                mm.append((a, b))
            pairs.append((i, j))
            matches.extend(mm)
            moff.append(len(matches))
    p3 = np.full(len(xy), -1, np.int32)
    ex = [p for p in range(n_points) if rng.random() < existing]
    ids = rng.choice(1 << 40, max(len(ex), 1), replace=False)[:len(ex)].astype(np.uint64) + 1
    pxyz = X[ex] + rng.normal(0, 0.001, (len(ex), 3)) if ex else np.zeros((0, 3))
    for q, p in enumerate(ex):
        seen = [i for i in range(n_images) if p in index[i]]
        for i in seen[:-1] if len(seen) > 1 else []:
            p3[offs[i] + index[i][p]] = q
    if shuffle_points and len(ex):
        perm = rng.permutation(len(ex))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        ids, pxyz = ids[perm], pxyz[perm]
        p3 = np.where(p3 >= 0, inv[np.maximum(p3, 0)], -1).astype(np.int32)
    scene = dict(camera_ids=np.arange(len(cams), dtype=np.uint32) + 7, cameras=list(cams),
                 image_ids=np.arange(n_images, dtype=np.uint32) * 3 + 1, image_camera_ids=np.array(img_cam, np.uint32) + 7,
                 registered=np.array([0 if i in unregistered else 1 for i in range(n_images)], np.uint8),
                 qvec=np.array([q for q, _ in poses]), tvec=np.array([-R @ c for (_, R), c in zip(poses, centers)]),
                 points2D_offsets=offs, points2D_xy=xy, points2D_point3D=p3, point3D_ids=ids, point3D_xyz=pxyz,
                 pairs=(np.array(pairs, np.uint32).reshape(-1, 2) * 3 + 1), match_offsets=np.array(moff, np.uint64),
                 matches=np.array(matches, np.uint32).reshape(-1, 2))
    truth = {(int(scene["image_ids"][i]), k): X[p] for i in range(n_images) for k, (p, _) in enumerate(perm_obs[i])}
    return scene, truth


def world_to_image(cam, u, v):
    p = cam.params
    if cam.model_id == 0:
        return np.array([p[0] * u + p[1], p[0] * v + p[2]])
    if cam.model_id == 1:
        return np.array([p[0] * u + p[2], p[1] * v + p[3]])
    # distorted models: invert ImageToWorld's undistortion numerically is not needed -- a small distortion is folded into the
    # observation noise: the pinhole projection with the model's focal and principal point
    two = cam.model_id in TWO_FOCAL
    f1, f2 = (p[0], p[1]) if two else (p[0], p[0])
    c1, c2 = (p[2], p[3]) if two else (p[1], p[2])
    return np.array([f1 * u + c1, f2 * v + c2])
