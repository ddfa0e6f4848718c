"""Sequential numpy restatement of the reconstruction's point filters, what dsm_filter_points3D is compared with:

  Reconstruction::FilterObservationsWithNegativeDepth (src/base/reconstruction.cc:728-746) with DeleteObservation (:264-284):
      the walk over the images, deleting the whole point once its track is at length 2 or less
  FilterPoints3DWithLargeReprojectionError (:1414-1465), FilterPoints3DWithSmallTriangulationAngle (:1352-1412)
  ComputeMeanReprojectionError(track_ids) (:814-858) and the argument-free overload (:797-812)
  the verdict of FilterImages (:748-770) with CameraModelHasBogusParams (src/base/camera_models.h:473-528)

The state is the reference's: per point a track (a list of observation indices, Track::DeleteElement keeps its order) or
deleted.  Scalar arithmetic follows the device's order (csrc/point_filter.hip, csrc/ba_project.h): the rotation of the
normalised quaternion as Eigen's toRotationMatrix, P = ((R0 X0 + R1 X1) + R2 X2) + t per row, the centre -R^T t; depth and e^2
are evaluated per observation up front (they do not change while the filters run).  Margins are the report's: the relative
distance |a - t| / max(|a|, |t|) of every compared value from its threshold."""
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
DBL_MAX = float(np.finfo(np.float64).max)
DEG_TO_RAD = 0.0174532925199432954743716805978692718781530857086181640625  # util/math.h
NUM_PARAMS = (3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12)
TWO_FOCAL = (1, 4, 5, 6, 7, 10)
NEG_DEPTH, REPROJ, TRI_ANGLE, MEAN_ERROR = 1, 2, 4, 8
LANE_CUT = 16  # csrc/point_filter.hip PF_LANE_CUT: tracks up to it take the lane path
SCAN_BLOCK = 1024  # PF_SCAN: items of one block of the compaction's scan (over the n + 1 observation flags)


def default_options(**kw):
    o = dict(max_reproj_error=4.0, min_tri_angle=1.5, min_focal_length_ratio=0.1, max_focal_length_ratio=10.0, max_extra_param=1.0)
    o.update(kw)
    return o


def margin(a, thr):
    if not math.isfinite(a):
        return math.inf
    den = max(abs(a), abs(thr))
    return abs(a - thr) / den if den > 0 else 0.0


def world_to_image(model, p, u, v):
    """CameraModel::WorldToImage in ba_project.h's order (arrays u, v)."""
    p = [float(x) for x in p]
    with np.errstate(all="ignore"):
        if model not in TWO_FOCAL:
            du, dv = _distortion(model, p[3:], u, v)
            return p[0] * (u + du) + p[1], p[0] * (v + dv) + p[2]
        if model == 7:
            omega = p[4]
            radius2 = u * u + v * v
            omega2 = omega * omega
            if omega2 < 1e-4:
                factor = (omega2 * radius2) / 3.0 - omega2 / 12.0 + 1.0
            else:
                t = math.tan(omega / 2.0)
                small = (-2.0 * t * (4.0 * radius2 * t * t - 3.0)) / (3.0 * omega)
                radius = np.sqrt(radius2)
                big = np.arctan(radius * 2.0 * t) / (radius * omega)
                factor = np.where(radius2 < 1e-4, small, big)
            return p[0] * (u * factor) + p[2], p[1] * (v * factor) + p[3]
        if model == 10:
            r = np.sqrt(u * u + v * v)
            theta = np.arctan(r)
            ok = r > EPS
            rs = np.where(ok, r, 1.0)
            u, v = np.where(ok, theta * u / rs, u), np.where(ok, theta * v / rs, v)
        du, dv = _distortion(model, p[4:], u, v)
        return p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]


def _distortion(model, e, u, v):
    if model == 2:
        r2 = u * u + v * v
        radial = e[0] * r2
        return u * radial, v * radial
    if model == 3:
        r2 = u * u + v * v
        radial = e[0] * r2 + e[1] * r2 * r2
        return u * radial, v * radial
    if model == 4:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        radial = e[0] * r2 + e[1] * r2 * r2
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2), v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2))
    if model in (5, 8, 9):
        r = np.sqrt(u * u + v * v)
        ok = r > EPS
        rs = np.where(ok, r, 1.0)
        theta = np.arctan(r)
        theta2 = theta * theta
        if model == 8:
            thetad = theta * (1.0 + e[0] * theta2)
        elif model == 9:
            theta4 = theta2 * theta2
            thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4)
        else:
            theta4 = theta2 * theta2
            theta6 = theta4 * theta2
            theta8 = theta4 * theta4
            thetad = theta * (1.0 + e[0] * theta2 + e[1] * theta4 + e[2] * theta6 + e[3] * theta8)
        return np.where(ok, u * thetad / rs - u, u * 0.0), np.where(ok, v * thetad / rs - v, v * 0.0)
    if model == 6:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        radial = (1.0 + e[0] * r2 + e[1] * r4 + e[4] * r6) / (1.0 + e[5] * r2 + e[6] * r4 + e[7] * r6)
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) - u, v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) - v)
    if model == 10:
        u2, uv, v2 = u * u, u * v, v * v
        r2 = u2 + v2
        r4 = r2 * r2
        r6 = r4 * r2
        r8 = r6 * r2
        radial = e[0] * r2 + e[1] * r4 + e[4] * r6 + e[5] * r8
        return (u * radial + 2.0 * e[2] * uv + e[3] * (r2 + 2.0 * u2) + e[6] * r2,
                v * radial + 2.0 * e[3] * uv + e[2] * (r2 + 2.0 * v2) + e[7] * r2)
    return u * 0.0, v * 0.0


def image_poses(qvec, tvec):
    """Per image: R [N, 9] (row-major) of the normalised quaternion, and the projection centre -R^T t [N, 3]."""
    q = np.asarray(qvec, np.float64).reshape(-1, 4)
    t = np.asarray(tvec, np.float64).reshape(-1, 3)
    nq = np.sqrt(((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3])
    w, x, y, z = q[:, 0] / nq, q[:, 1] / nq, q[:, 2] / nq, q[:, 3] / nq
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)], 1)
    C = np.stack([-((R[:, k] * t[:, 0] + R[:, 3 + k] * t[:, 1]) + R[:, 6 + k] * t[:, 2]) for k in range(3)], 1)
    return R, C


def camera_list(scene):
    """(model, params, width, height) per camera, as Context.filter_points3D builds its dsm_camera array."""
    models = np.asarray(scene["camera_model_ids"], np.int64).reshape(-1)
    params = np.asarray(scene["camera_params"], np.float64).reshape(-1)
    out, at = [], 0
    for c, m in enumerate(models):
        k = NUM_PARAMS[m]
        pr = params[at:at + k]
        at += k
        pp = 2 if m in TWO_FOCAL else 1
        if scene.get("camera_width") is not None:
            w, h = int(scene["camera_width"][c]), int(scene["camera_height"][c])
        else:
            w, h = max(int(np.ceil(2 * pr[pp])), 0), max(int(np.ceil(2 * pr[pp + 1])), 0)
        out.append((int(m), pr, w, h))
    return out


def has_bogus_params(cam, o, mg):
    """CameraModelHasBogusParams; the ratio tests' margins relative to their bounds into mg[0]."""
    m, pr, w, h = cam
    two = m in TWO_FOCAL
    pp, nf = (2, 2) if two else (1, 1)
    cx, cy = pr[pp], pr[pp + 1]
    if cx < 0 or cx > w or cy < 0 or cy > h:
        return True
    max_size = float(max(w, h))
    lo, hi, me = o["min_focal_length_ratio"], o["max_focal_length_ratio"], o["max_extra_param"]
    for i in range(nf):
        ratio = pr[i] / max_size
        with np.errstate(all="ignore"):
            mg[0] = min(mg[0], float(np.float64(abs(ratio - lo)) / np.float64(lo)), float(np.float64(abs(ratio - hi)) / np.float64(hi)))
        if ratio < lo or ratio > hi:
            return True
    first_extra = NUM_PARAMS[m] if m in (0, 1) else (4 if two else 3)
    for i in range(first_extra, NUM_PARAMS[m]):
        if me > 0:
            mg[0] = min(mg[0], abs(abs(pr[i]) - me) / me)
        if abs(pr[i]) > me:
            return True
    return False


def residuals(scene):
    """Per observation: its point, depth (row 2 of the projection matrix . (X, 1)) and e^2 (DBL_MAX behind the camera)."""
    toff = np.asarray(scene["track_offsets"], np.int64).reshape(-1)
    P = len(toff) - 1
    oimg = np.asarray(scene["obs_image"], np.int64).reshape(-1)
    oxy = np.asarray(scene["obs_xy"], np.float64).reshape(-1, 2)
    xyz = np.asarray(scene["xyz"], np.float64).reshape(-1, 3)
    icam = np.asarray(scene["image_camera"], np.int64).reshape(-1)
    opoint = np.repeat(np.arange(P), toff[1:] - toff[:-1])
    R, C = image_poses(scene["qvec"], scene["tvec"])
    t = np.asarray(scene["tvec"], np.float64).reshape(-1, 3)
    T, X = R[oimg], xyz[opoint]
    px = ((T[:, 0] * X[:, 0] + T[:, 1] * X[:, 1]) + T[:, 2] * X[:, 2]) + t[oimg, 0]
    py = ((T[:, 3] * X[:, 0] + T[:, 4] * X[:, 1]) + T[:, 5] * X[:, 2]) + t[oimg, 1]
    pz = ((T[:, 6] * X[:, 0] + T[:, 7] * X[:, 1]) + T[:, 8] * X[:, 2]) + t[oimg, 2]
    e2 = np.full(len(oimg), DBL_MAX)
    front = ~(pz < EPS)
    cams = camera_list(scene)
    ocam = icam[oimg] if len(oimg) else oimg
    for c, (m, pr, _, _) in enumerate(cams):
        k = np.nonzero(front & (ocam == c))[0]
        if len(k):
            x, y = world_to_image(m, pr, px[k] / pz[k], py[k] / pz[k])
            dx, dy = x - oxy[k, 0], y - oxy[k, 1]
            e2[k] = dx * dx + dy * dy
    return opoint, pz, e2, C


def tri_angles(c1, c2, X):
    """CalculateTriangulationAngle (src/base/triangulation.cc:122-145) for arrays of centre pairs; NaN as the reference's."""
    with np.errstate(all="ignore"):
        b, r, s = c1 - c2, X - c1, X - c2
        base2 = (b[:, 0] * b[:, 0] + b[:, 1] * b[:, 1]) + b[:, 2] * b[:, 2]
        ray1 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        ray2 = (s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2]
        den = 2.0 * np.sqrt(ray1 * ray2)
        nom = (ray1 + ray2) - base2
        a = np.abs(np.arccos(nom / np.where(den == 0.0, 1.0, den)))
        c = math.pi - a
        out = np.where(c < a, c, a)  # std::min(a, c): NaN stays NaN
        return np.where(den == 0.0, 0.0, out)


def walk_negative_depth(toff, oimg, negative, num_images):
    """FilterObservationsWithNegativeDepth as the reference runs it: the images in order, every point2D that still has a
    point3D, DeleteObservation.  Returns (tracks: a list per point or None for a deleted point, num_filtered per point)."""
    P = len(toff) - 1
    tracks = [list(range(int(toff[p]), int(toff[p + 1]))) for p in range(P)]
    opoint = np.repeat(np.arange(P), np.asarray(toff[1:]) - np.asarray(toff[:-1]))
    has_point = np.ones(len(oimg), bool)  # Point2D::HasPoint3D
    nf = np.zeros(P, np.int64)
    by_image = [[] for _ in range(num_images)]
    for o, i in enumerate(oimg):
        by_image[int(i)].append(o)
    for i in range(num_images):
        for o in by_image[i]:
            if not has_point[o] or not negative[o]:
                continue
            p = int(opoint[o])
            if len(tracks[p]) <= 2:  # DeleteObservation: DeletePoint3D
                for x in tracks[p]:
                    has_point[x] = False
                tracks[p] = None
            else:
                tracks[p].remove(o)
                has_point[o] = False
            nf[p] += 1
    return tracks, nf


def closed_form_negative_depth(L, n):
    """What the device computes per point: (survives, num_filtered).  The k-th negative meets a track of L - (k - 1) elements
    and deletes the point once that is <= 2; a point without a negative is never visited (so a track of length 0 or 1 without
    one stays -- the issue's L - n >= 2 alone would delete it)."""
    if n == 0:
        return True, 0
    if L - n >= 2:
        return True, n
    return False, min(n, max(L - 1, 1))


def filter_points3D(scene, passes=REPROJ | TRI_ANGLE, point_selected=None, image_selected=None, **options):
    """The passes in bit order over the scene dict of Context.bundle_adjust / Context.filter_points3D.  Returns a dict with the
    device's outputs (point_keep, obs_keep, point_error, kept_track_offsets, kept_obs, image_filtered), the report's counts
    (num_filtered, points_deleted, observations_deleted: [4]), per-point num_filtered [P, 3] and margins [P, 3] (depth, e^2,
    angle), the two means, pairs_evaluated, and the minima of the margins."""
    o = default_options(**options)
    toff = np.asarray(scene["track_offsets"], np.int64).reshape(-1)
    P = len(toff) - 1
    oimg = np.asarray(scene["obs_image"], np.int64).reshape(-1)
    n = len(oimg)
    icam = np.asarray(scene["image_camera"], np.int64).reshape(-1)
    N = len(icam)
    xyz = np.asarray(scene["xyz"], np.float64).reshape(-1, 3)
    opoint, depth, e2, centres = residuals(scene)
    thr2 = o["max_reproj_error"] * o["max_reproj_error"]
    min_angle = o["min_tri_angle"] * DEG_TO_RAD
    # the selection, fixed from the input
    if point_selected is None and image_selected is None:
        sel = np.ones(P, bool)
    else:
        sel = np.zeros(P, bool) if point_selected is None else np.asarray(point_selected).reshape(P) != 0
        if image_selected is not None:
            hit = (np.asarray(image_selected).reshape(N) != 0)[oimg]
            sel = sel.copy()
            np.logical_or.at(sel, opoint[hit], True)
    mg = np.full((P, 3), math.inf)
    nf = np.zeros((P, 3), np.int64)
    pdel, odel = np.zeros(4, np.int64), np.zeros(4, np.int64)
    error = np.full(P, -1.0)
    tracks = [list(range(int(toff[p]), int(toff[p + 1]))) for p in range(P)]
    for p in range(P):
        if (passes & NEG_DEPTH) or (sel[p] and (passes & (REPROJ | MEAN_ERROR))):
            for x in tracks[p]:
                mg[p, 0] = min(mg[p, 0], margin(depth[x], EPS))
    if passes & NEG_DEPTH:  # ignores the selection: the reference's pass has none
        before = [len(t) for t in tracks]
        tracks, nf1 = walk_negative_depth(toff, oimg, depth < EPS, N)
        nf[:, 0] = nf1
        for p in range(P):
            if tracks[p] is None:
                pdel[0] += 1
                odel[0] += before[p]
            else:
                odel[0] += before[p] - len(tracks[p])
    if passes & REPROJ:
        for p in range(P):
            t = tracks[p]
            if t is None or not sel[p]:
                continue
            if len(t) < 2:
                nf[p, 1] += len(t)
                pdel[1] += 1
                odel[1] += len(t)
                tracks[p] = None
                continue
            s, to_delete = 0.0, []
            for x in t:
                if e2[x] != DBL_MAX:
                    mg[p, 1] = min(mg[p, 1], margin(e2[x], thr2))
                if e2[x] > thr2:
                    to_delete.append(x)
                else:
                    s += math.sqrt(e2[x])
            if len(to_delete) >= len(t) - 1:
                nf[p, 1] += len(t)
                pdel[1] += 1
                odel[1] += len(t)
                tracks[p] = None
            else:
                nf[p, 1] += len(to_delete)
                odel[1] += len(to_delete)
                for x in to_delete:
                    t.remove(x)
                error[p] = s / len(t)  # SetError after the deletions: the remaining length
    pairs = 0
    if passes & TRI_ANGLE:
        for p in range(P):
            t = tracks[p]
            if t is None or not sel[p]:
                continue
            keep = False
            if len(t) >= 2:
                i1, i2 = np.tril_indices(len(t), -1)  # the reference's order: i1 ascending, i2 < i1 ascending
                imgs = oimg[t]
                a = tri_angles(centres[imgs[i1]], centres[imgs[i2]], xyz[p][None, :])
                ok = a >= min_angle
                m = [margin(float(v), min_angle) for v in a]
                if ok.any():
                    first = int(np.argmax(ok))
                    keep = True
                    mg[p, 2] = m[first]
                    pairs += first + 1
                else:
                    mg[p, 2] = min(m)
                    pairs += len(a)
            if not keep:
                nf[p, 2] += 1
                pdel[2] += 1
                odel[2] += len(t)
                tracks[p] = None
                error[p] = -1.0
    mean_err, total_len, total_sum = math.nan, 0, 0.0
    sums = np.zeros(P)
    if passes & MEAN_ERROR:
        for p in range(P):
            t = tracks[p]
            if t is None or not sel[p]:
                continue
            s = 0.0
            for x in t:
                if e2[x] == DBL_MAX:
                    continue
                s += math.sqrt(e2[x])
            with np.errstate(all="ignore"):
                error[p] = float(np.float64(s) / np.float64(len(t)))
            total_len += len(t)
            sums[p] = s
        total_sum = float(np.sum(sums[[p for p in range(P) if tracks[p] is not None and sel[p]]])) if P else 0.0
        with np.errstate(all="ignore"):
            mean_err = float(np.float64(total_sum) / np.float64(total_len))
    point_keep = np.array([t is not None for t in tracks], bool).reshape(P)
    obs_keep = np.zeros(n, bool)
    koff = np.zeros(P + 1, np.int64)
    for p in range(P):
        if tracks[p] is not None:
            obs_keep[tracks[p]] = True
            koff[p + 1] = len(tracks[p])
    koff = np.cumsum(koff)
    kept_obs = np.array([x for t in tracks if t is not None for x in t], np.int64)
    error[~point_keep] = -1.0
    have = point_keep & (error != -1.0)
    reg = np.ones(N, bool) if scene.get("image_registered") is None else np.asarray(scene["image_registered"]).reshape(N) != 0
    observed = np.zeros(N, bool)
    observed[oimg[obs_keep]] = True
    bmg = [math.inf]
    bogus = np.array([has_bogus_params(c, o, bmg) for c in camera_list(scene)], bool)
    image_filtered = reg & (~observed | bogus[icam]) if N else np.zeros(0, bool)
    return {"point_keep": point_keep, "obs_keep": obs_keep, "point_error": error, "kept_track_offsets": koff, "kept_obs": kept_obs,
            "image_filtered": image_filtered, "num_filtered": np.append(nf.sum(0), 0), "points_deleted": pdel,
            "observations_deleted": odel, "point_num_filtered": nf, "margins": mg, "selected": sel,
            "mean_reprojection_error": mean_err, "mean_error_observations": total_len,
            "mean_point_error": float(error[have].sum() / have.sum()) if have.any() else 0.0, "pairs_evaluated": pairs,
            "min_depth_margin": float(mg[:, 0].min()) if P else math.inf, "min_error_margin": float(mg[:, 1].min()) if P else math.inf,
            "min_angle_margin": float(mg[:, 2].min()) if P else math.inf, "min_bogus_margin": bmg[0]}


def clear_points(exp, threshold=1e-9):
    """The points all of whose margins are at or above the threshold: they must agree decision for decision."""
    return (exp["margins"] >= threshold).all(1)


def perturbed(scene, seed):
    """The scene with every floating-point input moved by one ulp in a seeded direction."""
    rng = np.random.default_rng(seed)
    out = dict(scene)
    for key in ("camera_params", "qvec", "tvec", "xyz", "obs_xy"):
        a = np.array(scene[key], np.float64, copy=True)
        out[key] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return out


def error_sensitivity(scene, seeds, **kw):
    """The largest relative change of a clear point's error (and of the two means) under one-ulp moves of every input."""
    base = filter_points3D(scene, **kw)
    clear = clear_points(base) & base["point_keep"] & (base["point_error"] > 0)
    worst = 0.0
    for s in seeds:
        got = filter_points3D(perturbed(scene, s), **kw)
        both = clear & got["point_keep"]
        if both.any():
            worst = max(worst, float(np.max(np.abs(got["point_error"][both] - base["point_error"][both]) / base["point_error"][both])))
        for key in ("mean_reprojection_error", "mean_point_error"):
            if math.isfinite(base[key]) and base[key] > 0 and math.isfinite(got[key]):
                worst = max(worst, abs(got[key] - base[key]) / base[key])
    return worst
