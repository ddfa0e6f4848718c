"""The normative restatement of dsm_find_next_images: IncrementalMapper::FindNextImages
(src/sfm/incremental_mapper.cc:202-256, the ranks of :46-73) over the state the reference keeps incrementally --
Image::Increment / DecrementCorrespondenceHasPoint3D (src/base/image.cc:113-137) and VisibilityPyramid::SetPoint / ResetPoint
(src/base/visibility_pyramid.cc:53-106) -- with dicts and sets, one observation at a time.

Two forms of the same quantities:
  Reconstruction   the reference's bookkeeping: counters and pyramids maintained through add_observation / delete_observation
  stateless()      the definition the device call implements: recomputed from the correspondences and the observations' points
tests/test_next_images_cpu.py holds the two to each other over random sequences of added and removed observations, and the
pyramid to the expectations of the reference's visibility_pyramid_test.cc (tests/golden/visibility_pyramid_scores.json)."""
import numpy as np

from tests import initial_pair_ref

NUM_LEVELS = 6  # Image::kNumPoint3DVisibilityPyramidLevels
MAX_VISIBLE_POINTS_NUM, MAX_VISIBLE_POINTS_RATIO, MIN_UNCERTAINTY = 0, 1, 2


def default_options(**kw):
    o = dict(image_selection_method=MIN_UNCERTAINTY, abs_pose_min_num_inliers=30, max_reg_trials=3)  # incremental_mapper.h:87-131
    o.update(kw)
    return o


class VisibilityPyramid:
    def __init__(self, num_levels, width, height):
        self.width, self.height, self.score = int(width), int(height), 0
        self.pyramid = [dict() for _ in range(num_levels)]  # level -> {(cy, cx): count}; level l is dim x dim, dim = 2^(l + 1)
        self.max_score = sum((1 << (level + 1)) ** 4 for level in range(num_levels))

    def cell_for_point(self, x, y):
        assert self.width > 0 and self.height > 0
        max_dim = 1 << len(self.pyramid)

        def cell(v, extent):
            with np.errstate(over="ignore"):
                q = np.float64(max_dim) * np.float64(v) / np.float64(extent)  # max_dim * x / width_, left to right in double
            assert q >= 0 and np.isfinite(v)  # the cast of a negative double to size_t is undefined: the call refuses it
            return max_dim - 1 if q >= max_dim else int(q)

        return cell(x, self.width), cell(y, self.height)

    def set_point(self, x, y):
        assert self.pyramid
        cx, cy = self.cell_for_point(x, y)
        for i in range(len(self.pyramid) - 1, -1, -1):
            level = self.pyramid[i]
            level[(cy, cx)] = level.get((cy, cx), 0) + 1
            if level[(cy, cx)] == 1:
                self.score += (1 << (i + 1)) ** 2  # level.size()
            cx, cy = cx >> 1, cy >> 1
        assert self.score <= self.max_score

    def reset_point(self, x, y):
        assert self.pyramid
        cx, cy = self.cell_for_point(x, y)
        for i in range(len(self.pyramid) - 1, -1, -1):
            level = self.pyramid[i]
            level[(cy, cx)] -= 1
            assert level[(cy, cx)] >= 0
            if level[(cy, cx)] == 0:
                self.score -= (1 << (i + 1)) ** 2
            cx, cy = cx >> 1, cy >> 1
        assert self.score <= self.max_score


class Image:
    def __init__(self, image_id, camera, xy, num_levels=NUM_LEVELS):
        self.image_id, self.xy = image_id, xy
        self.registered = False
        self.point3D = [-1] * len(xy)
        self.num_correspondences_have_point3D = [0] * len(xy)
        self.num_visible_points3D = 0
        self.num_observations = 0
        self.pyramid = VisibilityPyramid(num_levels, camera.width, camera.height)  # Image::SetUp

    def increment_correspondence_has_point3D(self, idx):
        self.num_correspondences_have_point3D[idx] += 1
        if self.num_correspondences_have_point3D[idx] == 1:
            self.num_visible_points3D += 1
        self.pyramid.set_point(self.xy[idx][0], self.xy[idx][1])
        assert self.num_visible_points3D <= self.num_observations

    def decrement_correspondence_has_point3D(self, idx):
        self.num_correspondences_have_point3D[idx] -= 1
        assert self.num_correspondences_have_point3D[idx] >= 0
        if self.num_correspondences_have_point3D[idx] == 0:
            self.num_visible_points3D -= 1
        self.pyramid.reset_point(self.xy[idx][0], self.xy[idx][1])
        assert self.num_visible_points3D <= self.num_observations


class Reconstruction:
    """One problem: its images, the correspondence graph of the pairs inside it (DatabaseCache::Load, with the duplicate rule),
    and the reference's incremental bookkeeping of Reconstruction::SetObservationAsTriangulated / ResetTriObservations."""

    def __init__(self, scene, problem, candidates_only=False):
        self.view = initial_pair_ref.View(scene, problem)
        v = self.view
        self.ids = v.ids
        self.images = {}
        for k, i in enumerate(self.ids):
            if candidates_only and int(problem["registered"][k]):
                continue  # its pyramid is never read, and its coordinates may be ones CellForPoint is undefined for
            self.images[i] = Image(i, v.camera[i], v.points(i))
            # CorrespondenceGraph::Finalize / DatabaseCache: points2D with at least one correspondence
            self.images[i].num_observations = sum(1 for f in range(v.num_points2D(i)) if v.corrs.get((i, f)))
        self.point3D = {}  # (image id, point2D idx) -> point, for every image of the problem
        self.registered = {i: False for i in self.ids}

    def register(self, image_id):
        self.registered[image_id] = True
        if image_id in self.images:
            self.images[image_id].registered = True

    def add_observation(self, image_id, idx, point):
        assert self.registered[image_id], "Reconstruction::AddObservation CHECKs image.IsRegistered()"
        assert (image_id, idx) not in self.point3D and point >= 0
        self.point3D[(image_id, idx)] = point
        for cid, cidx in self.view.corrs.get((image_id, idx), ()):  # SetObservationAsTriangulated
            if cid in self.images:
                self.images[cid].increment_correspondence_has_point3D(cidx)

    def delete_observation(self, image_id, idx):
        del self.point3D[(image_id, idx)]
        for cid, cidx in self.view.corrs.get((image_id, idx), ()):  # ResetTriObservations
            if cid in self.images:
                self.images[cid].decrement_correspondence_has_point3D(cidx)


def stateless(scene, problem, num_levels=NUM_LEVELS):
    """Per image of the problem (num_visible, num_observations, score) from the definition: a point2D is visible when one of
    its correspondences in the problem ends on an observation with a point; the score counts occupied cells per level.  The
    score of a registered image is 0 by the call's definition (only a candidate's pyramid is evaluated)."""
    v = initial_pair_ref.View(scene, problem)
    out = []
    for k, i in enumerate(v.ids):
        pts = v.points(i)
        visible = [f for f in range(len(pts)) if any(problem["obs_point3D"][v.ids.index(c)][cf] >= 0 for c, cf in v.corrs.get((i, f), ()))]
        nobs = sum(1 for f in range(len(pts)) if v.corrs.get((i, f)))
        score = 0
        if not int(problem["registered"][k]):
            pyr = VisibilityPyramid(num_levels, v.camera[i].width, v.camera[i].height)
            cells = {pyr.cell_for_point(pts[f][0], pts[f][1]) for f in visible}
            for level in range(num_levels):
                shift = num_levels - 1 - level
                score += len({(cx >> shift, cy >> shift) for cx, cy in cells}) * (1 << (level + 1)) ** 2
        out.append((len(visible), nobs, score))
    return out


def rank(method, image):
    if method == MAX_VISIBLE_POINTS_NUM:
        return np.float32(image.num_visible_points3D)
    if method == MAX_VISIBLE_POINTS_RATIO:
        return np.float32(image.num_visible_points3D) / np.float32(image.num_observations)
    return np.float32(image.pyramid.score)


def find_next_images_from(recon, problem, o):
    """FindNextImages over a Reconstruction's counters.  The reference sorts an unordered map's content unstably by the rank
    alone: its ties are open, and the ruling closes them by ascending image id."""
    n = len(recon.ids)
    trials = dict(zip(recon.ids, [int(x) for x in problem.get("num_reg_trials", [0] * n)]))
    filtered = {i for i, f in zip(recon.ids, problem.get("filtered", [0] * n)) if int(f)}
    image_ranks, other_image_ranks = [], []
    for i in recon.ids:
        if recon.registered[i]:
            continue
        image = recon.images[i]
        if image.num_visible_points3D < o["abs_pose_min_num_inliers"]:
            continue
        if trials[i] >= o["max_reg_trials"]:
            continue
        r = rank(o["image_selection_method"], image)
        if i not in filtered and trials[i] == 0:
            image_ranks.append((i, r))
        else:
            other_image_ranks.append((i, r))
    out = []
    for bucket in (image_ranks, other_image_ranks):
        out += [i for i, _ in sorted(bucket, key=lambda t: (-float(t[1]), t[0]))]
    return out


def build(scene, problem):
    """The problem's Reconstruction with the state of the call's arguments, reached the way the mapper reaches it: images
    registered, observations added one by one."""
    recon = Reconstruction(scene, problem, candidates_only=True)
    for k, i in enumerate(recon.ids):
        if int(problem["registered"][k]):
            recon.register(i)
    for k, i in enumerate(recon.ids):
        for f, p in enumerate(problem["obs_point3D"][k]):
            if int(p) >= 0:
                recon.add_observation(i, f, int(p))
    return recon


def find_next_images(scene, problems, **kw):
    """What Context.find_next_images returns as results, from the incremental bookkeeping."""
    o = default_options(**kw)
    res = []
    for pr in problems:
        recon = build(scene, pr)
        nv, no, score = [], [], []
        for k, i in enumerate(recon.ids):
            if i in recon.images:
                im = recon.images[i]
                nv.append(im.num_visible_points3D), no.append(im.num_observations), score.append(im.pyramid.score)
            else:  # a registered image: the counts from the definition, the score 0
                t = stateless(scene, pr)[k]
                nv.append(t[0]), no.append(t[1]), score.append(0)
        res.append({"next_image_ids": find_next_images_from(recon, pr, o), "num_visible": np.array(nv, np.uint32),
                    "num_observations": np.array(no, np.uint32), "score": np.array(score, np.uint64)})
    return res


# ================================================================== FindLocalBundle (incremental_mapper.cc:932-1099)
def default_local_bundle_options(**kw):
    o = dict(local_ba_num_images=6, local_ba_min_tri_angle=6.0)  # incremental_mapper.h:98-102
    o.update(kw)
    return o


def exact_acos():
    """The correctly rounded acos of the host build (csrc/exact_acos.h)."""
    from dagsfm_amd import capi
    return capi.initial_pair_host_lib().dsm_ip_host_acos


def percentile(elems, p):
    """Percentile (util/math.h:231-246); std::round rounds halves away from zero.  A NaN orders behind every number (the
    reference's nth_element leaves that open)."""
    assert elems and 0 <= p <= 100
    import math
    x = p / 100 * (len(elems) - 1)
    idx = int(math.floor(x + 0.5))
    idx = max(0, min(len(elems) - 1, idx))
    return sorted(elems, key=lambda a: (a != a, a))[idx]


def deg_to_rad(deg):
    return deg * 0.0174532925199432954743716805978692718781530857086181640625  # DegToRad, util/math.h:198-200


class Model:
    """One problem's Reconstruction as FindLocalBundle reads it: Image::Points2D with their points, Point3D::Track, the poses."""

    def __init__(self, problem):
        self.ids = [int(i) for i in problem["image_ids"]]
        self.registered = dict(zip(self.ids, [int(r) for r in problem["registered"]]))
        self.points2D = {i: [int(p) for p in problem["obs_point3D"][k]] for k, i in enumerate(self.ids)}
        self.qvec = {i: problem["qvec"][k] for k, i in enumerate(self.ids)}
        self.tvec = {i: problem["tvec"][k] for k, i in enumerate(self.ids)}
        self.xyz = np.asarray(problem["point_xyz"], np.float64).reshape(-1, 3)
        self.track = {}
        for i in self.ids:
            for f, p in enumerate(self.points2D[i]):
                if p >= 0:
                    assert self.registered[i]
                    self.track.setdefault(p, []).append((i, f))

    def projection_center(self, i):
        return initial_pair_ref.projection_center(self.qvec[i], self.tvec[i])


def find_local_bundle(problem, image_id, acos, margins=None, **kw):
    """The reference's text, loop by loop.  Returns a dict: bundle_image_ids; the overlap list (ids, shared, and tri_angle as the
    device reports it: for every image at or above the loosest overlap threshold of a query that enters the chain, else -1);
    lazy_tri_angle: the angles the reference itself computed (-1: never reached)."""
    o = default_local_bundle_options(**kw)
    m = Model(problem)
    assert m.registered[image_id]
    shared_observations = {}
    num_points3D = 0
    for p in m.points2D[image_id]:
        if p >= 0:
            num_points3D += 1
            for tid, _ in m.track[p]:
                if tid != image_id:
                    shared_observations[tid] = shared_observations.get(tid, 0) + 1
    overlapping = sorted(shared_observations.items(), key=lambda t: (-t[1], t[0]))  # the ruling closes the unstable sort's ties
    num_images = o["local_ba_num_images"] - 1
    num_eff_images = min(num_images, len(overlapping))
    res = {"overlap_image_ids": [i for i, _ in overlapping], "overlap_shared": [c for _, c in overlapping],
           "overlap_tri_angle": [-1.0] * len(overlapping), "lazy_tri_angle": [-1.0] * len(overlapping), "accepted_at": [],
           "num_points3D": num_points3D}
    if len(overlapping) == num_eff_images:
        res["bundle_image_ids"] = [i for i, _ in overlapping]
        return res
    min_tri_angle_rad = deg_to_rad(o["local_ba_min_tri_angle"])
    thresholds = [(min_tri_angle_rad / a, b * num_points3D) for a, b in
                  ((1.0, 0.6), (1.5, 0.6), (2.0, 0.5), (2.5, 0.4), (3.0, 0.3), (4.0, 0.2), (5.0, 0.1), (6.0, 0.1))]
    proj_center = m.projection_center(image_id)

    def tri_angle_of(other):
        shared_points3D = [m.xyz[p] for p in m.points2D[image_id] if p >= 0]
        c2 = m.projection_center(other)
        return percentile([initial_pair_ref.tri_angle(proj_center, c2, X, acos) for X in shared_points3D], 75)

    tri_angles = res["lazy_tri_angle"]
    used = [False] * len(overlapping)
    bundle = []
    for t, (th_angle, th_shared) in enumerate(thresholds):
        for idx in range(len(overlapping)):
            if overlapping[idx][1] < th_shared:
                break
            if used[idx]:
                continue
            if tri_angles[idx] < 0.0:
                tri_angles[idx] = tri_angle_of(overlapping[idx][0])
            if margins is not None:
                margins.append(abs(tri_angles[idx] - th_angle) / max(th_angle, 2.220446049250313e-16))
            if tri_angles[idx] >= th_angle:
                bundle.append(overlapping[idx][0])
                res["accepted_at"].append(t)  # the threshold that took it; 8: the fill-up
                used[idx] = True
                if len(bundle) >= num_eff_images:
                    break
        if len(bundle) >= num_eff_images:
            break
    if len(bundle) < num_eff_images:
        for idx in range(len(overlapping)):
            if not used[idx]:
                bundle.append(overlapping[idx][0])
                res["accepted_at"].append(8)
                used[idx] = True
                if len(bundle) >= num_eff_images:
                    break
    res["bundle_image_ids"] = bundle
    for idx, (i, c) in enumerate(overlapping):  # what the device reports: every angle a threshold could reach
        if not c < 0.1 * num_points3D:
            res["overlap_tri_angle"][idx] = tri_angles[idx] if tri_angles[idx] >= 0.0 or tri_angles[idx] != tri_angles[idx] else tri_angle_of(i)
    return res


def find_local_bundles(problems, queries, **kw):
    """What Context.find_local_bundles returns as results, and the smallest margin of a tri_angle against a threshold."""
    acos, margins = exact_acos(), []
    res = [find_local_bundle(problems[p], i, acos, margins, **kw) for p, i in queries]
    finite = [x for x in margins if x == x]
    return res, (min(finite) if finite else float("inf"))
