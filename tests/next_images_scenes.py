"""Scenes of dsm_find_next_images: the smallest shapes at which a kernel can still go wrong.  Each scene is
(scene, problems, option keywords); get(name) builds it once."""
import numpy as np

from dagsfm_amd import capi

W, H = 640, 480


class Builder:
    def __init__(self):
        self.cam_ids, self.cams, self.image_ids, self.image_cams, self.xy, self.pairs, self.matches = [], [], [], [], [], [], []

    def camera(self, width=W, height=H):
        self.cam_ids.append(len(self.cam_ids) + 1)
        self.cams.append(capi.simple_pinhole(500.0, width / 2, height / 2, width, height, True))
        return self.cam_ids[-1]

    def image(self, image_id, cam, xy):
        self.image_ids.append(image_id), self.image_cams.append(cam)
        self.xy.append(np.asarray(xy, np.float64).reshape(-1, 2))

    def pair(self, id1, id2, matches):
        self.pairs.append((id1, id2))
        self.matches.append(np.asarray(matches, np.uint32).reshape(-1, 2))

    def n(self, image_id):
        return len(self.xy[self.image_ids.index(image_id)])

    def scene(self):
        off = np.concatenate([[0], np.cumsum([len(x) for x in self.xy])]).astype(np.uint32)
        moff = np.concatenate([[0], np.cumsum([len(m) for m in self.matches])]).astype(np.uint64)
        return dict(camera_ids=np.array(self.cam_ids, np.uint32), cameras=list(self.cams), image_ids=np.array(self.image_ids, np.uint32),
                    image_camera_ids=np.array(self.image_cams, np.uint32), points2D_offsets=off,
                    points2D_xy=np.concatenate(self.xy + [np.zeros((0, 2))]), pairs=np.array(self.pairs, np.uint32).reshape(-1, 2),
                    match_offsets=moff, matches=np.concatenate(self.matches + [np.zeros((0, 2), np.uint32)]))


def problem(b, image_ids, registered, points, trials=None, filtered=()):
    """points: {(image id, point2D idx): point}; trials: {image id: num_reg_trials}."""
    obs = []
    for i in image_ids:
        a = np.full(b.n(i), -1, np.int32)
        for (pi, f), p in points.items():
            if pi == i:
                a[f] = p
        obs.append(a)
    return dict(image_ids=list(image_ids), registered=[int(i in registered) for i in image_ids], obs_point3D=obs,
                num_reg_trials=[int((trials or {}).get(i, 0)) for i in image_ids], filtered=[int(i in filtered) for i in image_ids])


def identity(n):
    return [(k, k) for k in range(n)]


def star(b, cam, center_id, n_center, leaves, rng):
    """A registered image `center_id` with n_center points2D, all with a point; leaf images {id: n} matched to it one to one."""
    b.image(center_id, cam, rng.uniform([0, 0], [W, H], (n_center, 2)))
    for i, n in leaves.items():
        b.image(i, cam, rng.uniform([0, 0], [W, H], (n, 2)))
        b.pair(center_id, i, identity(min(n, n_center)))
    return {(center_id, f): f for f in range(n_center)}


def word_edges():
    """Images of 0, 1, 31, 32, 33, 63, 64, 65 and 257 points2D: the bitmap's word edges, the lane loop's edges."""
    rng, b = np.random.default_rng(1), Builder()
    cam = b.camera()
    sizes = [0, 1, 31, 32, 33, 63, 64, 65, 257]
    pts = star(b, cam, 100, 257, {k + 1: n for k, n in enumerate(sizes)}, rng)
    ids = [100] + list(range(1, len(sizes) + 1))
    return b.scene(), [problem(b, ids, {100}, pts)], dict(abs_pose_min_num_inliers=1)


def cell_borders():
    """Points exactly on cell borders (x = width k / 64), at the width, beyond it, and a camera that is not square."""
    rng, b = np.random.default_rng(2), Builder()
    cam = b.camera(1000, 333)
    xs = [1000 * k / 64 for k in range(64)] + [1000.0, 1000.5, 5000.0, 1e300, np.nextafter(1000 * 17 / 64, 0), 0.0]
    ys = [333 * k / 64 for k in range(64)] + [333.0, 333.5, 1e300, 700.0, np.nextafter(333 * 17 / 64, 0), 0.0]
    xy = np.stack([xs, ys], 1)
    b.image(100, cam, rng.uniform([0, 0], [1000, 333], (len(xy), 2)))
    b.image(1, cam, xy)
    b.image(2, cam, xy[::-1])
    b.pair(100, 1, identity(len(xy)))
    b.pair(2, 100, identity(len(xy)))
    pts = {(100, f): f for f in range(len(xy))}
    return b.scene(), [problem(b, [100, 1, 2], {100}, pts)], dict(abs_pose_min_num_inliers=1)


def full_and_single():
    """Every finest cell of one image occupied (the maximum score 17 895 696), exactly one cell of another."""
    rng, b = np.random.default_rng(3), Builder()
    cam = b.camera()
    gx, gy = np.meshgrid((np.arange(64) + 0.5) * W / 64, (np.arange(64) + 0.5) * H / 64)
    full = np.stack([gx.ravel(), gy.ravel()], 1)
    b.image(100, cam, rng.uniform([0, 0], [W, H], (4096, 2)))
    b.image(1, cam, full)
    b.image(2, cam, np.tile([[W / 2 + 1, H / 2 + 1]], (40, 1)))
    b.pair(100, 1, identity(4096))
    b.pair(100, 2, identity(40))
    pts = {(100, f): f for f in range(4096)}
    return b.scene(), [problem(b, [100, 1, 2], {100}, pts)], dict(abs_pose_min_num_inliers=30)


def duplicates():
    """Matches dropped by the duplicate rule: the survivor decides visibility.  Pair (100, 1): (0, 0) kept, (0, 1) and (1, 0)
    dropped; point2D 0 of image 100 has a point, point2D 1 has none -- so point2D 0 of image 1 is visible through the survivor
    and point2D 1 is not, although a dropped match would have reached a point.  Pair (1, 101), written from the candidate:
    (2, 5) kept, (3, 5) dropped, and only then would point2D 3 have been visible."""
    rng, b = np.random.default_rng(4), Builder()
    cam = b.camera()
    for i in (100, 101, 1):
        b.image(i, cam, rng.uniform([0, 0], [W, H], (8, 2)))
    b.pair(100, 1, [(0, 0), (0, 1), (1, 0), (2, 4)])
    b.pair(1, 101, [(2, 5), (3, 5), (6, 6)])
    pts = {(100, 0): 0, (100, 2): 1, (101, 5): 2}
    return b.scene(), [problem(b, [100, 101, 1], {100, 101}, pts)], dict(abs_pose_min_num_inliers=1)


def no_point_correspondences():
    """A point2D whose correspondences all end on observations without a point: observed, not visible."""
    rng, b = np.random.default_rng(5), Builder()
    cam = b.camera()
    for i in (100, 101, 1, 2):
        b.image(i, cam, rng.uniform([0, 0], [W, H], (6, 2)))
    b.pair(100, 1, identity(6))
    b.pair(101, 1, identity(6))
    b.pair(1, 2, identity(6))  # a correspondence between two candidates: it never makes a point2D visible
    pts = {(100, 0): 0, (101, 0): 0, (100, 1): 1, (101, 2): 2}
    return b.scene(), [problem(b, [100, 101, 1, 2], {100, 101}, pts)], dict(abs_pose_min_num_inliers=1)


def shared_images():
    """Two problems that share images but differ in state, and one that sees fewer pairs."""
    rng, b = np.random.default_rng(6), Builder()
    cam = b.camera()
    for i in (10, 11, 12, 13):
        b.image(i, cam, rng.uniform([0, 0], [W, H], (20, 2)))
    for a, c in ((10, 11), (11, 12), (12, 13), (10, 13), (10, 12)):
        b.pair(a, c, [(k, (k + a) % 20) for k in range(0, 20, 1 + (a + c) % 3)])
    p1 = problem(b, [10, 11, 12, 13], {10}, {(10, f): f for f in range(0, 20, 2)})
    p2 = problem(b, [13, 12, 11, 10], {12, 13}, {(12, f): f for f in range(5, 15)} | {(13, f): 20 + f for f in range(3)})
    p3 = problem(b, [11, 10, 12], {11}, {(11, f): f for f in range(20)})
    return b.scene(), [p1, p2, p3], dict(abs_pose_min_num_inliers=1)


def ranks():
    """Equal ranks (id order), both buckets, and counts that order differently under the three methods: the candidates see
    10, 10, 10, 12 and 6 visible points2D with 10, 20, 10, 40 and 6 observations; image 5's few points are spread out, image
    4's many sit in one cell."""
    rng, b = np.random.default_rng(7), Builder()
    cam = b.camera()
    b.image(100, cam, rng.uniform([0, 0], [W, H], (48, 2)))
    b.image(101, cam, rng.uniform([0, 0], [W, H], (48, 2)))
    pts = {(100, f): f for f in range(48)}  # image 101 is registered and has no points: observed through it, never visible
    spread = np.stack([(np.arange(40) % 8 + 0.5) * W / 8, (np.arange(40) // 8 + 0.5) * H / 8], 1)
    same = np.tile([[10.0, 10.0]], (40, 1))
    specs = {1: (spread, 10, 10), 2: (spread, 10, 20), 3: (spread, 10, 10), 4: (same, 12, 40), 5: (spread[::-1] * 0.99, 6, 6), 6: (spread, 10, 10),
             7: (spread, 10, 10)}
    for i, (xy, nvis, nobs) in specs.items():
        b.image(i, cam, xy)
        b.pair(100, i, identity(nvis))
        if nobs > nvis:
            b.pair(i, 101, [(k, k) for k in range(nvis, nobs)])
    ids = [7, 100, 3, 2, 1, 101, 4, 5, 6]
    pr = problem(b, ids, {100, 101}, pts, trials={6: 1, 2: 0}, filtered={7})
    return b.scene(), [pr], dict(abs_pose_min_num_inliers=6)


def boundaries():
    """num_visible equal to abs_pose_min_num_inliers and one below; num_reg_trials equal to max_reg_trials and one below."""
    rng, b = np.random.default_rng(8), Builder()
    cam = b.camera()
    pts = star(b, cam, 100, 40, {1: 30, 2: 29, 3: 35, 4: 35, 5: 31}, rng)
    pr = problem(b, [100, 1, 2, 3, 4, 5], {100}, pts, trials={3: 3, 4: 2})
    return b.scene(), [pr], dict(abs_pose_min_num_inliers=30, max_reg_trials=3)


def nothing_eligible():
    """A problem with nothing eligible beside one with something, an empty problem, and a problem without pairs."""
    rng, b = np.random.default_rng(9), Builder()
    cam = b.camera()
    pts = star(b, cam, 100, 12, {1: 12, 2: 12}, rng)
    b.image(50, cam, rng.uniform([0, 0], [W, H], (5, 2)))
    b.image(51, cam, np.zeros((0, 2)))
    none = problem(b, [100, 1, 2], {100}, pts, trials={1: 1, 2: 1})
    some = problem(b, [2, 100], {100}, pts)
    all_registered = problem(b, [100, 1], {100, 1}, pts)
    lonely = problem(b, [50, 51], set(), {})
    empty = problem(b, [], set(), {})
    return b.scene(), [none, some, empty, all_registered, lonely], dict(abs_pose_min_num_inliers=12, max_reg_trials=1)


def many_slots():
    """One problem of 300 slots: the placement's counting crosses a workgroup, and most keys tie but for the id."""
    rng, b = np.random.default_rng(10), Builder()
    cam = b.camera()
    reg = list(range(1000, 1010))
    for i in reg:
        b.image(i, cam, rng.uniform([0, 0], [W, H], (12, 2)))
    cand = [int(x) for x in rng.permutation(np.arange(1, 291))]
    pts = {(i, f): 12 * k + f for k, i in enumerate(reg) for f in range(12)}
    for i in cand:
        n = 4 + i % 5
        b.image(i, cam, rng.uniform([0, 0], [W, H], (n, 2)) if i % 7 else np.tile([[5.0, 5.0]], (n, 1)))
        r = reg[i % 10]
        if i % 2:
            b.pair(r, i, identity(n - i % 3))
        else:
            b.pair(i, r, identity(n - i % 3))
    ids = [int(x) for x in rng.permutation(np.array(reg + cand))]
    trials = {i: i % 4 for i in cand if i % 11 == 0}
    pr = problem(b, ids, set(reg), pts, trials=trials, filtered={i for i in cand if i % 13 == 0})
    return b.scene(), [pr], dict(abs_pose_min_num_inliers=3)


def random_case(seed, n_images=8, n_problems=3):
    """A random scene: a ring with chords, random match lists with repeated features, random registrations and points."""
    rng, b = np.random.default_rng(seed), Builder()
    cams = [b.camera(), b.camera(800, 300)]
    ids = [int(x) for x in rng.permutation(np.arange(1, n_images + 1) * 3)]
    for i in ids:
        b.image(i, cams[i % 2], rng.uniform([0, 0], [900, 500], (int(rng.integers(0, 40)), 2)))
    for a in range(n_images):
        for step in (1, 2, 3):
            i, j = ids[a], ids[(a + step) % n_images]
            if rng.random() < 0.2 or b.n(i) == 0 or b.n(j) == 0 or (j, i) in b.pairs or (i, j) in b.pairs:
                continue
            n = int(rng.integers(0, 30))
            b.pair(i, j, np.stack([rng.integers(0, b.n(i), n), rng.integers(0, b.n(j), n)], 1))
    problems = []
    for _ in range(n_problems):
        sub = [int(x) for x in rng.permutation(ids)[:int(rng.integers(2, n_images + 1))]]
        reg = {i for i in sub if rng.random() < 0.5}
        pts = {(i, f): int(rng.integers(0, 50)) for i in reg for f in range(b.n(i)) if rng.random() < 0.6}
        problems.append(problem(b, sub, reg, pts, trials={i: int(rng.integers(0, 4)) for i in sub if rng.random() < 0.3},
                                filtered={i for i in sub if rng.random() < 0.2}))
    return b.scene(), problems, dict(abs_pose_min_num_inliers=int(rng.integers(1, 4)), image_selection_method=int(rng.integers(0, 3)))


def _random(seed):
    return lambda: random_case(seed)


SCENES = {"word_edges": word_edges, "cell_borders": cell_borders, "full_and_single": full_and_single, "duplicates": duplicates,
          "no_point_correspondences": no_point_correspondences, "shared_images": shared_images, "ranks": ranks, "boundaries": boundaries,
          "nothing_eligible": nothing_eligible, "many_slots": many_slots, "random_1": _random(101), "random_2": _random(102),
          "random_3": _random(103)}
NAMES = list(SCENES)
METHODS = (0, 1, 2)
_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]


def permuted(scene, problems, seed):
    """The same scene with its problems and pairs in another order, and the matches of every pair without a repeated feature
    (so that the duplicate rule drops none) shuffled.  Returns (scene, problems, the problems' permutation)."""
    rng = np.random.default_rng(seed)
    s = dict(scene)
    pairs = np.asarray(scene["pairs"]).reshape(-1, 2)
    moff = np.asarray(scene["match_offsets"], np.int64)
    m = np.asarray(scene["matches"]).reshape(-1, 2)
    order = rng.permutation(len(pairs))
    lists = []
    for k in order:
        mk = m[moff[k]:moff[k + 1]]
        if len(mk) and len(set(mk[:, 0])) == len(mk) and len(set(mk[:, 1])) == len(mk):
            mk = mk[rng.permutation(len(mk))]
        lists.append(mk)
    s["pairs"] = pairs[order]
    s["match_offsets"] = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    s["matches"] = np.concatenate(lists + [np.zeros((0, 2), np.uint32)]).astype(np.uint32)
    perm = [int(x) for x in rng.permutation(len(problems))]
    return s, [problems[k] for k in perm], perm


# ================================================================== dsm_find_local_bundles
def lb_case(rng, centers, n_points, nfeat, seen, registered=None, ids=None, repeats=(), quat_scale=1.0):
    """One problem of FindLocalBundle.  centers: the images' projection centres (identity rotations up to a scale of the
    quaternion, and a small rotation for odd images); n_points points in front of them at depth about 10; seen[k]: the points
    image k observes (indices), placed on distinct points2D among nfeat[k]; repeats: (image index, point) observed once more."""
    n = len(centers)
    ids = list(ids) if ids is not None else [10 + 3 * k for k in range(n)]
    registered = [1] * n if registered is None else list(registered)
    xyz = rng.uniform([-1, -1, 9], [1, 1, 11], (n_points, 3))
    qvec, tvec, obs = [], [], []
    for k in range(n):
        a = 0.02 * (k % 3)  # a rotation about y by angle a: q = (cos a/2, 0, sin a/2, 0)
        q = np.array([np.cos(a / 2), 0.0, np.sin(a / 2), 0.0]) * (quat_scale if k % 2 else 1.0)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        qvec.append(q), tvec.append(-R @ np.asarray(centers[k], np.float64))
        o = np.full(nfeat[k], -1, np.int32)
        pts = list(seen[k]) + [p for kk, p in repeats if kk == k]
        where = rng.permutation(nfeat[k])[:len(pts)]
        o[np.sort(where)] = pts
        obs.append(o)
    return dict(image_ids=ids, registered=registered, obs_point3D=obs, qvec=np.array(qvec), tvec=np.array(tvec), point_xyz=xyz), nfeat


def lb_scene(problems_and_nfeat):
    """The scene arrays find_local_bundles reads (image ids and point2D counts) for problems on disjoint or shared images."""
    count = {}
    for pr, nfeat in problems_and_nfeat:
        for i, n in zip(pr["image_ids"], nfeat):
            assert count.setdefault(i, n) == n
    ids = sorted(count)[::-1]
    off = np.concatenate([[0], np.cumsum([count[i] for i in ids])]).astype(np.uint32)
    return dict(image_ids=np.array(ids, np.uint32), points2D_offsets=off), [pr for pr, _ in problems_and_nfeat]


def baseline(deg):
    return 10.0 * np.tan(np.radians(deg))


def lb_copy_and_chain():
    """Five overlapping images (the copy path at the default of six) and one more (the chain), on the same images."""
    rng = np.random.default_rng(21)
    c6 = [[0, 0, 0]] + [[baseline(d), 0, 0] for d in (7, 5, 3, 2, 1)]
    c7 = c6 + [[baseline(8), 0.1, 0]]
    a = lb_case(rng, c6, 30, [40] * 6, [range(30)] + [range(0, 30 - 2 * k) for k in range(5)])
    b = lb_case(rng, c7, 30, [40] * 7, [range(30)] + [range(0, 30 - 2 * k) for k in range(6)])
    s, problems = lb_scene([a, b])
    return s, problems, [(0, 10), (1, 10), (1, 13)], {}


def lb_thresholds():
    """Images accepted at the first, the second, the fifth and the eighth threshold, and by the fill-up only: angles of about
    7, 5, 2.2, 1.1, 0.5 and 0.3 degrees and full overlap, and an image of a large angle below the loosest overlap threshold."""
    rng = np.random.default_rng(22)
    degs = (0.3, 2.2, 7, 0.5, 1.1, 5)
    c = [[0, 0, 0]] + [[baseline(d), 0, 0] for d in degs] + [[baseline(20), 0, 0]]
    seen = [range(40)] + [range(40)] * 6 + [range(3)]
    pr = lb_case(rng, c, 40, [64] * 8, seen)
    s, problems = lb_scene([pr])
    return s, problems, [(0, 10)], {}


def lb_overlap_edge():
    """A shared count exactly equal to 0.6 NumPoints3D (12 of 20: taken at the first threshold) and one below (11: not before
    the third), which changes the order of the bundle."""
    rng = np.random.default_rng(23)
    c = [[0, 0, 0], [baseline(3.5), 0, 0], [baseline(7), 0, 0], [baseline(8), 0, 0], [baseline(9), 0, 0]]
    a = lb_case(rng, c, 20, [25] * 5, [range(20), range(14), range(12), range(2), range(1)])
    b = lb_case(rng, c, 20, [25] * 5, [range(20), range(14), range(11), range(2), range(1)], ids=[40, 43, 46, 49, 52])
    s, problems = lb_scene([a, b])
    return s, problems, [(0, 10), (1, 40)], dict(local_ba_num_images=3)


def lb_sizes():
    """NumPoints3D of 1, 2, 3, 4, 64, 65 and 257: Percentile's index 0, its rounding at .5 (n = 3: 0.75 * 2 = 1.5 -> 2), the
    lane loop's edges.  Four other images each, three wanted."""
    rng = np.random.default_rng(24)
    cases = []
    for j, n in enumerate((1, 2, 3, 4, 64, 65, 257)):
        c = [[0, 0, 0]] + [[baseline(d), 0.01 * j, 0] for d in (6.5, 4.5, 2.5, 0.7)]
        cases.append(lb_case(rng, c, n, [n + 3] * 5, [range(n)] * 5, ids=[100 * (j + 1) + k for k in range(5)]))
    s, problems = lb_scene(cases)
    return s, problems, [(j, 100 * (j + 1)) for j in range(7)], dict(local_ba_num_images=4)


def lb_degenerate():
    """A point referenced by two points2D of the query (counted twice, its angle twice in the list); two track elements on the
    same other image; a candidate whose centre equals the query's (angle 0); a point at the query's centre and one at a
    candidate's (zero denominator: angle 0); an unregistered image in the problem; a quaternion that is not normalised."""
    rng = np.random.default_rng(25)
    c = [[0.5, 0.25, 0.125], [0.5, 0.25, 0.125], [baseline(6.5) + 0.5, 0.25, 0.125], [baseline(3) + 0.5, 0.25, 0.125], [3.0, 0, 0], [4.0, 0, 0]]
    seen = [range(12), range(12), range(12), range(10), range(9), []]
    pr, nfeat = lb_case(rng, c, 12, [20] * 6, seen, registered=[1, 1, 1, 1, 1, 0], repeats=[(0, 3), (0, 3), (2, 5), (3, 0)], quat_scale=2.5)
    pr["point_xyz"][0] = c[0]            # a point at the query's centre
    pr["point_xyz"][1] = c[2]            # ... and at a candidate's
    pr["qvec"][0] = [1.0, 0.0, 0.0, 0.0]  # the query and its twin share the centre exactly: identity rotations
    pr["qvec"][1] = [4.0, 0.0, 0.0, 0.0]
    pr["tvec"][0] = pr["tvec"][1] = [-0.5, -0.25, -0.125]
    s, problems = lb_scene([(pr, nfeat)])
    return s, problems, [(0, 10), (0, 16), (0, 13)], dict(local_ba_num_images=3)


def lb_options():
    """local_ba_num_images = 2 and local_ba_min_tri_angle = 0 on the threshold scene."""
    s, problems, queries, _ = lb_thresholds()
    return s, problems, queries, dict(local_ba_num_images=2, local_ba_min_tri_angle=0.0)


def lb_zero_angle():
    s, problems, queries, _ = lb_thresholds()
    return s, problems, queries, dict(local_ba_min_tri_angle=0.0)


def lb_queries():
    """Several queries on one problem, the same image queried in two problems, a query without points and one without overlap."""
    rng = np.random.default_rng(26)
    n = 9
    c = [[baseline(1.3) * k, 0.05 * (k % 2), 0] for k in range(n)]
    seen = [sorted(rng.permutation(50)[:int(rng.integers(15, 45))]) for _ in range(n)]
    a = lb_case(rng, c, 50, [60] * n, seen)
    seen_b = [sorted(rng.permutation(30)[:int(rng.integers(5, 30))]) for _ in range(n - 2)] + [[], [29]]
    seen_b = [[p for p in x if p != 29] for x in seen_b[:-1]] + [[29]]
    b = lb_case(rng, c[::-1], 30, [60] * n, seen_b, ids=[10 + 3 * k for k in range(n)][::-1])
    s, problems = lb_scene([a, b])
    return s, problems, [(0, 10), (0, 13), (1, 10), (0, 34), (1, 34), (1, 31), (1, 16), (0, 22)], dict(local_ba_num_images=5)


def lb_random(seed):
    def build():
        rng = np.random.default_rng(seed)
        cases, queries = [], []
        for j in range(3):
            n = int(rng.integers(2, 12))
            c = rng.uniform([-2, -0.3, -0.3], [2, 0.3, 0.3], (n, 3))
            npts = int(rng.integers(1, 80))
            reg = [1] + [int(rng.random() < 0.8) for _ in range(n - 1)]
            seen = [sorted(rng.permutation(npts)[:int(rng.integers(0, npts + 1))]) if reg[k] else [] for k in range(n)]
            ids = [1000 * j + int(x) for x in rng.permutation(np.arange(1, 50))[:n]]
            cases.append(lb_case(rng, c, npts, [npts + 5] * n, seen, registered=reg, ids=ids, quat_scale=0.5))
            queries += [(j, ids[k]) for k in range(n) if reg[k] and rng.random() < 0.7]
        s, problems = lb_scene(cases)
        return s, problems, queries, dict(local_ba_num_images=int(rng.integers(2, 7)), local_ba_min_tri_angle=float(rng.choice([6.0, 3.0, 12.0])))
    return build


LB_SCENES = {"copy_and_chain": lb_copy_and_chain, "thresholds": lb_thresholds, "overlap_edge": lb_overlap_edge, "sizes": lb_sizes,
             "degenerate": lb_degenerate, "options": lb_options, "zero_angle": lb_zero_angle, "queries": lb_queries, "random_1": lb_random(301),
             "random_2": lb_random(302), "random_3": lb_random(303)}
LB_NAMES = list(LB_SCENES)
_lb_cache = {}


def lb_get(name):
    if name not in _lb_cache:
        _lb_cache[name] = LB_SCENES[name]()
    return _lb_cache[name]


def lb_permuted(problems, queries, seed):
    """The same problems in another order with every problem's points renumbered, and the queries in another order.  Returns
    (problems, queries, the queries' permutation)."""
    rng = np.random.default_rng(seed)
    perm = [int(x) for x in rng.permutation(len(problems))]
    new_index = {old: new for new, old in enumerate(perm)}
    out = []
    for old in perm:
        pr = dict(problems[old])
        m = len(pr["point_xyz"])
        renumber = rng.permutation(m)  # old point -> new point
        xyz = np.zeros((m, 3))
        xyz[renumber] = pr["point_xyz"]
        pr["point_xyz"] = xyz
        pr["obs_point3D"] = [np.where(o >= 0, renumber[np.maximum(o, 0)] if m else o, -1).astype(np.int32) for o in pr["obs_point3D"]]
        out.append(pr)
    qperm = [int(x) for x in rng.permutation(len(queries))]
    return out, [(new_index[queries[k][0]], queries[k][1]) for k in qperm], qperm
