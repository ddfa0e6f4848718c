"""Small scenes for dsm_find_initial_pairs: 2 to 10 images, 40 to 300 correspondences per pair, and
init_min_num_inliers lowered to 30 so that the shapes stay tiny.  Every scene is a function of nothing: the same bytes on every
machine (numpy's default_rng with a fixed seed).  SCENES maps a name to a builder returning (scene, problems, options): the scene
dict of Context.find_initial_pairs, a list of problem dicts, and the keywords of default_initial_pair_options.  The GPU tests and
the CPU test of the margins walk the same table."""
import math

import numpy as np

from dagsfm_amd import capi

W, H, F = 1000, 750, 800.0
MIN_INLIERS = 30


def pinhole(prior=True):
    return capi.simple_pinhole(F, W / 2, H / 2, W, H, prior)


def look_at(center, target=(0.0, 0.0, 0.0), roll=0.0):
    """World -> camera rotation (rows x, y, z) of a camera at `center` looking at `target`, and t = -R c."""
    c = np.asarray(center, float)
    z = np.asarray(target, float) - c
    z /= np.linalg.norm(z)
    up = np.array([0.0, 1.0, 0.0]) if abs(z[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    cr, sr = math.cos(roll), math.sin(roll)
    R = np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]) @ R
    return R, -R @ c


def project(cam, u, v):
    """Camera::WorldToImage for the models the scenes use: 0 SIMPLE_PINHOLE, 4 OPENCV, 5 OPENCV_FISHEYE (k1..k4 = 0)."""
    p = cam.params
    if cam.model_id == 0:
        return np.array([p[0] * u + p[1], p[0] * v + p[2]])
    if cam.model_id == 4:
        k1, k2, p1, p2 = p[4], p[5], p[6], p[7]
        r2 = u * u + v * v
        rad = k1 * r2 + k2 * r2 * r2
        du = u * rad + 2 * p1 * u * v + p2 * (r2 + 2 * u * u)
        dv = v * rad + 2 * p2 * u * v + p1 * (r2 + 2 * v * v)
        return np.array([p[0] * (u + du) + p[2], p[1] * (v + dv) + p[3]])
    if cam.model_id == 5:
        r = math.sqrt(u * u + v * v)
        s = math.atan(r) / r if r > 1e-12 else 1.0
        return np.array([p[0] * s * u + p[2], p[1] * s * v + p[3]])
    raise ValueError(cam.model_id)


class Builder:
    """Images see subsets of a point cloud; a pair's matches are the points both images see, a share of them mismatched."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.cams, self.img_cam, self.poses, self.obs = [], [], [], []
        self.pairs, self.moff, self.matches = [], [0], []

    def camera(self, cam):
        self.cams.append(cam)
        return len(self.cams) - 1

    def image(self, R, t, X, point_ids, cam=0, noise=0.3):
        """An image observing the points X[point_ids] (feature order shuffled); returns its index."""
        order = [int(p) for p in self.rng.permutation(point_ids)]
        xy = []
        for p in order:
            Xc = R @ X[p] + t
            xy.append(project(self.cams[cam], Xc[0] / Xc[2], Xc[1] / Xc[2]) + self.rng.normal(0, noise, 2))
        self.poses.append((R, t))
        self.img_cam.append(cam)
        self.obs.append((order, np.array(xy).reshape(-1, 2)))
        return len(self.obs) - 1

    def raw_image(self, xy, cam=0):
        """An image of given pixel positions; feature k is 'point' k."""
        self.poses.append(None)
        self.img_cam.append(cam)
        self.obs.append((list(range(len(xy))), np.asarray(xy, float).reshape(-1, 2)))
        return len(self.obs) - 1

    def pair(self, i, j, limit=None, wrong=0.0, extra=()):
        """The matches of images i, j over their common points, in ascending feature index of i (at most `limit`); a share
        `wrong` is redirected to another free feature of j; `extra` (idx1, idx2) matches are appended as they are."""
        idx_j = {p: k for k, p in enumerate(self.obs[j][0])}
        m = [(a, idx_j[p]) for a, p in enumerate(self.obs[i][0]) if p in idx_j]
        if limit is not None:
            m = m[:limit]
        used = {b for _, b in m}
        free = [b for b in range(len(self.obs[j][0])) if b not in used]
        for k in range(len(m)):
            if free and self.rng.random() < wrong:
                m[k] = (m[k][0], free.pop(int(self.rng.integers(0, len(free)))))
        m += list(extra)
        self.pairs.append((i, j))
        self.matches += m
        self.moff.append(len(self.matches))
        return len(m)

    def scene(self, id_of=lambda i: 3 * i + 2):
        n = len(self.obs)
        offs = np.concatenate([[0], np.cumsum([len(o[0]) for o in self.obs])]).astype(np.uint32)
        xy = np.concatenate([o[1] for o in self.obs]) if n else np.zeros((0, 2))
        return dict(camera_ids=np.arange(len(self.cams), dtype=np.uint32) + 11, cameras=list(self.cams),
                    image_ids=np.array([id_of(i) for i in range(n)], np.uint32), image_camera_ids=np.array(self.img_cam, np.uint32) + 11,
                    points2D_offsets=offs, points2D_xy=xy,
                    pairs=np.array([(id_of(i), id_of(j)) for i, j in self.pairs], np.uint32).reshape(-1, 2),
                    match_offsets=np.array(self.moff, np.uint64), matches=np.array(self.matches, np.uint32).reshape(-1, 2))


def cloud(rng, n, extent=1.0, depth=1.0):
    return rng.uniform([-extent, -extent, -depth], [extent, extent, depth], (n, 3))


def ring_center(k, n, radius=6.0, arc=2 * math.pi):
    a = arc * k / n
    return [radius * math.sin(a), 0.3 * math.cos(3 * a), -radius * math.cos(a)]


OPTS = dict(init_min_num_inliers=MIN_INLIERS)


def ring(seed=1, n_images=6, n_points=120, cams=None, arc=math.pi):
    """Cameras on an arc around a cloud; neighbours share more points than distant images, so the first candidate is a pair of
    neighbours with a wide enough baseline."""
    b = Builder(seed)
    for c in cams or [pinhole()]:
        b.camera(c)
    X = cloud(b.rng, n_points)
    for k in range(n_images):
        R, t = look_at(ring_center(k, n_images, arc=arc), roll=0.05 * k)
        lo = int(k * 0.3 * n_points / (n_images - 1))
        b.image(R, t, X, range(lo, min(n_points, lo + int(n_points * 0.7))), cam=k % len(b.cams))
    for i in range(n_images):
        for j in range(i + 1, n_images):
            b.pair(i, j, wrong=0.1)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def forward_motion():
    """The best-ranked pair is a camera and the same camera moved along its optical axis: |tvec.z| = 1, rejected."""
    b = Builder(2)
    b.camera(pinhole())
    X = cloud(b.rng, 150, extent=1.2)
    R0, t0 = look_at([0, 0, -6.0])
    i0 = b.image(R0, t0, X, range(150))
    i1 = b.image(R0, -R0 @ np.array([0, 0, -4.5]), X, range(150))
    R2, t2 = look_at([3.0, 0.2, -5.2])
    i2 = b.image(R2, t2, X, range(20, 130))
    b.pair(i0, i1, wrong=0.05)
    b.pair(i0, i2, wrong=0.05)
    b.pair(i1, i2, limit=60, wrong=0.05)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def small_baseline():
    """The top pairs are a hub and five images a hair's breadth away from it (the angle test fails); the sixth candidate has
    a real baseline: success at the sixth candidate."""
    b = Builder(3)
    b.camera(pinhole())
    X = cloud(b.rng, 160, extent=1.2)
    R0, t0 = look_at([0, 0, -6.0])
    hub = b.image(R0, t0, X, range(160))
    near = []
    for k in range(5):
        R, t = look_at([0.12 * (k + 1), 0.05 * (k - 2), -6.0], roll=0.02 * k)
        near.append(b.image(R, t, X, range(160)))
    R, t = look_at([3.2, 0.3, -5.0])
    far = b.image(R, t, X, range(160))
    for k, im in enumerate(near):
        b.pair(hub, im, limit=150 - 12 * k, wrong=0.05)
    b.pair(far, hub, limit=70, wrong=0.05)  # written (far, hub): the candidate is (hub, far), its matches swapped
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def planar():
    """All points on one plane: PLANAR, the pose comes from H."""
    b = Builder(4)
    b.camera(pinhole())
    X = cloud(b.rng, 140, extent=1.5, depth=0.0)
    for c in ([-2.5, 0.4, -5.0], [2.5, -0.3, -5.5], [0.2, 2.0, -6.0]):
        R, t = look_at(c)
        b.image(R, t, X, range(140))
    b.pair(0, 1, wrong=0.05)
    b.pair(0, 2, limit=90, wrong=0.05)
    b.pair(1, 2, limit=80, wrong=0.05)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def pure_rotation():
    """Two images from one centre: PANORAMIC, tri_angle 0, rejected -- and nothing else to try: no pair found."""
    b = Builder(5)
    b.camera(pinhole())
    X = cloud(b.rng, 120, extent=1.0)
    R0, t0 = look_at([0, 0, -6.0])
    b.image(R0, t0, X, range(120), noise=0.0)
    R1, _ = look_at([0, 0, -6.0], target=(0.5, 0.1, 0.0), roll=0.1)
    b.image(R1, -R1 @ np.array([0, 0, -6.0]), X, range(120), noise=0.0)
    b.pair(0, 1)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def watermark():
    """A pair whose matches sit in the image border and differ by one pixel translation: WATERMARK, rejected by configuration;
    the next candidate is a real pair."""
    b = Builder(6)
    b.camera(pinhole())
    rng = b.rng
    n = 200
    side = rng.integers(0, 4, n)
    along = rng.uniform(0.02, 0.98, n)
    depth = rng.uniform(0.01, 0.07, n)
    x = np.where(side == 0, depth, np.where(side == 1, 1 - depth, along)) * W
    y = np.where(side == 2, depth, np.where(side == 3, 1 - depth, along)) * H
    # keep both copies inside the border after the shift
    xy = np.stack([x, y], 1)
    wa = b.raw_image(xy)
    wb = b.raw_image(xy + np.array([2.0, 1.5]))
    X = cloud(rng, 150, extent=1.2)
    R0, t0 = look_at([-2.5, 0.2, -5.0])
    R1, t1 = look_at([2.5, -0.2, -5.5])
    i0 = b.image(R0, t0, X, range(150))
    i1 = b.image(R1, t1, X, range(150))
    b.pair(wa, wb)
    b.pair(i0, i1, limit=120, wrong=0.05)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def nothing_found():
    """Four images a hair's breadth apart: every candidate fails the angle test; the tried list is the whole candidate list."""
    b = Builder(7)
    b.camera(pinhole())
    X = cloud(b.rng, 120, extent=1.2)
    for k in range(4):
        R, t = look_at([0.1 * k, 0.04 * k, -6.0], roll=0.03 * k)
        b.image(R, t, X, range(120))
    for i in range(4):
        for j in range(i + 1, 4):
            b.pair(i, j, limit=110 - 9 * (i + j), wrong=0.05)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def batching():
    """Three problems over overlapping subsets of a ring of ten images, one with a tried pair, one with a seed image, and an
    image registered elsewhere."""
    s, _, o = ring(seed=8, n_images=10, n_points=160, arc=1.5 * math.pi)
    ids = [int(x) for x in s["image_ids"]]
    problems = [dict(image_ids=ids[0:6], tried_pairs=[(ids[1], ids[0])]),
                dict(image_ids=ids[7:2:-1], num_registrations=[0, 1, 0, 0, 0], init_num_reg_trials=[0, 0, 2, 0, 1]),
                dict(image_ids=ids[4:10], seed_image2=ids[8])]
    return s, problems, o


def duplicates():
    """The pair with the most raw matches keeps 29 after the duplicate rule (its later matches repeat features): below the
    threshold of 30, so it is no candidate and its images rank by what they keep."""
    b = Builder(9)
    b.camera(pinhole())
    X = cloud(b.rng, 120, extent=1.2)
    centers = ([-2.5, 0.2, -5.0], [2.5, -0.2, -5.5], [0.0, 2.2, -5.5])
    for c in centers:
        R, t = look_at(c)
        b.image(R, t, X, range(120))
    # pair (0, 1): 29 clean matches by point, then 40 repeats of features already used
    idx1 = {p: k for k, p in enumerate(b.obs[1][0])}
    clean = [(a, idx1[p]) for a, p in enumerate(b.obs[0][0])][:29]
    repeats = [(clean[k % 29][0], (clean[(k + 7) % 29][1])) for k in range(40)]
    b.pairs.append((0, 1))
    b.matches += clean + repeats
    b.moff.append(len(b.matches))
    b.pair(0, 2, limit=60, wrong=0.05, extra=[(0, 0)] * 3)  # three repeats behind 60 kept ones
    b.pair(2, 1, limit=50, wrong=0.05)
    s = b.scene()
    return s, [dict(image_ids=list(s["image_ids"]))], dict(OPTS)


def camera_models():
    """The ring on an OPENCV and an OPENCV_FISHEYE camera, one of them without a prior focal length."""
    cams = [capi.camera(4, [800.0, 810.0, 500.0, 375.0, 0.02, -0.01, 0.001, 0.0005], W, H, prior=False),
            capi.camera(5, [800.0, 805.0, 500.0, 375.0, 0.0, 0.0, 0.0, 0.0], W, H, prior=True)]
    return ring(seed=10, n_images=6, n_points=120, cams=cams)


def triangulation_edge(n):
    """Two images given as the two seeds, exactly n correspondences: most well inside the gates, every seventh a far point
    whose angle is below the minimum, every eleventh a mismatch that triangulates behind a camera or anywhere."""
    def build():
        b = Builder(100 + n)
        b.camera(pinhole())
        rng = b.rng
        X = cloud(rng, n, extent=1.0)
        far = np.arange(n) % 7 == 3
        X[far] = X[far] * np.array([4.0, 4.0, 0.0]) + np.array([0.0, 0.0, 40.0 + 5.0 * rng.random()])
        R0, t0 = look_at([-2.2, 0.1, -5.0])
        R1, t1 = look_at([2.2, -0.1, -5.2])
        i0 = b.image(R0, t0, X, range(n))
        i1 = b.image(R1, t1, X, range(n))
        idx1 = {p: k for k, p in enumerate(b.obs[i1][0])}
        m = [(a, idx1[p]) for a, p in enumerate(b.obs[i0][0])]
        bad = [k for k in range(n) if k % 11 == 5]
        for k, k2 in zip(bad, bad[1:] + bad[:1]):  # rotate the second features of the mismatches: still one-to-one
            m[k] = (m[k][0], idx1[b.obs[i0][0][k2]])
        b.pairs.append((i0, i1))
        b.matches += m
        b.moff.append(len(b.matches))
        s = b.scene()
        ids = [int(x) for x in s["image_ids"]]
        return s, [dict(image_ids=ids, seed_image1=ids[1], seed_image2=ids[0])], dict(OPTS)
    return build


SCENES = {"ring": ring, "forward_motion": forward_motion, "small_baseline": small_baseline, "planar": planar,
          "pure_rotation": pure_rotation, "watermark": watermark, "nothing_found": nothing_found, "batching": batching,
          "duplicates": duplicates, "camera_models": camera_models}
for _n in (63, 64, 65, 257):
    SCENES["triangulation_%d" % _n] = triangulation_edge(_n)

_cache = {}


def get(name):
    """(scene, problems, option keywords) of a named scene, built once."""
    if name not in _cache:
        _cache[name] = SCENES[name]()
    return _cache[name]
