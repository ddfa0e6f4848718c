"""Synthetic scenes for the PatchMatch tests, built without any file: a band-limited random texture on a slanted plane, or on
two planes with a depth step, seen by 2-6 pinhole views.  Every pixel is the texture at the point where its viewing ray meets
the scene -- for a plane that is the plane-induced homography of the texture -- so the ground-truth depth and normal of every
pixel are known exactly."""
import numpy as np


def _texture(seed, n_waves=24, max_freq=2.5):
    """A sum of random plane waves with spatial frequencies up to max_freq cycles per world unit -> f(u, v) in [0, 1]."""
    rng = np.random.RandomState(seed)
    freq = rng.uniform(-max_freq, max_freq, size=(n_waves, 2))
    phase = rng.uniform(0, 2 * np.pi, size=n_waves)
    amp = rng.uniform(0.5, 1.0, size=n_waves)

    def f(u, v):
        acc = np.zeros_like(u, dtype=np.float64)
        for (fu, fv), p, a in zip(freq, phase, amp):
            acc += a * np.sin(2 * np.pi * (fu * u + fv * v) + p)
        acc /= 2.0 * np.sqrt((amp ** 2).sum() / 2.0)  # about +-2 sigma inside [-1, 1]
        return np.clip(0.5 + 0.5 * acc, 0.0, 1.0)
    return f


def make_scene(kind="slanted", width=48, height=40, n_views=4, seed=0, sizes=None, focal=None, baseline=0.15, depth=4.0):
    """kind: "slanted" (one plane) or "step" (a nearer plane over the world's x < 0 in front of a farther one).
    sizes: per-view (width, height), default all (width, height).  View 0 looks straight at the scene; the others sit on a
    ring of radius `baseline` around it and turn towards the scene centre.
    Returns (images, truth): images a list of dicts data [h][w] uint8, K [9], R [9], T [3] float32 (x_cam = R x_world + T);
    truth a list of dicts depth [h][w], normal [3][h][w] float64 in each camera's frame (normal towards the camera)."""
    tex = _texture(seed)
    sizes = sizes or [(width, height)] * n_views
    if kind == "slanted":
        planes = [(np.array([0.35, -0.2, -1.0]), depth, None)]
    elif kind == "step":
        planes = [(np.array([0.1, 0.05, -1.0]), 0.8 * depth, "left"), (np.array([-0.15, 0.1, -1.0]), 1.15 * depth, None)]
    else:
        raise ValueError(kind)
    planes = [(n / np.linalg.norm(n), d, where) for n, d, where in planes]  # n . X = -d: the plane through (0, 0, d) for n = (0, 0, -1)
    images, truth = [], []
    for v, (w, h) in enumerate(sizes):
        f = focal or 1.1 * max(w, h)
        K = np.array([[f, 0, (w - 1) / 2.0 + 0.3], [0, f, (h - 1) / 2.0 - 0.2], [0, 0, 1]])
        if v == 0:
            C, R = np.zeros(3), np.eye(3)
        else:
            ang = 2 * np.pi * (v - 1) / max(n_views - 1, 1) + 0.4
            C = np.array([baseline * depth * np.cos(ang), baseline * depth * np.sin(ang), 0.05 * depth * (v % 2)])
            z = np.array([0.0, 0.0, depth]) - C  # look at the scene centre, a few degrees of roll on top
            z /= np.linalg.norm(z)
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.linalg.norm(x)
            roll = 0.05 * v
            Rz = np.array([[np.cos(roll), -np.sin(roll), 0], [np.sin(roll), np.cos(roll), 0], [0, 0, 1]])
            R = Rz @ np.stack([x, np.cross(z, x), z])
        T = -R @ C
        ys, xs = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
        rays_cam = np.stack([(xs - K[0, 2]) / K[0, 0], (ys - K[1, 2]) / K[1, 1], np.ones_like(xs)], axis=-1)
        rays = rays_cam @ R  # R^T applied to every ray: world directions
        best_t = np.full((h, w), np.inf)
        best_n = np.zeros((h, w, 3))
        colour = np.zeros((h, w))
        for k, (n, d, where) in enumerate(planes):
            t = (-d - C @ n) / (rays @ n)
            X = C + rays * t[..., None]
            ok = (t > 0) & (t < best_t)
            if where == "left":
                ok &= X[..., 0] < 0
            e1 = np.cross(n, [0.0, 1.0, 0.0])
            e1 /= np.linalg.norm(e1)
            e2 = np.cross(n, e1)
            c = tex(X @ e1 + 3.7 * k, X @ e2 - 1.3 * k)
            best_t = np.where(ok, t, best_t)
            best_n = np.where(ok[..., None], n, best_n)
            colour = np.where(ok, c, colour)
        images.append({"data": np.round(255.0 * colour).astype(np.uint8), "K": K.reshape(9).astype(np.float32),
                       "R": R.reshape(9).astype(np.float32), "T": T.astype(np.float32)})
        normal_cam = best_n @ R.T
        flip = (normal_cam * rays_cam).sum(axis=-1) > 0
        normal_cam = np.where(flip[..., None], -normal_cam, normal_cam)
        truth.append({"depth": best_t.copy(), "normal": np.moveaxis(normal_cam, -1, 0).copy()})  # rays_cam has z = 1: t is the depth
    return images, truth
