"""The fixture models of the source selection tests and their references by tests/source_selection_ref.py,
computed once per process and shared by test_source_selection_cpu.py and test_source_selection_gpu.py.

A model is a dict R [n][9], T [n][3], xyz [m][3] (float32) and tracks (a list of index lists).  cases() lists every
(name, model name, keyword arguments) the tests run; reference(name) is the restatement's result for it."""
import functools

import numpy as np

from tests import source_selection_ref as ref

f32 = np.float32
IDENTITY = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def _model(R, T, xyz, tracks):
    return {"R": np.asarray(R, dtype=f32).reshape(-1, 9), "T": np.asarray(T, dtype=f32).reshape(-1, 3),
            "xyz": np.asarray(xyz, dtype=f32).reshape(-1, 3), "tracks": [[int(i) for i in t] for t in tracks]}


def _cameras(rng, n, radius=6.0):
    """n cameras on a shell of `radius` around the origin that look at it, with random roll: R, T with T = -R C."""
    Rs, Ts = [], []
    for _ in range(n):
        c = rng.normal(size=3)
        c *= radius * rng.uniform(0.8, 1.2) / np.linalg.norm(c)
        z = -c / np.linalg.norm(c)
        x = np.cross(z, rng.normal(size=3))
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        Rs.append(R.reshape(9))
        Ts.append(-R @ c)
    return Rs, Ts


def model_tracks():
    """Track lengths 0, 1, 2, 3, 63, 64, 65, 257 and 363 (images repeat in the long ones), one image three times in a track, a
    track of one image repeated, points after and between empty tracks."""
    rng = np.random.default_rng(2801)
    n = 48
    R, T = _cameras(rng, n)
    tracks = [[], [5], [], [7, 9], [1, 2, 3]]
    for L in (63, 64, 65, 257, 363):
        tracks.append(rng.integers(0, n, L).tolist())
    tracks += [[], [], [4, 11, 4, 20, 4], [6, 6, 6, 6], [], [0, 47]]
    xyz = rng.uniform(-1.5, 1.5, (len(tracks), 3))
    return _model(R, T, xyz, tracks)


PAIR_COUNTS = (1, 2, 3, 4, 5, 64, 65, 257)


def model_pairs():
    """Pairs (2 k, 2 k + 1) with 1, 2, 3, 4, 5 (the four residues of the percentile index), 64, 65 and 257 items."""
    rng = np.random.default_rng(2802)
    R, T = _cameras(rng, 2 * len(PAIR_COUNTS))
    tracks = []
    for k, c in enumerate(PAIR_COUNTS):
        tracks += [[2 * k, 2 * k + 1]] * c
    xyz = rng.uniform(-2.0, 2.0, (len(tracks), 3))
    return _model(R, T, xyz, tracks)


DEPTH_COUNTS = (1, 99, 100, 101, 200)


def model_images():
    """Image 0 is in no track; image 1 has depths <= 0 only, one of them exactly 0; images 2 .. 6 have 1, 99, 100, 101 and 200
    kept depths (and a few that are not kept).  Identity rotations: the depth is z + T[2]."""
    rng = np.random.default_rng(2803)
    n = 2 + len(DEPTH_COUNTS) + 2
    R = [IDENTITY] * n
    T = [[0.0, 0.0, 0.0], [0.0, 0.0, -2.0]] + [[0.1 * k, -0.2 * k, 0.5 * k] for k in range(len(DEPTH_COUNTS))] + [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.5]]
    xyz, tracks = [[0.3, 0.1, 2.0], [0.2, 0.4, 1.0], [0.0, 0.0, -3.0]], [[1], [1], [1]]
    for k, c in enumerate(DEPTH_COUNTS):
        for z in rng.uniform(0.5, 40.0, c):
            xyz.append([rng.uniform(-1, 1), rng.uniform(-1, 1), z])
            tracks.append([2 + k])
        for z in (-1.0, -0.5 * k):  # not kept: z + T[2] = z + 0.5 k <= 0
            xyz.append([0.0, 0.0, z - 0.5 * k])
            tracks.append([2 + k])
    # two points seen by the last two images, so that the model has items as well
    xyz += [[0.5, 0.5, 7.0], [-0.5, 0.25, 9.0]]
    tracks += [[n - 2, n - 1], [n - 1, n - 2]]
    m = _model(R, T, xyz, tracks)
    assert float(ref.depth(m["R"][1], m["T"][1], m["xyz"][0])) == 0.0
    return m


def model_geometry():
    """An obtuse ray angle (the pi - a branch), a point at a projection centre (denominator 0), two images with one centre."""
    R = [IDENTITY] * 4
    C = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 3.0, 1.0]]
    T = [[-c[0], -c[1], -c[2]] for c in C]
    xyz = [[1.0, 0.25, 0.0],  # between centres 0 and 1: the rays enclose more than 90 degrees
           [2.0, 0.0, 0.0],   # at the centre of images 1 and 2
           [0.5, 0.75, 4.0], [0.25, -0.5, 5.0], [1.5, 1.0, 3.0]]
    tracks = [[0, 1, 3], [0, 1, 2, 3], [0, 1, 2, 3], [3, 2, 1, 0], [2, 1]]
    return _model(R, T, xyz, tracks)


def model_collinear():
    """A point exactly on the line through two centres (X = -2 C1 with C0 = 0), found by search: the quotient of
    CalculateTriangulationAngle rounds to 1 + 2^-52 and the item's angle is NaN (the ruling of DESIGN.md 28).  A second pair with
    ordinary points next to it, and a pair whose only item is that NaN."""
    c1 = [float.fromhex("0x1.d8d3d4p-3"), float.fromhex("0x1.7b5c0ep-1"), float.fromhex("0x1.597438p-1")]
    R = [IDENTITY] * 4
    C = [[0.0, 0.0, 0.0], c1, [1.0, -2.0, 0.5], [0.0, 0.0, 0.0]]
    T = [[-c[0], -c[1], -c[2]] for c in C]
    X = [-2.0 * v for v in c1]
    xyz = [X, [0.5, 0.5, 3.0], [0.25, 1.0, 4.0], [1.0, 0.0, 5.0], X]
    tracks = [[0, 1], [0, 1, 2], [0, 1, 2], [1, 0], [3, 1]]
    return _model(R, T, xyz, tracks)


def model_gate():
    """Image 0 shares 3 points with image 4 and 2 points with each of the images 1, 2 and 3 (equal counts: ascending index)."""
    rng = np.random.default_rng(2806)
    R, T = _cameras(rng, 6)
    tracks = [[0, 4]] * 3 + [[0, 3]] * 2 + [[0, 1]] * 2 + [[2, 0]] * 2 + [[5, 4]]
    xyz = rng.uniform(-1.5, 1.5, (len(tracks), 3))
    return _model(R, T, xyz, tracks)


def model_scene():
    """A moderate scene of dagsfm_amd/synthetic.py: 240 images, the point pool of the scene, every track cut from the images
    that see the point (it projects inside the frame, in front of the camera) down to 2 .. 8 of them."""
    from dagsfm_amd import synthetic
    scene = synthetic.Scene(240, 64, seed=28, n_pool=6000)
    rng = np.random.default_rng(2807)
    poses = [scene.pose(i) for i in range(scene.n_images)]
    R = np.stack([p[0] for p in poses])
    t = np.stack([p[1] for p in poses])
    pc = np.einsum("irc,pc->ipr", R, scene.points) + t[:, None, :]  # [image][point][3]
    u = scene.focal * pc[..., 0] / pc[..., 2] + scene.width / 2.0
    v = scene.focal * pc[..., 1] / pc[..., 2] + scene.height / 2.0
    seen = (pc[..., 2] > 0) & (u >= 0) & (u < scene.width) & (v >= 0) & (v < scene.height)
    tracks = []
    for p in range(len(scene.points)):
        ids = np.nonzero(seen[:, p])[0]
        keep = min(len(ids), int(rng.integers(2, 9)))
        tracks.append(rng.choice(ids, size=keep, replace=False).tolist() if keep >= 2 else [])
    return _model(R.reshape(-1, 9), t, scene.points, tracks)


MODELS = {"tracks": model_tracks, "pairs": model_pairs, "images": model_images, "geometry": model_geometry, "collinear": model_collinear,
          "gate": model_gate, "scene": model_scene}
NAN_MODELS = ("collinear",)  # every other fixture has nan_items == 0 in the restatement


@functools.lru_cache(maxsize=None)
def model(name):
    return MODELS[name]()


@functools.lru_cache(maxsize=None)
def gate_thresholds():
    """(deg_equal, deg_above): min_triangulation_angle values whose float radians equal the angle of the gate model's pair (0, 4)
    exactly, and the next float above it.  Found by search on the CPU around angle / (pi / 180)."""
    a, b, _, angle = reference("gate")["pairs"]
    k = [i for i in range(len(a)) if (a[i], b[i]) == (0, 4)][0]
    target = f32(angle[k])
    out = []
    for want in (target, np.nextafter(target, f32(np.inf))):
        deg = float(want) / ref.DEG_TO_RAD
        for _ in range(64):
            if ref.min_angle_rad(deg) == want:
                break
            deg = float(np.nextafter(deg, np.inf if ref.min_angle_rad(deg) < want else -np.inf))
        assert ref.min_angle_rad(deg) == want
        out.append(deg)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases():
    """((name, model name, keyword arguments), ...)"""
    out = [("tracks", "tracks", {}), ("tracks_angle0", "tracks", {"min_triangulation_angle": 0.0, "max_num_src_images": 5})]
    for p in (0.0, 33.0, 50.0, 75.0, 100.0):
        out.append(("pairs_p%d" % p, "pairs", {"triangulation_angle_percentile": p, "min_triangulation_angle": 0.0}))
    out += [("images", "images", {}), ("geometry", "geometry", {"min_triangulation_angle": 0.0}), ("geometry_gated", "geometry", {}),
            ("collinear", "collinear", {"min_triangulation_angle": 0.0}), ("collinear_p100", "collinear", {"min_triangulation_angle": 0.0,
                                                                                                         "triangulation_angle_percentile": 100.0}),
            ("gate", "gate", {})]
    for m in (0, 1, 4, 7):  # none, one, exactly the candidates of image 0, more
        out.append(("gate_max%d" % m, "gate", {"max_num_src_images": m}))
    out.append(("gate_mask", "gate", {"candidate_mask": (1, 1, 1, 1, 0, 1)}))  # image 4, the otherwise-first neighbour of image 0, is out
    out.append(("scene", "scene", {}))
    out.append(("scene_mask", "scene", {"candidate_mask": tuple(int(i % 3 != 0) for i in range(240)), "max_num_src_images": 3}))
    return tuple(out)


def gate_cases():
    """The two threshold cases, which need the reference of "gate" first."""
    deg_equal, deg_above = gate_thresholds()
    return (("gate_equal", "gate", {"min_triangulation_angle": deg_equal}), ("gate_above", "gate", {"min_triangulation_angle": deg_above}))


def case(name):
    for c in cases() + gate_cases():
        if c[0] == name:
            return c
    raise KeyError(name)


def case_names():
    return [c[0] for c in cases()] + ["gate_equal", "gate_above"]


@functools.lru_cache(maxsize=None)
def reference(name):
    _, model_name, kw = case(name) if name not in ("gate",) else ("gate", "gate", {})
    m = model(model_name)
    kw = dict(kw)
    if "candidate_mask" in kw:
        kw["candidate_mask"] = list(kw["candidate_mask"])
    return ref.select(m["R"], m["T"], m["xyz"], m["tracks"], **kw)


def same(result, want):
    """None, or what differs between a result dict (capi) and the restatement's, compared bit for bit."""
    if [list(s) for s in result["sources"]] != [list(s) for s in want["sources"]]:
        bad = [a for a in range(len(want["sources"])) if list(result["sources"][a]) != list(want["sources"][a])]
        return "sources of image %d: %r, the restatement has %r" % (bad[0], result["sources"][bad[0]], want["sources"][bad[0]])
    if np.asarray(result["depth_ranges"], dtype=f32).tobytes() != np.asarray(want["depth_ranges"], dtype=f32).tobytes():
        return "depth ranges differ"
    for k, what in enumerate(("a", "b", "count")):
        if np.asarray(result["pairs"][k]).tolist() != np.asarray(want["pairs"][k]).tolist():
            return "pair table: %s differs" % what
    got, exp = np.asarray(result["pairs"][3], dtype=f32).view(np.uint32), np.asarray(want["pairs"][3], dtype=f32).view(np.uint32)
    nan = np.isnan(np.asarray(want["pairs"][3], dtype=f32))  # any NaN of the restatement is the quiet NaN of the device
    if not (np.where(nan, np.isnan(np.asarray(result["pairs"][3], dtype=f32)), got == exp)).all():
        k = int(np.nonzero(~np.where(nan, np.isnan(np.asarray(result["pairs"][3], dtype=f32)), got == exp))[0][0])
        return "pair (%d, %d): angle bits %08x, the restatement has %08x" % (want["pairs"][0][k], want["pairs"][1][k], got[k], exp[k])
    return None
