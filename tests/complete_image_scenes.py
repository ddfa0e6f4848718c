"""Scenes of the CompleteImage tests: hand-built known answers, one per branch of the reference's loop, and
random reconstructions with observations stripped and whole points taken out, so there is something to complete and something
to create.

The hand-built scenes use tests/track_update_scenes.py's geometry (Tiny): SIMPLE_PINHOLE f = 500, image i looks along +z from
(0.5 i, 0, -8) with the identity rotation, the points lie at z = 0, a feature is the exact projection of its point plus a stated
offset in pixels.  Two neighbouring images see a point at the origin under 3.58 degrees (min_angle 1.5).  Answers that follow by
hand:
  * a list of n <= 15 entries always takes C(n, 2) LORANSAC trials (min_num_trials = max_num_trials = C(n, 2));
  * a list of 16 exact inliers finds all 16 at trial 0, so ComputeNumTrials gives 1: with min_num_trials = 0 the abort is set
    at trial 1 and the loop ends with 3 trials counted; with min_num_trials = 3 it is set at trial 3: 5 trials;
  * a new point's track is the list's inliers in list order: the correspondences in (pair, match) order, then the point2D;
  * the first new id is the largest id + 1 (1 in a scene without points).
New points' xyz are estimates (compared with the restatement by tolerance); tracks, ids, counts and trials are exact."""
import numpy as np

from tests import complete_image_ref as ref
from tests import track_update_scenes as tus

MERGE, COMPLETE = ref.MERGE, ref.COMPLETE
MIN_MARGIN = 1e-9
Tiny, O = tus.Tiny, tus.O


def _case(t, images, tracks, tris, modified, complete_trials, ransac_trials, steps=(), selected=None, counts=(), **options):
    """images: image indices to complete, in order; tracks: {id: [(image index, point2D_idx)]} of the whole result."""
    return dict(scene=t.scene(), images=[t.image_id(i) for i in images], steps=list(steps), selected=selected, options=options,
                tracks={int(p): t.obs(e) for p, e in tracks.items()}, tris=list(tris), modified=sorted(modified), counts=list(counts),
                complete_trials=complete_trials, ransac_trials=ransac_trials)


def X(j, step=0.1):
    return np.array([step * j, 0.0, 0.0])


def _simple(n_images, **kw):
    """r in image 0 with one correspondence in every other image, all exact projections of the origin"""
    t = Tiny(n_images, **kw)
    r = t.feat(0, O)
    c = [t.feat(i, O) for i in range(1, n_images)]
    for x in c:
        t.link(r, x)
    return t, r, c


def _list_of(n):
    """one item whose list holds n entries: n - 1 correspondences and the point2D, all inliers"""
    t, r, c = _simple(n)
    trials = n * (n - 1) // 2 if n <= 15 else 3
    return _case(t, [0], {1: c + [r]}, [n], [1], 0, trials, ignore_two_view_tracks=0)


def _carried(two_images):
    """Item a: 2 correspondences (n = 3, leaves min_num_trials = 3).  Item b: 15 correspondences (n = 16).  In one image b runs
    with 3 (5 trials), in two images with 0 (3 trials)."""
    t = Tiny(17)
    Xa, Xb = O, X(3)
    ib = 16 if two_images else 0
    ra = t.feat(0, Xa)
    rb = t.feat(ib, Xb)
    ca = [t.feat(1, Xa), t.feat(2, Xa)]
    cb = [t.feat(i, Xb) for i in range(1, 16)]
    for x in ca:
        t.link(ra, x)
    for x in cb:
        t.link(rb, x)
    if two_images:
        return _case(t, [0, 16], {1: ca + [ra], 2: cb + [rb]}, [3, 16], [1, 2], 0, 3 + 3)
    return _case(t, [0], {1: ca + [ra], 2: cb + [rb]}, [3 + 16], [1, 2], 0, 3 + 5)


def _reach(r_offset, with_h):
    """Point 10 = [a0 (image 0, point2D 0), a1]; a1 - f2 - g - r, r is image 0's point2D 1 and g its only correspondence."""
    t = Tiny(5)
    a0, a1 = t.feat(0, O), t.feat(1, O)
    r = t.feat(0, O, dx=r_offset)
    f2, g = t.feat(2, O), t.feat(3, O)
    t.link(a0, a1)
    t.link(a1, f2)
    t.link(f2, g)
    t.link(g, r)
    t.point(10, O, [a0, a1])
    h = None
    if with_h:
        h = t.feat(4, O)
        t.link(r, h)
    return t, a0, a1, r, f2, g, h


def chain(k):
    """k listed images with one item each.  Item j (image j, its point X(j)) has a correspondence u_j of its own (image k), s_j
    (image k + 1 + j, a projection of X(j)) and, for j >= 1, s_(j - 1), which item j - 1 has too.  Item 0 creates
    [u_0, s_0, r_0] (3 trials); item 1 finds s_0 taken and is skipped; so s_1 is free at item 2's turn, an outlier of its list
    of 4 (6.25 px; 6 trials), and so on: the even items create, the odd ones are skipped."""
    t = Tiny(2 * k + 1)
    r = [t.feat(j, X(j)) for j in range(k)]
    u = [t.feat(k, X(j)) for j in range(k)]
    s = [t.feat(k + 1 + j, X(j)) for j in range(k)]
    for j in range(k):
        t.link(r[j], u[j])
    for j in range(k):
        t.link(r[j], s[j])
        if j + 1 < k:
            t.link(r[j + 1], s[j])
    tracks = {1 + j // 2: [u[j], s[j], r[j]] for j in range(0, k, 2)}
    n_even = (k + 1) // 2
    return _case(t, list(range(k)), tracks, [3 if j % 2 == 0 else 0 for j in range(k)], list(tracks), 0, 3 + 6 * (n_even - 1))


def many_items(K):
    """K items in one image, each with a correspondence in images 1 and 2: K new points, 3 trials each"""
    t = Tiny(3)
    tracks = {}
    for j in range(K):
        Xj = X(j, 0.02)
        r, a, b = t.feat(0, Xj), t.feat(1, Xj), t.feat(2, Xj)
        t.link(r, a)
        t.link(r, b)
        tracks[1 + j] = [a, b, r]
    return _case(t, [0], tracks, [3 * K], list(tracks), 0, 3 * K)


def long_complete(L):
    """Image 0's point2D has a point of L elements (images 0 .. L - 1); the last element has a free correspondence"""
    t = Tiny(L + 1)
    a = [t.feat(i, O) for i in range(L)]
    f = t.feat(L, O)
    t.link(a[-1], f)
    t.point(21, O, a)
    return _case(t, [0], {21: a + [f]}, [1], [21], 1, 0)


def cases():
    """name -> case.  Every answer is worked out in the comment above its scene."""
    out = {}
    # the image is not registered / its camera has bogus parameters: CompleteImage returns 0 before the loop
    for name, kw in (("unregistered_image", dict(unregistered=(0,))), ("bogus_camera", dict(bogus=(0,)))):
        t, r, c = _simple(3, **kw)
        out[name] = _case(t, [0], {}, [0], [], 0, 0)
    # point2D 0 has point 10 = [a0, a1]: Complete(10) tests f2 through a1 (1 trial) and takes it
    t = Tiny(3)
    a0, a1, f2 = t.feat(0, O), t.feat(1, O), t.feat(2, O)
    t.link(a0, a1)
    t.link(a1, f2)
    t.point(10, O, [a0, a1])
    out["complete_branch"] = _case(t, [0], {10: [a0, a1, f2]}, [1], [10], 1, 0)
    # r - c and nothing else: a two-view observation, ignored ...
    t, r, c = _simple(2)
    out["two_view_ignored"] = _case(t, [0], {}, [0], [], 0, 0)
    # ... and with ignore_two_view_tracks = 0 a list of 2: one trial, the track is [c, r]
    out["two_view_triangulated"] = _case(t, [0], {1: c + [r]}, [2], [1], 0, 1, ignore_two_view_tracks=0)
    # r's correspondence a1 has a point (a1 has a second correspondence: no two-view observation): skipped, no estimate
    t = Tiny(3)
    r, a1, a2 = t.feat(0, O), t.feat(1, O), t.feat(2, O)
    t.link(r, a1)
    t.link(a1, a2)
    t.point(10, O, [a1, a2])
    out["correspondence_has_point"] = _case(t, [0], {10: [a1, a2]}, [0], [], 0, 0)
    # r's only correspondence is in an unregistered image / on a bogus camera: the list is empty after Find
    for name, kw in (("empty_unregistered", dict(unregistered=(1,))), ("empty_bogus", dict(bogus=(1,)))):
        t = Tiny(3, **kw)
        r, f1, f2 = t.feat(0, O), t.feat(1, O), t.feat(2, O)
        t.link(r, f1)
        t.link(f1, f2)
        out[name] = _case(t, [0], {}, [0], [], 0, 0)
    # two views 3.58 degrees apart under min_angle 5: the only sample gives no model, 1 trial
    t, r, c = _simple(2)
    out["angle_below_min"] = _case(t, [0], {}, [0], [], 0, 1, ignore_two_view_tracks=0, min_angle=5.0)
    # image 1 stands behind the point looking away: the rays meet at the point, which has depth -8 there
    t, r, c = _simple(2, behind=(1,))
    out["negative_depth"] = _case(t, [0], {}, [0], [], 0, 1, ignore_two_view_tracks=0)
    # the correspondence is 40 px off across the epipolar line: the rays are skew, the midpoint is 20 px from both features,
    # the model has no inlier
    t = Tiny(2)
    r, c1 = t.feat(0, O), t.feat(1, O, dy=40.0)
    t.link(r, c1)
    out["no_inliers"] = _case(t, [0], {}, [0], [], 0, 1, ignore_two_view_tracks=0)
    # the point2D is 30 px off along the epipolar lines: its samples meet at another depth with two inliers, the three
    # correspondences agree: the new track is without the point2D that started it.  C(4, 2) = 6 trials
    t = Tiny(4)
    r = t.feat(0, O, dx=30.0)
    c = [t.feat(i, O) for i in (1, 2, 3)]
    for x in c:
        t.link(r, x)
    out["reference_is_outlier"] = _case(t, [0], {1: c}, [3], [1], 0, 6)
    # the third correspondence is 30 px off: the track is the other two and the point2D
    t = Tiny(4)
    r = t.feat(0, O)
    c = [t.feat(1, O), t.feat(2, O), t.feat(3, O, dx=30.0)]
    for x in c:
        t.link(r, x)
    out["inlier_subset"] = _case(t, [0], {1: [c[0], c[1], r]}, [3], [1], 0, 6)
    # list sizes: 3 (the local optimisation begins), 15 (the last exhaustive one, 105 trials), 16 (min_num_trials 0: 3 trials)
    for n in (3, 15, 16):
        out["list_%d" % n] = _list_of(n)
    out["carried_min_trials"] = _carried(False)
    out["carried_resets_per_image"] = _carried(True)
    # Complete(10) at point2D 0 walks a1 -> f2 (trial 1, taken) -> g (trial 2, taken) -> r (trial 3: 50 px off, refused).  r
    # is point2D 1: its only correspondence g has a point now, so it is skipped (without the walk r and g would triangulate)
    t, a0, a1, r, f2, g, _ = _reach(50.0, False)
    out["complete_takes_the_correspondence"] = _case(t, [0], {10: [a0, a1, f2, g]}, [2], [10], 3, 0)
    # complete_max_transitivity 3, r exact: the walk takes f2, g and r (level 2, the last: r is not enqueued), so h behind r is
    # not tested.  Point2D 1 = r has the point now: a second Complete(10) over the whole track tests h through r (trial 4)
    t, a0, a1, r, f2, g, h = _reach(0.0, True)
    out["second_complete_of_the_point"] = _case(t, [0], {10: [a0, a1, f2, g, r, h]}, [4], [10], 4, 0, complete_max_transitivity=3)
    # rA (image 0) has c1, c2; rC (image 3) has c2, c4; all see the origin.  [A, C]: A creates [c1, c2, rA], C finds c2 taken.
    # [C, A]: C creates [c2, c4, rC] (pair (2, 3) was linked before (3, 4)), A finds c2 taken
    t = Tiny(5)
    rA, c1, c2, rC, c4 = t.feat(0, O), t.feat(1, O), t.feat(2, O), t.feat(3, O), t.feat(4, O)
    t.link(rA, c1)
    t.link(rA, c2)
    t.link(rC, c2)
    t.link(rC, c4)
    out["order_A_C"] = _case(t, [0, 3], {1: [c1, c2, rA]}, [3, 0], [1], 0, 3)
    out["order_C_A"] = _case(t, [3, 0], {1: [c2, c4, rC]}, [3, 0], [1], 0, 3)
    for k in (1, 2, 9):
        out["chain_%d" % k] = chain(k)
    for K in (63, 64, 65):
        out["items_%d" % K] = many_items(K)
    for L in (16, 17):
        out["complete_track_%d" % L] = long_complete(L)
    return out


def check_case(case, got):
    """got (the dict of complete_images, the library's or the restatement's) against the hand-computed answer: tracks, ids,
    image_num_tris, modified ids and both trial counts exactly; existing points' xyz bit for bit."""
    ids = sorted(case["tracks"])
    assert [int(i) for i in got["point_ids"]] == ids
    toff = [int(x) for x in got["track_offsets"]]
    sc = case["scene"]
    old = {int(p): k for k, p in enumerate(sc["point3D_ids"])}
    for k, pid in enumerate(ids):
        assert [tuple(int(v) for v in o) for o in got["track_obs"][toff[k]:toff[k + 1]]] == case["tracks"][pid], pid
        if pid in old:
            want = np.asarray(sc["point3D_xyz"], np.float64).reshape(-1, 3)[old[pid]]
            assert np.asarray(got["xyz"][k], np.float64).tobytes() == want.tobytes(), pid
    assert [int(c) for c in got["image_num_tris"]] == case["tris"]
    assert [int(i) for i in got["modified"]] == case["modified"]
    assert [int(c) for c in got["step_counts"]] == case["counts"]
    assert trial_counts(got) == (case["complete_trials"], case["ransac_trials"]), trial_counts(got)


def trial_counts(got):
    """(complete_trials, ransac_trials) of a restatement result or of a library result"""
    if "report" in got:
        return int(got["report"].complete_trials), int(got["report"].ransac_trials)
    return int(got["complete_trials"]), int(got["ransac_trials"])


def same_result(a, b, rtol=1e-9):
    """ids, track order, modified, counts, image_num_tris and both trial counts exactly; the xyz of the points of the input
    bit for bit where both sides are given them (old_ids), the others within rtol relative (the SVD and the
    eigen-solver of the restatement round differently from the device's Jacobi sweeps)."""
    for key in ("point_ids", "track_offsets", "track_obs", "modified", "step_counts", "image_num_tris"):
        assert np.array_equal(np.asarray(a[key], np.int64), np.asarray(b[key], np.int64)), key
    xa, xb = np.asarray(a["xyz"], np.float64), np.asarray(b["xyz"], np.float64)
    assert (np.abs(xa - xb) <= rtol * np.maximum(np.abs(xb), 1.0)).all(), "xyz"
    assert trial_counts(a) == trial_counts(b), "trial counts"


def old_xyz_same_bytes(scene, got):
    """every point of the input that is still in the result has its xyz unchanged, bit for bit"""
    old = {int(p): np.asarray(x, np.float64).tobytes() for p, x in zip(scene["point3D_ids"], np.asarray(scene["point3D_xyz"]).reshape(-1, 3))}
    n = 0
    for p, x in zip(got["point_ids"], got["xyz"]):
        if int(p) in old:
            assert np.asarray(x, np.float64).tobytes() == old[int(p)], int(p)
            n += 1
    return n


def result_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in
                    ("point_ids", "xyz", "track_offsets", "track_obs", "modified", "step_counts", "image_num_tris"))


def without_points(scene, fraction, seed):
    """The scene with a fraction of its points3D taken out whole: their features are free, and the first of them an image's
    loop meets starts a new point."""
    rng = np.random.default_rng([seed, 31337])
    toff = np.asarray(scene["track_offsets"], np.int64)
    tobs = np.asarray(scene["track_obs"]).reshape(-1, 2)
    keep = [p for p in range(len(toff) - 1) if rng.random() >= fraction]
    s = dict(scene)
    s["point3D_ids"] = np.asarray(scene["point3D_ids"])[keep]
    s["point3D_xyz"] = np.asarray(scene["point3D_xyz"]).reshape(-1, 3)[keep]
    s["track_offsets"] = np.concatenate([[0], np.cumsum((toff[1:] - toff[:-1])[keep])]).astype(np.uint64)
    s["track_obs"] = np.concatenate([tobs[toff[p]:toff[p + 1]] for p in keep] + [np.zeros((0, 2), tobs.dtype)]).reshape(-1, 2)
    return s


def random_scene(n_images, n_points, seed, cameras=None, **kw):
    """track_update_scenes.random_scene (a third of the observations stripped, some points split) with a quarter of the points
    taken out.  cameras: the scene's camera list replaced (a small distortion is observation noise)."""
    s = without_points(tus.random_scene(n_images, n_points, seed, **kw), 0.25, seed)
    if cameras is not None:
        # the features were projected by SIMPLE_PINHOLE f = 500, c = (320, 240): the same rays through the new cameras' focal
        # lengths and principal points
        from tests import retriangulation_ref as rt
        s["cameras"] = list(cameras)
        s["camera_ids"] = np.arange(len(cameras), dtype=np.uint32) + 7
        s["image_camera_ids"] = (np.arange(n_images, dtype=np.uint32) % len(cameras)) + 7
        off = np.asarray(s["points2D_offsets"], np.int64)
        xy = np.array(s["points2D_xy"], np.float64, copy=True).reshape(-1, 2)
        for i in range(n_images):
            cam = cameras[i % len(cameras)]
            for k in range(off[i], off[i + 1]):
                xy[k] = rt.world_to_image(cam, (xy[k, 0] - 320.0) / 500.0, (xy[k, 1] - 240.0) / 500.0)
        s["points2D_xy"] = xy
    return s


# one parameter set per camera model (tests/test_retriangulation_gpu.py's): focal lengths near 500, small distortion
CAMS = [(0, [500, 320, 240]), (1, [500, 510, 320, 240]), (2, [500, 320, 240, 0.01]), (3, [500, 320, 240, 0.01, -0.005]),
        (4, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005]), (5, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005]),
        (6, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005, 0.001, 0.0, 0.0, 0.0]), (7, [500, 510, 320, 240, 0.05]),
        (8, [500, 320, 240, 0.01]), (9, [500, 320, 240, 0.01, -0.005]),
        (10, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005, 0.001, 0.0, 0.0005, 0.0005])]
_models = {}


def model_scene(model, to_world):
    """(scene, image ids to complete, the restatement's result, seeds skipped): 6 images on camera model `model`, built once"""
    if model not in _models:
        from dagsfm_amd import capi
        mid, params = CAMS[model]
        cams = [capi.camera(mid, params, 640, 480)]
        images = [5, 0, 2]
        _, scene, exp, skipped = first_clear_seed(lambda seed: random_scene(6, 50, seed, cameras=cams), 100 * model + 1, images, to_world=to_world)
        _models[model] = (scene, [int(scene["image_ids"][i]) for i in images], exp, skipped)
    return _models[model]


def synthetic_scene(n_images, seed):
    return without_points(tus.synthetic_scene(n_images, seed), 0.25, seed)


# the random scenes of both suites: name -> (builder, first seed, images to complete (indices), steps)
RANDOM = {"small": (lambda seed: random_scene(8, 60, seed), 1, list(range(8)), ()),
          "small_steps": (lambda seed: random_scene(8, 60, seed), 1, [5, 2], (MERGE, COMPLETE)),
          "forty": (lambda seed: synthetic_scene(40, seed), 11, [39, 38, 7], ())}
MAX_SEED_SKIPS = 1  # of any 10 consecutive seeds
_random = {}


def run_ref(scene, images, steps=(), selected=None, to_world=None, **options):
    ids = [int(scene["image_ids"][i]) for i in images]
    return ref.complete_images(scene, ids, steps, selected, to_world=to_world, **options)


def first_clear_seed(build, seed, images, steps=(), to_world=None, tries=10, **options):
    """(seed, scene, the restatement's result, seeds skipped) of the first seed from `seed` on whose scene has every margin of
    the run at MIN_MARGIN or above"""
    for s in range(seed, seed + tries):
        scene = build(s)
        exp = run_ref(scene, images, steps, to_world=to_world, **options)
        if ref.min_margin(exp) >= MIN_MARGIN:
            return s, scene, exp, s - seed
    raise AssertionError("no clear scene in %d seeds" % tries)


def named_random_scene(name):
    """(scene, image ids to complete, steps, the restatement's result, seeds skipped), built once"""
    if name not in _random:
        build, seed, images, steps = RANDOM[name]
        _, scene, exp, skipped = first_clear_seed(build, seed, images, steps)
        _random[name] = (scene, [int(scene["image_ids"][i]) for i in images], list(steps), exp, skipped)
    return _random[name]


def digest(result):
    """sha256 over every array of a result dict (sorted keys, the report left out)"""
    import hashlib
    h = hashlib.sha256()
    for key in sorted(result):
        v = result[key]
        if key == "report":
            continue
        for part in (v if isinstance(v, (list, tuple)) else [v]):
            h.update(key.encode())
            h.update(np.ascontiguousarray(part).tobytes())
    return h.hexdigest()


def existing_entry_digests(ctx):
    """name -> digest of what dsm_update_tracks (both step orders), dsm_retriangulate and dsm_retriangulate_pairs return on one
    scene each: the entries whose code moved when dsm_complete_images was added"""
    from dagsfm_amd import capi
    from tests import retriangulation_ref as rt
    s = tus.named_random_scene("small")
    out = {"update_tracks_%d%d" % tuple(steps): digest(ctx.update_tracks(s, steps)) for steps in tus.STEP_ORDERS}
    scene, _ = rt.make_scene(n_images=8, n_points=60, track=(2, 6), noise=0.3, wrong=0.1, existing=0.3, seed=2)
    out["retriangulate"] = digest(ctx.retriangulate(scene, [int(i) for i in scene["image_ids"][2:6]]))
    scene, _ = rt.make_scene(n_images=8, n_points=80, track=(3, 6), noise=0.3, wrong=0.1, existing=0.3, seed=0)
    out["retriangulate_pairs"] = digest(ctx.retriangulate_pairs(scene, capi.default_pair_retriangulation_options()))
    return out


CASES = cases()


def invalid_cases():
    """(name, scene, image ids, options): every call dsm_complete_images refuses beyond what dsm_update_tracks refuses"""
    base = CASES["order_A_C"]["scene"]
    ids = CASES["order_A_C"]["images"]
    return [("unknown_image", base, [ids[0], 999], {}), ("repeated_image", base, [ids[0], ids[0]], {}),
            ("max_transitivity_2", base, ids, dict(max_transitivity=2)), ("max_num_trials_0", base, ids, dict(ransac_max_num_trials=0)),
            ("confidence_0", base, ids, dict(ransac_confidence=0.0)), ("confidence_1", base, ids, dict(ransac_confidence=1.0)),
            ("negative_min_angle", base, ids, dict(min_angle=-1.0)), ("nan_min_angle", base, ids, dict(min_angle=float("nan"))),
            ("transitivity_0", base, ids, dict(complete_max_transitivity=0)),
            ("nan_threshold", base, ids, dict(complete_max_reproj_error=float("nan")))]
