"""Re-triangulation of the separators on the device (dsm_retriangulate) against the sequential numpy
restatement (tests/retriangulation_ref.py): decisions identical and xyz within 1e-9 relative wherever every margin of the
scene is >= 1e-9; totals within 2 % otherwise.  Also byte-identical repeats and shuffles, the argument errors, and the chain
dsm_align_clusters -> merge -> dsm_retriangulate -> dsm_bundle_adjust."""
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import oracle_lib
from tests import retriangulation_ref as ref

pytestmark = pytest.mark.gpu
MARGIN = 1e-9
RTOL = 1e-9


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def to_world():
    orc = oracle_lib.load()
    return lambda cam, xy: orc.image_to_world(cam, np.asarray(xy, np.float64))


def compare(dev, exp, clear_required=False):
    """True when compared decision for decision, False when the scene is unclear (totals checked)."""
    clear = ref.min_margin(exp) >= MARGIN
    if clear_required:
        assert clear, ref.min_margin(exp)
    if not clear:
        assert abs(int(dev["num_tris"]) - exp["num_tris"]) <= max(2, 0.02 * exp["num_tris"])
        return False
    assert int(dev["num_tris"]) == exp["num_tris"]
    assert [int(x) for x in dev["new_point_ids"]] == exp["new_point_ids"]
    offs = dev["new_track_offsets"]
    tracks = [[tuple(int(v) for v in o) for o in dev["new_track_obs"][offs[k]:offs[k + 1]]] for k in range(len(offs) - 1)]
    assert tracks == [[tuple(t) for t in tr] for tr in exp["new_tracks"]]
    if exp["new_xyz"]:
        e = np.array(exp["new_xyz"])
        assert (np.abs(dev["new_xyz"] - e) <= RTOL * np.maximum(np.abs(e), 1.0)).all()
    assert [(int(a), int(b), int(c)) for (a, b), c in zip(dev["continued_obs"], dev["continued_point_ids"])] == exp["continued"]
    return True


def run(ctx, scene, seps, to_world=None, **kw):
    o = capi.default_triangulation_options(**kw)
    dev = ctx.retriangulate(scene, seps, o)
    exp = ref.triangulate(scene, seps, options=kw, to_world=to_world)
    return dev, exp


def test_hand_scenes(ctx):
    s, _ = ref.make_scene(n_images=2, n_points=10, track=(2, 2), noise=0.05, wrong=0.0, seed=4)
    sep = [int(s["image_ids"][0])]
    for kw in ({}, {"ignore_two_view_tracks": 0}):
        dev, exp = run(ctx, s, sep, **kw)
        compare(dev, exp, clear_required=True)
    s, _ = ref.make_scene(n_images=4, n_points=30, track=(4, 4), noise=0.1, wrong=0.0, existing=1.0, seed=5)
    dev, exp = run(ctx, s, [int(s["image_ids"][-1])])
    assert len(exp["continued"]) > 0 and compare(dev, exp)
    s, _ = ref.make_scene(n_images=5, n_points=40, track=(5, 5), noise=0.1, wrong=0.0, seed=7, unregistered=(4,))
    dev, exp = run(ctx, s, [int(s["image_ids"][0]), int(s["image_ids"][4])])
    assert compare(dev, exp) and list(dev["num_tris_per_separator"])[1] == 0
    s2 = dict(s, cameras=[capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)])
    dev = ctx.retriangulate(s2, [int(s["image_ids"][0])])
    assert dev["num_tris"] == 0 and dev["report"].num_separators == 0


CAMS = [(0, [500, 320, 240]), (1, [500, 510, 320, 240]), (2, [500, 320, 240, 0.01]), (3, [500, 320, 240, 0.01, -0.005]),
        (4, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005]), (5, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005]),
        (6, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005, 0.001, 0.0, 0.0, 0.0]), (7, [500, 510, 320, 240, 0.05]),
        (8, [500, 320, 240, 0.01]), (9, [500, 320, 240, 0.01, -0.005]),
        (10, [500, 510, 320, 240, 0.01, -0.005, 0.001, 0.0005, 0.001, 0.0, 0.0005, 0.0005])]


@pytest.mark.parametrize("model", range(11))
def test_random_scenes_every_camera_model(ctx, to_world, model):
    mid, params = CAMS[model]
    cams = [capi.camera(mid, params, 640, 480), capi.simple_pinhole(480.0, 320.0, 240.0, 640, 480)]
    clear = 0
    for seed in range(3):
        s, _ = ref.make_scene(n_images=9, n_points=90, track=(2, 7), noise=0.3, wrong=0.1, existing=0.2, cameras=cams,
                              seed=100 * model + seed)
        seps = [int(x) for x in s["image_ids"][2:7]]
        dev, exp = run(ctx, s, seps, to_world=to_world)
        clear += compare(dev, exp)
        assert dev["report"].num_problems == len(exp["problems"])
    assert clear >= 2


def test_long_tracks_dynamic_trials(ctx):
    s, _ = ref.make_scene(n_images=24, n_points=40, track=(17, 24), noise=0.3, wrong=0.15, seed=11, spacing=0.3)
    dev, exp = run(ctx, s, [int(s["image_ids"][12])])
    compare(dev, exp)
    assert dev["report"].ransac_trials > 0 and max(len(t) for t in exp["new_tracks"]) > 15


def test_shared_separators_force_rounds(ctx):
    s, _ = ref.make_scene(n_images=10, n_points=120, track=(3, 8), noise=0.3, wrong=0.1, existing=0.3, seed=12)
    seps = [int(x) for x in s["image_ids"]][::-1]  # every image a separator, in descending order: sorted by the call
    dev, exp = run(ctx, s, seps)
    assert dev["report"].num_rounds > 1 and dev["report"].num_deferred > 0
    compare(dev, exp)
    assert [int(x) for x in dev["num_tris_per_separator"]] == [exp["num_tris_per_separator"][i] for i in seps] or \
        ref.min_margin(exp) < MARGIN


def test_random_scene_clear_fraction(ctx):
    clear, total = 0, 0
    for seed in range(20):
        s, _ = ref.make_scene(n_images=8, n_points=70, track=(2, 6), noise=0.3, wrong=0.1, existing=0.25, seed=500 + seed)
        dev, exp = run(ctx, s, [int(x) for x in s["image_ids"][1:7]])
        clear += compare(dev, exp)
        total += 1
    assert clear >= 0.9 * total, (clear, total)


def shuffled(s, rng, points=True, matches=True):
    s = dict(s)
    if points and len(s["point3D_ids"]):
        perm = rng.permutation(len(s["point3D_ids"]))
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        s["point3D_ids"], s["point3D_xyz"] = s["point3D_ids"][perm], s["point3D_xyz"][perm]
        p3 = s["points2D_point3D"]
        s["points2D_point3D"] = np.where(p3 >= 0, inv[np.maximum(p3, 0)], -1).astype(np.int32)
    if matches:
        m = s["matches"].copy()
        off = s["match_offsets"]
        for k in range(len(off) - 1):
            m[off[k]:off[k + 1]] = m[off[k]:off[k + 1]][rng.permutation(int(off[k + 1] - off[k]))]
        s["matches"] = m
    return s


def same(a, b):
    for k in ("new_point_ids", "new_xyz", "new_track_offsets", "new_track_obs", "continued_obs", "continued_point_ids",
              "touched_obs", "touched_point_ids", "num_tris_per_separator"):
        assert a[k].tobytes() == b[k].tobytes(), k


def test_byte_identical_repeats_and_shuffles(ctx):
    rng = np.random.default_rng(13)
    s, _ = ref.make_scene(n_images=10, n_points=150, track=(2, 8), noise=0.3, wrong=0.1, existing=0.3, seed=13)
    seps = [int(x) for x in s["image_ids"][1:9]]
    base = ctx.retriangulate(s, seps)
    assert base["report"].num_tris > 0 and base["report"].num_continued > 0
    same(base, ctx.retriangulate(s, seps))
    same(base, ctx.retriangulate(shuffled(s, rng, matches=False), seps))
    same(base, ctx.retriangulate(shuffled(s, rng, points=False), seps))
    same(base, ctx.retriangulate(shuffled(s, rng), seps))


def split_scene():
    """one feature per image, 7 images: 0, 1, 2 and 6 see point A, 3..5 see point B; image 6 is matched to 1 and 2 only.
    Separator 0's Create splits its list (images 0..5) into two points by the recursion, B first (depth 0), then A (depth 1);
    separator 6, in a later round, continues onto A, the point of the second level."""
    rng = np.random.default_rng(6)
    s, truth = ref.make_scene(n_images=7, n_points=1, track=(7, 7), noise=0.0, wrong=0.0, seed=6, spacing=2.0)
    A = truth[(int(s["image_ids"][0]), 0)]
    B = A + np.array([3.0, 2.0, 0.0])
    for i in range(7):
        P, _ = ref.pose_matrix(s["qvec"][i], s["tvec"][i])
        x = np.array(P).reshape(3, 4) @ np.append(B if 3 <= i <= 5 else A, 1.0)
        s["points2D_xy"][i] = [500.0 * x[0] / x[2] + 320.0, 500.0 * x[1] / x[2] + 240.0] + rng.normal(0, 0.05, 2)
    ids = [int(v) for v in s["image_ids"]]
    keep = [k for k, (a, b) in enumerate(s["pairs"]) if not (int(b) == ids[6] and int(a) not in ids[1:3])]
    s["pairs"] = s["pairs"][keep]
    s["matches"] = s["matches"][keep]
    s["match_offsets"] = np.arange(len(keep) + 1, dtype=np.uint64)
    return s, ids


def test_recursive_create_and_continue_onto_a_second_level_point(ctx):
    s, ids = split_scene()
    dev, exp = run(ctx, s, [ids[6], ids[0]])
    assert compare(dev, exp, clear_required=True)
    first = int(dev["new_point_ids"][0])
    assert [int(x) for x in dev["new_point_ids"]] == [first, first + 1]  # one problem, depths 0 and 1
    offs = dev["new_track_offsets"]
    tracks = [sorted(int(o[0]) for o in dev["new_track_obs"][offs[k]:offs[k + 1]]) for k in range(2)]
    assert sorted(tracks) == [ids[0:3], ids[3:6]]
    assert tracks[1] == ids[0:3]                                         # A came from the second level
    assert [tuple(int(v) for v in o) for o in dev["continued_obs"]] == [(ids[6], 0)]
    assert [int(x) for x in dev["continued_point_ids"]] == [first + 1]  # Continue read the depth-1 point
    assert dev["report"].num_rounds == 2 and dev["report"].num_problems == 2
    assert [int(x) for x in dev["num_tris_per_separator"]] == [1, 6]


def test_invalid_arguments(ctx):
    s, _ = ref.make_scene(n_images=4, n_points=30, track=(2, 4), noise=0.3, wrong=0.0, existing=0.3, seed=14)
    seps = [int(s["image_ids"][1])]
    ctx.retriangulate(s, seps)

    def bad(_seps=None, **kw):
        opts = kw.pop("_opts", None)
        with pytest.raises(capi.DsmError):
            ctx.retriangulate(dict(s, **kw), seps if _seps is None else _seps, capi.default_triangulation_options(**(opts or {})))

    def changed(key, idx, value):
        a = np.array(s[key], copy=True)
        a[idx] = value
        return a

    p = s["pairs"].copy()
    p[1] = [p[1][0], p[1][0]]
    bad(pairs=p)                                                     # self-pair
    p = s["pairs"].copy()
    p[1] = p[0][::-1]
    bad(pairs=p)                                                     # repeated pair, other order
    bad(pairs=changed("pairs", (0, 1), 999))                        # a pair on an unknown image id
    bad(image_ids=changed("image_ids", 1, s["image_ids"][0]))        # repeated image id
    bad(image_camera_ids=changed("image_camera_ids", 0, 999))        # an image on an unknown camera id
    bad(matches=changed("matches", (0, 0), 10 ** 6))                 # index out of range
    bad(points2D_point3D=changed("points2D_point3D", 0, len(s["point3D_ids"])))
    bad(points2D_xy=changed("points2D_xy", (3, 1), np.nan))          # non-finite input
    bad(qvec=changed("qvec", (2, 1), np.inf))
    bad(tvec=changed("tvec", (2, 0), np.nan))
    bad(point3D_xyz=changed("point3D_xyz", (0, 2), np.nan))
    bad(qvec=changed("qvec", 2, 0.0))                                # a zero qvec
    bad(points2D_offsets=changed("points2D_offsets", 0, 1))          # offsets not starting at 0 / decreasing
    po = s["points2D_offsets"]
    bad(points2D_offsets=changed("points2D_offsets", 2, int(po[1]) - 1))
    bad(match_offsets=changed("match_offsets", 0, 1))
    mo = s["match_offsets"]
    bad(match_offsets=changed("match_offsets", 1, int(mo[2]) + 1))
    c = capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480)
    c.model_id = 11
    bad(cameras=[c])                                                 # unknown model
    bad(_seps=[999])                                                 # a separator on an unknown image id
    bad(_seps=seps + seps)                                           # a repeated separator
    for opts in ({"max_transitivity": 2}, {"max_transitivity": 0}, {"create_max_angle_error": 0.0}, {"min_angle": -1.0},
                 {"continue_max_angle_error": -1.0}, {"ransac_confidence": 1.0}, {"ransac_max_num_trials": 0},
                 {"max_focal_length_ratio": 0.05}, {"min_focal_length_ratio": 0.0}, {"ransac_min_inlier_ratio": 2.0},
                 {"max_extra_param": -1.0}, {"create_max_angle_error": np.inf}):
        bad(_opts=opts)
    with pytest.raises(capi.DsmError):                               # next id at or below an existing one
        ctx.retriangulate(s, seps, None, next_point3D_id=int(s["point3D_ids"].max()))
    ctx.retriangulate(s, seps)                                       # the context is still usable


def test_chain_align_merge_retriangulate_bundle_adjust(ctx):
    """two clusters of one scene, each in its own planted Sim3 frame -> dsm_align_clusters (separators and transforms) ->
    the test's merge into the anchor's frame -> dsm_retriangulate -> dsm_bundle_adjust"""
    s, truth = ref.make_scene(n_images=12, n_points=240, track=(2, 6), noise=0.3, wrong=0.0, existing=0.5, seed=21)
    rng = np.random.default_rng(22)
    ids = [int(x) for x in s["image_ids"]]
    off = s["points2D_offsets"]
    p3 = s["points2D_point3D"]
    windows = [range(0, 7), range(5, 12)]
    planted = [(1.0, np.eye(3), np.zeros(3)), (1.7, ref.look_at_qvec(np.zeros(3), [1.0, 0.5, 2.0], rng)[1], np.array([4.0, -2.0, 1.0]))]
    clusters = []
    for w, (sc, Rc, tc) in zip(windows, planted):
        obs, pts = [], {}
        for i in w:
            for k in range(int(off[i + 1] - off[i])):
                p = int(p3[off[i] + k])
                if p >= 0:
                    obs.append((ids[i], k, pts.setdefault(p, len(pts))))
        order = sorted(pts, key=pts.get)
        clusters.append(dict(image_ids=np.array([ids[i] for i in w], np.uint32), point_ids=s["point3D_ids"][order],
                             xyz=sc * (s["point3D_xyz"][order] @ Rc.T) + tc, obs=np.array(obs, np.uint32).reshape(-1, 3),
                             order=order))
    al = ctx.align_clusters([{k: v for k, v in c.items() if k != "order"} for c in clusters])
    seps = [int(x) for x in al["separators"]]
    assert seps == ids[5:7]
    a = al["anchor"]
    # the merge: every point and pose into the anchor's frame with the returned Sim3s (the first cluster that holds it wins)
    merged = dict(s)
    xyz = np.zeros_like(s["point3D_xyz"])
    done = np.zeros(len(xyz), bool)
    qvec, tvec = np.zeros_like(s["qvec"]), np.zeros_like(s["tvec"])
    for c, (w, (sc, Rc, tc)) in enumerate(zip(windows, planted)):
        S, R, t = al["s"][c], al["R"][c], al["t"][c]
        for q, p in enumerate(clusters[c]["order"]):
            if not done[p]:
                xyz[p] = S * (R @ clusters[c]["xyz"][q]) + t
                done[p] = True
        for i in w:
            if qvec[i].any():
                continue
            Rw = ref.pose_matrix(s["qvec"][i], s["tvec"][i])[0]
            Rw, tw = np.array(Rw).reshape(3, 4)[:, :3], np.asarray(s["tvec"][i], float)
            R1 = Rw @ Rc.T                      # the pose in cluster c's frame
            t1 = sc * tw - R1 @ tc
            R2 = R1 @ R.T                       # and in the anchor's
            tvec[i] = S * t1 - R2 @ t
            qvec[i] = ref.rot_to_quat(R2)
    merged.update(point3D_xyz=xyz, qvec=qvec, tvec=tvec)
    out = ctx.retriangulate(merged, seps)
    assert out["report"].num_new_points > 0
    sa, Ra, ta = planted[a]
    offs = out["new_track_offsets"]
    errs = [np.linalg.norm(out["new_xyz"][k] - (sa * (Ra @ truth[tuple(int(v) for v in out["new_track_obs"][offs[k]])]) + ta)) / sa
            for k in range(len(offs) - 1)]
    assert np.median(errs) < 0.05 and np.mean(np.array(errs) < 0.2) > 0.9
    exp = ref.triangulate(merged, seps)                      # and the restatement on the merged reconstruction
    compare(out, exp)
    # the merged reconstruction for BA: existing tracks + continued observations + new points
    s = merged
    tracks = {}
    for i in range(len(ids)):
        for k in range(int(off[i + 1] - off[i])):
            if p3[off[i] + k] >= 0:
                tracks.setdefault(int(s["point3D_ids"][p3[off[i] + k]]), []).append((i, k))
    for (img, k), pid in zip(out["continued_obs"], out["continued_point_ids"]):
        tracks[int(pid)].append((ids.index(int(img)), int(k)))
    xyz = {int(p): x for p, x in zip(s["point3D_ids"], s["point3D_xyz"])}
    for kk in range(len(offs) - 1):
        pid = int(out["new_point_ids"][kk])
        xyz[pid] = out["new_xyz"][kk]
        tracks[pid] = [(ids.index(int(a)), int(b)) for a, b in out["new_track_obs"][offs[kk]:offs[kk + 1]]]
    pids = sorted(p for p in tracks if len(tracks[p]) >= 2)
    obs_image = [i for p in pids for i, _ in tracks[p]]
    obs_xy = [s["points2D_xy"][off[i] + k] for p in pids for i, k in tracks[p]]
    toff = np.concatenate([[0], np.cumsum([len(tracks[p]) for p in pids])])
    cam = s["cameras"][0]
    ba_scene = dict(camera_model_ids=[cam.model_id], camera_params=list(cam.params)[:3], image_camera=np.zeros(len(ids)),
                    qvec=s["qvec"], tvec=s["tvec"], image_constant_pose=np.array([1, 1] + [0] * (len(ids) - 2)),
                    point_ids=np.array(pids, np.uint64), xyz=np.array([xyz[p] for p in pids]), track_offsets=toff,
                    obs_image=obs_image, obs_xy=obs_xy)
    ba = ctx.bundle_adjust(ba_scene)
    assert ba["report"].termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE)
    assert ba["report"].final_cost <= ba["report"].initial_cost
    assert math.isfinite(ba["report"].final_cost)
