"""dsm_filter_points3D on the device against the sequential restatement (tests/point_filter_ref.py), DESIGN.md 16.

The comparison rule: a point whose margins are all >= 1e-9 in the restatement is clear and must agree decision for decision
(point_keep, every obs_keep bit, its compacted segment, its share of each num_filtered -- the device reports totals, so the
totals must agree up to what the unclear points can contribute); its error within ERROR_TOLERANCE (16 x the measured one-ulp
sensitivity, point_filter_scenes.py).  The other points must be reported, nothing more.  At most 1 % of a scene's points may
be unclear: test_point_filter_cpu.py holds every scene to that before it reaches a device."""
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import point_filter_ref as ref
from tests import point_filter_scenes as scenes
from tests import retriangulation_ref as rt
from tests.point_filter_scenes import ERROR_TOLERANCE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return capi.Context(0)


@pytest.fixture(scope="module")
def all_scenes():
    return scenes.scenes()


_expected = {}


def expected(name, scene, passes, **kw):
    """The restatement's answer, computed once per (scene, passes, selection, options) and left unchanged."""
    key = (name, passes, tuple(sorted((k, np.asarray(v).tobytes()) for k, v in kw.items())))
    if key not in _expected:
        _expected[key] = ref.filter_points3D(scene, passes=passes, **kw)
    return _expected[key]


def compare(scene, dev, exp, passes):
    toff = np.asarray(scene["track_offsets"], np.int64)
    P = len(toff) - 1
    clear = ref.clear_points(exp)
    unclear = np.nonzero(~clear)[0]
    assert len(unclear) <= 0.01 * P
    rep = dev["report"]
    assert rep.num_points == P and rep.num_observations == toff[-1]
    assert (dev["point_keep"][clear] == exp["point_keep"][clear]).all()
    dk, ek = np.asarray(dev["kept_track_offsets"], np.int64), exp["kept_track_offsets"]
    assert dk[0] == 0 and (np.diff(dk) >= 0).all() and dk[-1] == len(dev["kept_obs"]) == rep.num_observations_kept
    assert (np.diff(dk)[~dev["point_keep"]] == 0).all()
    for p in np.nonzero(clear)[0]:
        a, b = int(toff[p]), int(toff[p + 1])
        assert (dev["obs_keep"][a:b] == exp["obs_keep"][a:b]).all(), p
        assert dev["kept_obs"][dk[p]:dk[p + 1]].tolist() == exp["kept_obs"][ek[p]:ek[p + 1]].tolist(), p
        e, d = exp["point_error"][p], dev["point_error"][p]
        if e == -1.0 or not math.isfinite(e):
            assert d == e or (math.isnan(e) and math.isnan(d)), (p, d, e)
        else:
            assert abs(d - e) <= ERROR_TOLERANCE * abs(e), (p, d, e)
    for p in unclear:  # reported, nothing more
        assert dev["point_keep"][p] in (False, True) and (dev["point_error"][p] == -1.0 or dev["point_error"][p] >= 0)
    # the compaction is the obs_keep bits in order, whatever the points are
    assert dev["kept_obs"].tolist() == np.nonzero(dev["obs_keep"])[0].tolist()
    opoint = np.repeat(np.arange(P), np.diff(toff))
    assert (np.diff(dk) == np.bincount(opoint[dev["obs_keep"]], minlength=P)).all()
    assert not dev["obs_keep"][np.repeat(~dev["point_keep"], np.diff(toff))].any()
    slack = int(np.diff(toff)[unclear].sum()) + len(unclear)
    for k in range(4):
        assert abs(int(rep.num_filtered[k]) - int(exp["num_filtered"][k])) <= slack, k
        assert abs(int(rep.points_deleted[k]) - int(exp["points_deleted"][k])) <= len(unclear), k
        assert abs(int(rep.observations_deleted[k]) - int(exp["observations_deleted"][k])) <= slack, k
    assert rep.num_points_kept == dev["point_keep"].sum() and rep.num_selected == exp["selected"].sum()
    lens = np.diff(toff)
    assert rep.lane_path_tracks == (lens <= ref.LANE_CUT).sum() and rep.wave_path_tracks == (lens > ref.LANE_CUT).sum()
    if len(unclear) == 0:
        assert (dev["image_filtered"] == exp["image_filtered"]).all()
        assert rep.pairs_evaluated == exp["pairs_evaluated"]
        assert rep.mean_error_observations == exp["mean_error_observations"]
        for key in ("mean_reprojection_error", "mean_point_error"):
            e, d = exp[key], getattr(rep, key)
            assert (math.isnan(e) and math.isnan(d)) or abs(d - e) <= ERROR_TOLERANCE * abs(e), (key, d, e)
        for key in ("min_depth_margin", "min_error_margin", "min_angle_margin", "min_bogus_margin"):
            e, d = exp[key], getattr(rep, key)
            assert d == e or abs(d - e) <= 1e-6 * abs(e), (key, d, e)
    if not passes & ref.MEAN_ERROR:
        assert math.isnan(rep.mean_reprojection_error)


@pytest.mark.parametrize("passes", scenes.GRID_PASSES)
@pytest.mark.parametrize("name", ["edge", "models"])
def test_every_pass_alone_and_together(ctx, all_scenes, name, passes):
    """edge: tracks of 0 .. 3, around the lane / wave cut and of 300 views; models: all eleven camera models.  Both with
    observations behind cameras, gross outliers and a low-parallax group; observation counts that are no multiple of 64."""
    s = all_scenes[name]
    dev = ctx.filter_points3D(s, passes=passes)
    exp = expected(name, s, passes)
    compare(s, dev, exp, passes)
    if passes == 15:
        assert all(exp["points_deleted"][:3] > 0) and (dev["report"].wave_path_tracks > 0) == (name == "edge")


@pytest.mark.parametrize("n_obs", [ref.SCAN_BLOCK - 2, ref.SCAN_BLOCK - 1, ref.SCAN_BLOCK, 3 * ref.SCAN_BLOCK + 77])
def test_scan_block_edges(ctx, all_scenes, n_obs):
    """The compaction scans n_obs + 1 flags in blocks of SCAN_BLOCK: one block less one, exactly one, one more, two levels."""
    name = "obs%d" % n_obs
    s = all_scenes[name]
    assert len(s["obs_image"]) == n_obs
    compare(s, ctx.filter_points3D(s, passes=15), expected(name, s, 15), 15)


def test_three_scan_levels(ctx):
    """More than SCAN_BLOCK^2 observations: the scan's third level.  Identity rotations, so that depth is z + tz exactly and
    pass 1's closed form can be evaluated for every point in numpy."""
    rng = np.random.default_rng(31)
    P, L, N = 150001, 7, 50
    assert P * L + 1 > ref.SCAN_BLOCK ** 2
    s = {"camera_model_ids": [0], "camera_params": [500.0, 320.0, 240.0], "image_camera": np.zeros(N, np.uint32),
         "qvec": np.tile([1.0, 0, 0, 0], (N, 1)), "tvec": np.column_stack([np.zeros(N), np.zeros(N), rng.normal(size=N)]),
         "xyz": np.column_stack([rng.normal(size=P), rng.normal(size=P), rng.normal(scale=1.5, size=P) + 1.0]),
         "track_offsets": (np.arange(P + 1) * L).astype(np.uint32), "obs_image": rng.integers(0, N, P * L).astype(np.uint32),
         "obs_xy": np.zeros((P * L, 2))}
    dev = ctx.filter_points3D(s, passes=1)
    neg = (s["xyz"][:, 2][:, None] + s["tvec"][:, 2][s["obs_image"].reshape(P, L)]) < ref.EPS
    n = neg.sum(1)
    keep = (n == 0) | (L - n >= 2)
    obs_keep = (~neg & keep[:, None]).reshape(-1)
    assert (dev["point_keep"] == keep).all() and (dev["obs_keep"] == obs_keep).all()
    assert (dev["kept_obs"] == np.nonzero(obs_keep)[0]).all()
    assert (dev["kept_track_offsets"] == np.concatenate([[0], np.cumsum(obs_keep.reshape(P, L).sum(1))])).all()
    rep = dev["report"]
    assert rep.num_filtered[0] == np.where(keep, n, np.minimum(n, L - 1)).sum() and rep.points_deleted[0] == (~keep).sum()
    assert 0.05 < keep.mean() < 0.95


def test_selections(ctx, all_scenes):
    """point_selected, image_selected (FilterPoints3DInImages) and both: unselected points pass through the reprojection, angle and mean-error
    passes untouched, the negative-depth pass ignores the selection."""
    s = all_scenes["models"]
    P = len(s["xyz"])
    sel = scenes.selections(s)
    for tag, kw in sel.items():
        dev = ctx.filter_points3D(s, passes=15, **kw)
        exp = expected("models", s, 15, **kw)
        compare(s, dev, exp, 15)
        un = ~exp["selected"]
        assert (dev["point_error"][un] == -1.0).all()
        alone = expected("models", s, 1)  # an unselected point sees pass 1 and nothing else
        assert (dev["point_keep"][un] == alone["point_keep"][un]).all()
    assert 0 < expected("models", s, 15, **sel["i"])["selected"].sum() < P


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("point_keep", "obs_keep", "point_error", "kept_track_offsets", "kept_obs",
                                                                    "image_filtered")) and \
        all(list(getattr(a["report"], k)) == list(getattr(b["report"], k)) for k in ("num_filtered", "points_deleted", "observations_deleted"))


def permuted(s, perm):
    toff = np.asarray(s["track_offsets"], np.int64)
    idx = np.concatenate([np.arange(toff[p], toff[p + 1]) for p in perm] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = dict(s)
    out.update(xyz=s["xyz"][perm], point_ids=s["point_ids"][perm], obs_image=s["obs_image"][idx], obs_xy=s["obs_xy"][idx],
               track_offsets=np.concatenate([[0], np.cumsum(np.diff(toff)[perm])]).astype(np.uint32))
    return out, idx


def test_same_bytes_across_repeats_shuffles_and_batches(ctx, all_scenes):
    s = all_scenes["edge"]
    base = ctx.filter_points3D(s, passes=15)
    assert same(base, ctx.filter_points3D(s, passes=15))
    for key in ("mean_reprojection_error", "mean_point_error", "min_depth_margin", "min_error_margin", "min_angle_margin"):
        assert getattr(base["report"], key) == getattr(ctx.filter_points3D(s, passes=15)["report"], key)
    P = len(s["xyz"])
    perm = np.random.default_rng(4).permutation(P)
    t, idx = permuted(s, perm)
    got = ctx.filter_points3D(t, passes=15)
    assert np.array_equal(got["point_keep"], base["point_keep"][perm]) and np.array_equal(got["obs_keep"], base["obs_keep"][idx])
    assert np.array_equal(got["point_error"], base["point_error"][perm], equal_nan=True)
    assert np.array_equal(idx[got["kept_obs"]], np.concatenate(
        [base["kept_obs"][base["kept_track_offsets"][p]:base["kept_track_offsets"][p + 1]] for p in perm]))
    assert np.array_equal(got["image_filtered"], base["image_filtered"])
    toff = np.asarray(s["track_offsets"], np.int64)
    lens = np.diff(toff)
    for p in [int(np.argmax(lens)), int(np.nonzero(lens == ref.LANE_CUT)[0][0]), int(np.nonzero(lens == 3)[0][0]), int(np.nonzero(lens == 0)[0][0])]:
        one, idx1 = permuted(s, np.array([p]))  # the point alone against the same point inside the batch
        got = ctx.filter_points3D(one, passes=15)
        assert got["point_keep"][0] == base["point_keep"][p] and np.array_equal(got["obs_keep"], base["obs_keep"][idx1])
        assert np.array_equal(got["point_error"], base["point_error"][[p]], equal_nan=True)


def test_wave_path_and_lane_path_agree(ctx):
    """By construction of two scenes around the cut (point_filter_scenes.around_the_cut): the same tracks after pass 1, on the
    lane path in one scene and on the wave path in the other, give the same bytes."""
    a, b, P = scenes.around_the_cut()
    c = ref.LANE_CUT
    da, db = ctx.filter_points3D(a, passes=15), ctx.filter_points3D(b, passes=15)
    assert da["report"].lane_path_tracks == P and da["report"].wave_path_tracks == 0
    assert db["report"].lane_path_tracks == 0 and db["report"].wave_path_tracks == P
    assert db["report"].num_filtered[0] == P and db["report"].points_deleted[0] == 0
    assert np.array_equal(da["point_keep"], db["point_keep"]) and 0 < da["point_keep"].sum() < P
    assert np.array_equal(da["point_error"], db["point_error"])
    assert np.array_equal(da["obs_keep"].reshape(P, c), db["obs_keep"].reshape(P, c + 1)[:, :c]) and not db["obs_keep"].reshape(P, c + 1)[:, c].any()
    for key in ("mean_reprojection_error", "mean_point_error", "min_error_margin", "min_angle_margin", "pairs_evaluated"):
        assert getattr(da["report"], key) == getattr(db["report"], key), key
    assert list(da["report"].num_filtered)[1:] == list(db["report"].num_filtered)[1:]
    compare(a, da, ref.filter_points3D(a, passes=15), 15)
    compare(b, db, ref.filter_points3D(b, passes=15), 15)


def test_refusals(ctx):
    scenes.check_refusals(ctx)


def test_apply_point_filter_feeds_bundle_adjust(ctx, all_scenes):
    s = all_scenes["obs%d" % ref.SCAN_BLOCK]
    res = ctx.filter_points3D(s, passes=1 | 2 | 4)
    t = capi.Context.apply_point_filter(s, res)
    lens = np.diff(t["track_offsets"].astype(np.int64))
    assert len(t["xyz"]) == res["point_keep"].sum() == len(lens) and (lens >= 2).all() and lens.sum() == res["obs_keep"].sum()
    again = ctx.filter_points3D(t, passes=1 | 2 | 4)  # a fixed point: nothing left to remove
    assert again["point_keep"].all() and again["obs_keep"].all()
    assert np.array_equal(again["point_error"], res["point_error"][res["point_keep"]])
    t["image_constant_pose"] = np.array([1, 1] + [0] * (len(t["image_camera"]) - 2))
    ba = ctx.bundle_adjust(t)
    assert ba["report"].final_cost <= ba["report"].initial_cost


def ba_scene_of(s, tracks, xyz):
    """The dict of bundle_adjust / filter_points3D from tracks {point id: [(image index, point2D index)]} of a re-triangulation scene."""
    off = s["points2D_offsets"]
    pids = sorted(p for p in tracks if len(tracks[p]) >= 2)
    cam = s["cameras"][0]
    return dict(camera_model_ids=[cam.model_id], camera_params=list(cam.params)[:3], camera_width=[cam.width], camera_height=[cam.height],
                image_camera=np.zeros(len(s["image_ids"]), np.uint32), qvec=np.array(s["qvec"], float), tvec=np.array(s["tvec"], float),
                point_ids=np.array(pids, np.uint64), xyz=np.array([xyz[p] for p in pids], float).reshape(-1, 3),
                track_offsets=np.concatenate([[0], np.cumsum([len(tracks[p]) for p in pids])]).astype(np.uint32),
                obs_image=np.array([i for p in pids for i, _ in tracks[p]], np.uint32),
                obs_xy=np.array([s["points2D_xy"][off[i] + k] for p in pids for i, k in tracks[p]], float).reshape(-1, 2)), \
        [(p, i, k) for p in pids for i, k in tracks[p]]


def test_chain_align_merge_filter_retriangulate_filter_bundle_adjust_filter(ctx):
    """dsm_align_clusters -> merge -> filter_points3D(2 | 4) -> dsm_retriangulate -> filter_points3D(1) -> apply_point_filter ->
    dsm_bundle_adjust -> filter_points3D(8), on the planted scene of the chain test of the re-triangulation stage."""
    s, _ = rt.make_scene(n_images=12, n_points=240, track=(2, 6), noise=0.3, wrong=0.0, existing=0.5, seed=21)
    rng = np.random.default_rng(22)
    ids = [int(x) for x in s["image_ids"]]
    off, p3 = s["points2D_offsets"], s["points2D_point3D"]
    windows = [range(0, 7), range(5, 12)]
    planted = [(1.0, np.eye(3), np.zeros(3)), (1.7, rt.look_at_qvec(np.zeros(3), [1.0, 0.5, 2.0], rng)[1], np.array([4.0, -2.0, 1.0]))]
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
                             xyz=sc * (s["point3D_xyz"][order] @ Rc.T) + tc, obs=np.array(obs, np.uint32).reshape(-1, 3), order=order))
    al = ctx.align_clusters([{k: v for k, v in c.items() if k != "order"} for c in clusters])
    seps = [int(x) for x in al["separators"]]
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
            Rw = np.array(rt.pose_matrix(s["qvec"][i], s["tvec"][i])[0]).reshape(3, 4)[:, :3]
            R1 = Rw @ Rc.T
            t1 = sc * np.asarray(s["tvec"][i], float) - R1 @ tc
            R2 = R1 @ R.T
            tvec[i] = S * t1 - R2 @ t
            qvec[i] = rt.rot_to_quat(R2)
    merged.update(point3D_xyz=xyz, qvec=qvec, tvec=tvec)
    # FilterAllPoints3D on the merged reconstruction (distributed_mapper_controller.cpp:758-760)
    tracks = {}
    for i in range(len(ids)):
        for k in range(int(off[i + 1] - off[i])):
            if p3[off[i] + k] >= 0:
                tracks.setdefault(int(s["point3D_ids"][p3[off[i] + k]]), []).append((i, k))
    pos = {int(p): x for p, x in zip(s["point3D_ids"], xyz)}
    before, obs = ba_scene_of(merged, tracks, pos)
    f1 = ctx.filter_points3D(before, passes=2 | 4)
    assert f1["point_keep"].sum() > 0.8 * len(f1["point_keep"])
    new_p3 = np.array(p3, copy=True)
    tracked = {(i, k) for _, i, k in obs}
    for i in range(len(ids)):  # tracks the filter never saw (length 1) go as the reference's pass deletes them
        for k in range(int(off[i + 1] - off[i])):
            if new_p3[off[i] + k] >= 0 and (i, k) not in tracked:
                new_p3[off[i] + k] = -1
    for keep, (_, i, k) in zip(f1["obs_keep"], obs):
        if not keep:
            new_p3[off[i] + k] = -1
    merged["points2D_point3D"] = new_p3
    out = ctx.retriangulate(merged, seps)
    assert out["report"].num_new_points > 0
    tracks = {}
    for i in range(len(ids)):
        for k in range(int(off[i + 1] - off[i])):
            if new_p3[off[i] + k] >= 0:
                tracks.setdefault(int(s["point3D_ids"][new_p3[off[i] + k]]), []).append((i, k))
    for (img, k), pid in zip(out["continued_obs"], out["continued_point_ids"]):
        tracks.setdefault(int(pid), []).append((ids.index(int(img)), int(k)))
    offs = out["new_track_offsets"]
    for kk in range(len(offs) - 1):
        pid = int(out["new_point_ids"][kk])
        pos[pid] = out["new_xyz"][kk]
        tracks[pid] = [(ids.index(int(a)), int(b)) for a, b in out["new_track_obs"][offs[kk]:offs[kk + 1]]]
    scene, _ = ba_scene_of(merged, tracks, pos)
    scene["image_constant_pose"] = np.array([1, 1] + [0] * (len(ids) - 2))
    f2 = ctx.filter_points3D(scene, passes=1)  # the prelude of AdjustGlobalBundle
    solve = capi.Context.apply_point_filter(scene, f2)
    lens = np.diff(solve["track_offsets"].astype(np.int64))
    assert (lens >= 2).all() and solve["obs_image"].max() < len(ids) and len(solve["xyz"]) == len(lens) == len(solve["point_ids"])
    rmse0 = ctx.filter_points3D(solve, passes=8)["report"].mean_reprojection_error
    ba = ctx.bundle_adjust(solve)
    assert ba["report"].termination in (capi.BA_CONVERGENCE, capi.BA_NO_CONVERGENCE)
    after = dict(solve)
    after.update(camera_params=ba["camera_params"], qvec=ba["qvec"], tvec=ba["tvec"], xyz=ba["xyz"])
    rmse1 = ctx.filter_points3D(after, passes=8)["report"].mean_reprojection_error
    assert math.isfinite(rmse0) and math.isfinite(rmse1) and rmse1 < rmse0
