"""CPU-only: the numpy restatement of re-triangulating the separators (tests/retriangulation_ref.py) -- the
sampler order, the triangulation primitives, the correspondence graph's rules and small hand scenes with known answers."""
import itertools
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import retriangulation_ref as ref


@pytest.mark.parametrize("n", [2, 3, 5, 9, 16])
def test_combination_sampler_is_lexicographic_and_wraps(n):
    expect = list(itertools.combinations(range(n), 2))
    draws = ref.combinations(n, 2 * len(expect) + 3)
    assert draws[:len(expect)] == expect
    assert draws[len(expect):2 * len(expect)] == expect  # the reset after C(n, 2) draws
    assert draws[2 * len(expect):] == (expect * 3)[:3]


def random_pose(rng, center):
    q, R = ref.look_at_qvec(np.asarray(center, float), rng.uniform(-0.5, 0.5, 3), rng, roll=rng.uniform(-1, 1))
    return ref.pose_matrix(q, -R @ np.asarray(center, float))


def project(P, X):
    x = np.array(P).reshape(3, 4) @ np.append(X, 1.0)
    return (x[0] / x[2], x[1] / x[2])


def test_triangulate_point_and_multi_view_recover_planted_points():
    rng = np.random.default_rng(3)
    for _ in range(20):
        X = rng.uniform(-1, 1, 3)
        poses = [random_pose(rng, rng.uniform(-4, 4, 3) + [0, 0, -8]) for _ in range(5)]
        uvs = [project(P, X) for P, _ in poses]
        got = ref.triangulate_point(poses[0][0], poses[1][0], uvs[0], uvs[1])
        assert np.allclose(got, X, rtol=0, atol=1e-9)
        got = ref.triangulate_multi([P for P, _ in poses], uvs)
        assert np.allclose(got, X, rtol=0, atol=1e-9)
        for P, _ in poses:  # the planted point has no angular error in any view (acos near 1: within rounding, or NaN above 1)
            r = ref.residual(project(P, X), P, X)
            assert r < 1e-12 or math.isnan(r)


def tiny_scene(pairs, matches_per_pair, nfeat):
    """images 0..len(nfeat)-1 with ids i + 1, pinhole cameras; pairs in image indices"""
    cam = capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480)
    n = len(nfeat)
    moff = np.concatenate([[0], np.cumsum([len(m) for m in matches_per_pair])]).astype(np.uint64)
    return dict(camera_ids=np.array([1], np.uint32), cameras=[cam], image_ids=np.arange(n, dtype=np.uint32) + 1,
                image_camera_ids=np.ones(n, np.uint32), registered=np.ones(n, np.uint8), qvec=np.tile([1.0, 0, 0, 0], (n, 1)),
                tvec=np.zeros((n, 3)), points2D_offsets=np.concatenate([[0], np.cumsum(nfeat)]).astype(np.uint32),
                points2D_xy=np.zeros((int(sum(nfeat)), 2)), points2D_point3D=np.full(int(sum(nfeat)), -1, np.int32),
                point3D_ids=np.zeros(0, np.uint64), point3D_xyz=np.zeros((0, 3)),
                pairs=np.array(pairs, np.uint32).reshape(-1, 2) + 1, match_offsets=moff,
                matches=np.array([m for ms in matches_per_pair for m in ms], np.uint32).reshape(-1, 2))


def test_duplicate_rule_and_two_view_observation():
    s = tiny_scene([(0, 1), (0, 2), (1, 2)], [[(0, 0), (0, 1), (1, 1), (2, 0)], [(0, 0)], [(3, 3)]], [4, 4, 4])
    g = ref.build_graph(ref.Scene(s))
    # (0,1): (0,0) kept; (0,1) drops (feature 0 of image 0 already matched image 1); (1,1) kept; (2,0) drops (0 of image 1 taken)
    assert g[(0, 0)] == [(1, 0), (2, 0)]
    assert g[(1, 0)] == [(0, 0)]
    assert g[(0, 1)] == [(1, 1)] and g[(1, 1)] == [(0, 1)]
    assert (0, 2) not in g or g[(0, 2)] == []
    assert not ref.is_two_view(g, (0, 0))   # two correspondences
    assert not ref.is_two_view(g, (1, 0))   # its partner has two
    assert ref.is_two_view(g, (0, 1)) and ref.is_two_view(g, (1, 3))


def line_scene(n_views, **kw):
    return ref.make_scene(n_images=n_views, **kw)


def test_two_view_track_is_ignored():
    s, _ = ref.make_scene(n_images=2, n_points=10, track=(2, 2), noise=0.05, wrong=0.0, seed=4)
    out = ref.triangulate(s, [int(s["image_ids"][0])])
    assert out["new_point_ids"] == [] and out["num_tris"] == 0 and len(out["problems"]) > 0
    out = ref.triangulate(s, [int(s["image_ids"][0])], options=dict(ignore_two_view_tracks=0))
    assert len(out["new_point_ids"]) == len(out["problems"])


def test_continue_onto_an_existing_point():
    s, truth = ref.make_scene(n_images=4, n_points=30, track=(4, 4), noise=0.1, wrong=0.0, existing=1.0, seed=5)
    last = int(s["image_ids"][-1])  # every point is in the reconstruction, observed by all images but the last
    out = ref.triangulate(s, [last])
    assert len(out["continued"]) > 0 and out["new_point_ids"] == []
    ids = [int(x) for x in s["point3D_ids"]]
    for sid, k, pid in out["continued"]:
        assert sid == last and pid in ids
        X = s["point3D_xyz"][ids.index(pid)]
        assert np.linalg.norm(X - truth[(sid, k)]) < 0.05


def test_recursive_create_splits_one_list_into_two_points():
    """one feature matched in 6 images: 3 see point A, 3 see point B (wrong matches that agree among themselves)"""
    rng = np.random.default_rng(6)
    s, truth = ref.make_scene(n_images=6, n_points=1, track=(6, 6), noise=0.0, wrong=0.0, seed=6, spacing=2.0)
    A = truth[(int(s["image_ids"][0]), 0)]
    B = A + np.array([3.0, 2.0, 0.0])
    for i in (3, 4, 5):  # images 3..5 observe B at their only feature
        P, _ = ref.pose_matrix(s["qvec"][i], s["tvec"][i])
        u, v = project(P, B)
        s["points2D_xy"][i] = [500.0 * u + 320.0, 500.0 * v + 240.0]
    del rng
    out = ref.triangulate(s, [int(s["image_ids"][0])])
    assert len(out["new_point_ids"]) == 2
    tracks = sorted(sorted(t) for t in out["new_tracks"])
    ids = [int(x) for x in s["image_ids"]]
    assert tracks == [sorted((ids[i], 0) for i in (0, 1, 2)), sorted((ids[i], 0) for i in (3, 4, 5))]
    xyz = sorted(out["new_xyz"], key=lambda X: X[0])
    assert np.allclose(xyz[0], A, atol=0.05) and np.allclose(xyz[1], B, atol=0.05)
    assert out["new_point_ids"] == [out["new_point_ids"][0], out["new_point_ids"][0] + 1]


def test_bogus_camera_and_unregistered_image_are_skipped():
    s, _ = ref.make_scene(n_images=5, n_points=40, track=(5, 5), noise=0.1, wrong=0.0, seed=7, unregistered=(4,))
    sep = int(s["image_ids"][0])
    base = ref.triangulate(s, [sep])
    assert all(t[0] != int(s["image_ids"][4]) for tr in base["new_tracks"] for t in tr)  # the unregistered image never joins
    assert ref.triangulate(s, [int(s["image_ids"][4])])["num_tris"] == 0             # nor runs as a separator
    bogus = capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)                       # focal ratio 20 / 640 < 0.1
    s2 = dict(s, cameras=[bogus])
    out = ref.triangulate(s2, [sep])
    assert out["num_tris"] == 0 and out["problems"] == {}
    assert abs(out["bogus_margin"] - abs(20.0 / 640 - 0.1) / 0.1) < 1e-15


def test_num_trials_table():
    assert ref.num_trials(10, 10, 0.9999) == 1
    assert ref.num_trials(0, 10, 0.9999) == 2 ** 32 - 1
    # ceil(log(1e-4) / log(1 - r^2)): r = 0.9 -> 5.55 -> 6, r = 0.5 -> 32.0 -> 33, r = 0.2 -> 225.0 -> 226
    assert ref.num_trials(9, 10, 0.9999) == 6
    assert ref.num_trials(5, 10, 0.9999) == 33
    assert ref.num_trials(2, 10, 0.9999) == 226
    assert ref.num_trials(1, 2, 0.9999) == 33


def test_nan_residual_is_a_zero_margin():
    """a cosine that rounds to 1 or above (acos NaN: an outlier in the reference) is a decision rounding can flip"""
    P = [1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0]
    r, d = ref.residual_cos((0.0, 0.0), P, [0.0, 0.0, 5.0])
    assert d == 1.0 and r == 0.0 and not d <= ref.COSINE_EDGE
    views = [(P, [0, 0, 0], (0.0, 0.0)), ([1.0, 0, 0, -1.0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], [1.0, 0, 0], (-0.2, 0.0))]
    mg, rec = ref.Margins(), ref.Problem()
    ref.loransac(views, ref.default_options(), mg, rec)
    assert mg.residual == 0.0
