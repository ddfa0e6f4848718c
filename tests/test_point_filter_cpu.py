"""CPU-only: the restatement of the point filters (tests/point_filter_ref.py) against the reference's known answers, the closed
form of the negative-depth pass against the sequential walk, the conditions the GPU scenes must meet and the constant
behind the error tolerance.  The refusals need a context, which needs a device: the GPU file asserts them."""
import itertools
import math

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import point_filter_ref as ref
from tests import point_filter_scenes as scenes
from tests.point_filter_scenes import ERROR_SENSITIVITY, P3, P4, unit_scene

def count(scene, **kw):
    return int(ref.filter_points3D(scene, **kw)["point_keep"].sum())


RANDOM_XYZ = [0.3, -0.7, 0.6]  # Eigen::Vector3d::Random() in the reference's tests: any point does


def test_known_answers_filter_points3D():
    """TestFilterPoints3D (reconstruction_test.cc:315-356): FilterPoints3D = passes 2 | 4 over the named points."""
    f = dict(passes=ref.REPROJ | ref.TRI_ANGLE)
    s = unit_scene(2, [(RANDOM_XYZ, [])])
    assert count(s, point_selected=[0], max_reproj_error=0.0, min_tri_angle=0.0, **f) == 1  # not named: stays
    assert count(s, point_selected=[1], max_reproj_error=0.0, min_tri_angle=0.0, **f) == 0  # named: a track of length 0 goes
    assert count(unit_scene(2, [(RANDOM_XYZ, [0])]), point_selected=[1], max_reproj_error=0.0, min_tri_angle=0.0, **f) == 0
    s = unit_scene(2, [P3])
    assert count(s, point_selected=[1], max_reproj_error=0.0, min_tri_angle=0.0, **f) == 1  # e = 0 is not > 0; angle 0 >= 0
    assert count(s, point_selected=[1], max_reproj_error=0.0, min_tri_angle=1e-3, **f) == 0
    s = unit_scene(2, [P4])
    assert count(s, point_selected=[1], max_reproj_error=0.1, min_tri_angle=0.0, **f) == 1
    assert count(s, point_selected=[1], max_reproj_error=0.09, min_tri_angle=0.0, **f) == 0


def test_known_answers_filter_points3D_in_images():
    """TestFilterPoints3DInImages (:358-398): the points seen in the named images."""
    f = dict(passes=ref.REPROJ | ref.TRI_ANGLE, max_reproj_error=0.0)
    s = unit_scene(2, [(RANDOM_XYZ, [])])
    assert count(s, image_selected=[0, 0], min_tri_angle=0.0, **f) == 1
    assert count(s, image_selected=[1, 0], min_tri_angle=0.0, **f) == 1  # no observation: not in the image
    s = unit_scene(2, [(RANDOM_XYZ, [0])])
    assert count(s, image_selected=[0, 1], min_tri_angle=0.0, **f) == 1
    assert count(s, image_selected=[1, 0], min_tri_angle=0.0, **f) == 0
    s = unit_scene(2, [P3])
    assert count(s, image_selected=[1, 0], min_tri_angle=0.0, **f) == 1
    assert count(s, image_selected=[1, 0], min_tri_angle=1e-3, **f) == 0
    s = unit_scene(2, [P4])
    assert count(s, image_selected=[1, 0], passes=6, max_reproj_error=0.1, min_tri_angle=0.0) == 1
    assert count(s, image_selected=[1, 0], passes=6, max_reproj_error=0.09, min_tri_angle=0.0) == 0


def test_known_answers_filter_all_points():
    """TestFilterAllPoints (:400-429)."""
    assert count(unit_scene(2, [(RANDOM_XYZ, [])]), max_reproj_error=0.0, min_tri_angle=0.0) == 0
    assert count(unit_scene(2, [(RANDOM_XYZ, [0])]), max_reproj_error=0.0, min_tri_angle=0.0) == 0
    assert count(unit_scene(2, [P3]), max_reproj_error=0.0, min_tri_angle=0.0) == 1
    assert count(unit_scene(2, [P3]), max_reproj_error=0.0, min_tri_angle=1e-3) == 0
    assert count(unit_scene(2, [P4]), max_reproj_error=0.1, min_tri_angle=0.0) == 1
    assert count(unit_scene(2, [P4]), max_reproj_error=0.09, min_tri_angle=0.0) == 0


def test_known_answers_negative_depth():
    """TestFilterObservationsWithNegativeDepth (:431-453): a point without observations is never visited; one observation at
    depth 0.001 stays, at depth 0 its point goes."""
    for z in (1.0, 0.001, 0.0):
        assert count(unit_scene(2, [([0, 0, z], [])]), passes=ref.NEG_DEPTH) == 1
    assert count(unit_scene(2, [([0, 0, 0.001], [0])]), passes=ref.NEG_DEPTH) == 1
    out = ref.filter_points3D(unit_scene(2, [([0, 0, 0.0], [0])]), passes=ref.NEG_DEPTH)
    assert out["point_keep"].sum() == 0 and out["num_filtered"][0] == 1


def test_known_answers_filter_images():
    """TestFilterImages (:455-471): four registered images, one point seen by three, then by two; then the focal-length ratio."""
    opts = dict(passes=ref.MEAN_ERROR, min_focal_length_ratio=0.0, max_focal_length_ratio=10.0, max_extra_param=1.0)
    assert ref.filter_points3D(unit_scene(4, [(RANDOM_XYZ, [0, 1, 2])]), **opts)["image_filtered"].tolist() == [False, False, False, True]
    assert ref.filter_points3D(unit_scene(4, [(RANDOM_XYZ, [0, 1])]), **opts)["image_filtered"].sum() == 2
    opts["max_focal_length_ratio"] = 0.9  # f / max(w, h) = 1 > 0.9: every image goes
    assert ref.filter_points3D(unit_scene(4, [(RANDOM_XYZ, [0, 1])]), **opts)["image_filtered"].all()


def test_known_answers_mean_reprojection_error():
    """TestComputeMeanReprojectionError (:520-534) asserts the argument-free overload: 0 without points or errors, else the
    mean of the errors that are set.  Here: no pass sets one -> 0; pass 8 sets them."""
    assert ref.filter_points3D(unit_scene(2, []), passes=ref.MEAN_ERROR)["mean_point_error"] == 0
    assert ref.filter_points3D(unit_scene(2, [P3]), passes=ref.NEG_DEPTH)["mean_point_error"] == 0
    s = unit_scene(2, [([0.5, -0.5, 1.0], [0, 1]), ([-0.5, 2.5, 1.0], [0, 1])])  # errors 1 and 3 in both views
    out = ref.filter_points3D(s, passes=ref.MEAN_ERROR)
    assert out["point_error"].tolist() == [1.0, 3.0] and out["mean_point_error"] == 2.0 and out["mean_reprojection_error"] == 2.0
    assert math.isnan(ref.filter_points3D(s, passes=ref.MEAN_ERROR, point_selected=[0, 0])["mean_reprojection_error"])  # 0 / 0
    out = ref.filter_points3D(unit_scene(2, [([0.5, -0.5, 1.0], [0]), ([0.0, 0.0, -1.0], [0, 1])]), passes=ref.MEAN_ERROR)
    assert out["point_error"].tolist() == [1.0, 0.0] and out["mean_reprojection_error"] == 1.0 / 3.0  # behind: skipped, still counted in L


def test_closed_form_of_negative_depth_matches_the_walk_exhaustively():
    """Every (L, set of negatives) for L <= 6, the observations dealt to the images in two different orders."""
    for L in range(0, 7):
        for negs in itertools.product([False, True], repeat=L):
            for order in (list(range(L)), list(range(L))[::-1]):
                toff = np.array([0, L])
                tracks, nf = ref.walk_negative_depth(toff, np.array(order, np.int64), np.array(negs, bool), max(L, 1))
                alive, count_ = ref.closed_form_negative_depth(L, sum(negs))
                assert (tracks[0] is not None) == alive and nf[0] == count_, (L, negs)
                if alive:
                    assert tracks[0] == [i for i in range(L) if not negs[i]]


def test_closed_form_of_negative_depth_matches_the_walk_on_random_tracks():
    rng = np.random.default_rng(3)
    for _ in range(20):
        P, N = 60, 9
        lens = rng.integers(0, N + 1, P)
        toff = np.concatenate([[0], np.cumsum(lens)])
        oimg = np.concatenate([rng.permutation(N)[:L] for L in lens]).astype(np.int64)
        neg = rng.random(len(oimg)) < rng.choice([0.1, 0.5, 0.9])
        tracks, nf = ref.walk_negative_depth(toff, oimg, neg, N)
        for p in range(P):
            n = int(neg[toff[p]:toff[p + 1]].sum())
            alive, c = ref.closed_form_negative_depth(int(lens[p]), n)
            assert (tracks[p] is not None) == alive and nf[p] == c
            if alive:
                assert tracks[p] == [o for o in range(toff[p], toff[p + 1]) if not neg[o]]


def test_point_error_divides_by_the_kept_count():
    """Three views with errors 1, 3 and 10 against a threshold of 4: the third goes, the error is (1 + 3) / 2, not / 3."""
    s = unit_scene(3, [([0.5, -0.5, 1.0], [0, 1, 2])])
    s["obs_xy"] = np.array([[0.0, 0.0], [1.0, 3.0], [1.0, 10.0]])
    out = ref.filter_points3D(s, passes=ref.REPROJ, max_reproj_error=4.0)
    assert out["obs_keep"].tolist() == [True, True, False] and out["point_error"][0] == 2.0 and out["num_filtered"][1] == 1
    out = ref.filter_points3D(s, passes=ref.REPROJ, max_reproj_error=2.0)  # two of three marked: >= L - 1, the point goes with L counted
    assert not out["point_keep"][0] and out["num_filtered"][1] == 3 and out["point_error"][0] == -1.0


def test_nan_pair_is_not_a_sufficient_angle():
    """Two centres and a point on one line: the ratio of the law of cosines rounds above 1 for some offsets, acos is NaN,
    std::min(NaN, pi - NaN) is NaN and NaN >= threshold is false -- the exact angle is 0, the same side."""
    found = 0
    for k in range(1, 400):
        c1, c2, X = np.array([[0.1 * k, 0.3, 0.7]]), np.array([[0.1 * k + 1.0 / 3.0, 0.3, 0.7]]), np.array([[17.3 + k / 7.0, 0.3, 0.7]])
        a = ref.tri_angles(c1, c2, X)[0]
        if math.isnan(a):
            found += 1
            assert not (a >= 0.0) and ref.margin(a, 0.026) == math.inf
        else:
            assert a < 1e-6
    assert found > 0
    assert ref.tri_angles(np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)))[0] == 0.0  # denominator 0: angle 0


def test_option_defaults_match_reference():
    """IncrementalMapper::Options (src/sfm/incremental_mapper.h:96-108) = DistributedMapperController::Options'."""
    o = capi.default_point_filter_options()
    assert (o.max_reproj_error, o.min_tri_angle, o.min_focal_length_ratio, o.max_focal_length_ratio, o.max_extra_param) == \
        (4.0, 1.5, 0.1, 10.0, 1.0)
    assert o.passes == capi.FILTER_REPROJECTION_ERROR | capi.FILTER_TRIANGULATION_ANGLE
    assert ref.default_options() == {k: getattr(o, k) for k in ref.default_options()}
    assert (ref.NEG_DEPTH, ref.REPROJ, ref.TRI_ANGLE, ref.MEAN_ERROR) == \
        (capi.FILTER_NEGATIVE_DEPTH, capi.FILTER_REPROJECTION_ERROR, capi.FILTER_TRIANGULATION_ANGLE, capi.FILTER_MEAN_ERROR)


@pytest.fixture(scope="module")
def all_scenes():
    return scenes.scenes()


def test_scenes_meet_the_cap_on_unclear_points(all_scenes):
    """At most 1 % of a scene's points may have a margin below 1e-9 -- a condition on the scene, asserted here on the
    restatement alone, so that a scene that cannot meet it never reaches a device.  Every scene must also exercise what it is
    for: deletions in every pass, both paths."""
    for name, s, passes, kw in scenes.comparisons():  # the same (scene, passes, selection) set as the GPU file's
        exp = ref.filter_points3D(s, passes=passes, **kw)
        unclear = int((~ref.clear_points(exp)).sum())
        assert unclear <= 0.01 * len(exp["point_keep"]), (name, passes, sorted(kw), unclear)
    a, b, _ = scenes.around_the_cut()
    for name, s in list(all_scenes.items()) + [("cut_a", a), ("cut_b", b)]:
        exp = ref.filter_points3D(s, passes=15)
        if name != "cut_a":
            assert exp["points_deleted"][0] > 0 or name == "cut_b", name
            assert exp["observations_deleted"][0] > exp["points_deleted"][0] or name.startswith("obs"), name
        assert (exp["points_deleted"][1] > 0 or name.startswith("cut")) and exp["points_deleted"][2] > 0, name
        assert exp["observations_deleted"][1] > exp["points_deleted"][1], name
        assert 0 < exp["point_keep"].sum() < len(exp["point_keep"])
    lens = np.diff(all_scenes["edge"]["track_offsets"].astype(np.int64))
    assert {0, 1, 2, 3, ref.LANE_CUT - 1, ref.LANE_CUT, ref.LANE_CUT + 1, 300} <= set(lens.tolist())
    assert all(len(s["obs_image"]) % 64 for n, s in all_scenes.items() if n in ("edge", "models"))


def test_error_sensitivity_constant(all_scenes):
    """Re-measures the constant the error tolerance is built from (point_filter_scenes.ERROR_SENSITIVITY): every scene the GPU
    file compares, every pass mask that sets errors."""
    a, b, _ = scenes.around_the_cut()
    worst = 0.0
    for name, s in list(all_scenes.items()) + [("cut_a", a), ("cut_b", b)]:
        for passes in scenes.ERROR_SENSITIVITY_PASSES:
            worst = max(worst, ref.error_sensitivity(s, seeds=(1, 2, 3), passes=passes))
    print("measured error sensitivity: %.3g" % worst)
    assert 0 < worst <= ERROR_SENSITIVITY
