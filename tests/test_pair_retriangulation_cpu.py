"""CPU-only: the numpy restatement of re-triangulating the under-reconstructed pairs (tests/pair_retriangulation_ref.py,
DESIGN.md 19) on hand-built scenes whose answers are worked out here, and the option defaults."""
import numpy as np

from dagsfm_amd import capi
from tests import pair_retriangulation_ref as ref


def three_views(n_points=12, **kw):
    """three images that all see every point, matched pairwise without a wrong match; nothing reconstructed yet"""
    s, _ = ref.make_scene(n_images=3, n_points=n_points, track=(3, 3), noise=0.05, wrong=0.0, seed=3, **kw)
    assert [tuple(int(x) for x in p) for p in s["pairs"]] == [(1, 4), (1, 7), (4, 7)]
    assert list(np.diff(s["match_offsets"])) == [n_points] * 3
    return s


def test_a_pair_is_closed_by_what_earlier_pairs_added():
    """(1, 4) creates a point per correspondence; (1, 7) finds image 1's features on those points and continues image 7's onto
    them; by the turn of (4, 7) both features of each of its correspondences carry the same point: ratio 1, closed, no trial."""
    n = 12
    s = three_views(n)
    out = ref.retriangulate_pairs(s)
    assert out["pair_status"] == [ref.PROCESSED, ref.PROCESSED, ref.CLOSED_BY_ITS_TURN]
    assert out["re_num_trials"] == [1, 1, 0]
    assert out["pair_num_total_corrs"] == [n] * 3 and out["pair_num_tri_corrs"] == [n] * 3
    assert out["counts"] == dict(both=0, continue_tried=n, continue_taken=n, two_view_skipped=0, create_tried=n, create_taken=n)
    assert out["new_point_ids"] == list(range(1, n + 1)) and out["num_tris"] == 3 * n
    assert [[img for img, _ in t] for t in out["new_tracks"]] == [[1, 4]] * n
    assert [t[0][1] for t in out["new_tracks"]] == list(range(n))           # ascending point2D index of image1
    assert all(img == 7 for img, _, _ in out["continued"]) and len(out["touched"]) == 3 * n
    # the same call evaluated once up front would have processed (4, 7) as well: it was open when the call started
    again = ref.retriangulate_pairs(ref.fold(s, out["touched"], out["new_point_ids"], out["new_xyz"]),
                                    re_num_trials=out["re_num_trials"])
    assert again["pair_status"] == [ref.NOT_UNDER_RECONSTRUCTED] * 3 and again["num_tris"] == 0


def test_trial_is_counted_before_the_bogus_test_and_not_for_an_unregistered_image():
    s = three_views()
    bogus = dict(s, cameras=[capi.simple_pinhole(20.0, 320.0, 240.0, 640, 480)])  # focal ratio 20 / 640 < 0.1
    out = ref.retriangulate_pairs(bogus)
    assert out["pair_status"] == [ref.BOGUS_CAMERA] * 3 and out["re_num_trials"] == [1, 1, 1] and out["num_tris"] == 0
    out = ref.retriangulate_pairs(bogus, re_num_trials=out["re_num_trials"])
    assert out["pair_status"] == [ref.TRIALS_EXHAUSTED] * 3 and out["re_num_trials"] == [1, 1, 1]
    unreg = dict(s, registered=np.array([1, 1, 0], np.uint8))
    out = ref.retriangulate_pairs(unreg)
    assert out["pair_status"] == [ref.PROCESSED, ref.UNREGISTERED, ref.UNREGISTERED]
    assert out["re_num_trials"] == [1, 0, 0] and out["num_tris"] == 2 * 12 and not out["continued"]


def test_two_view_tracks_are_skipped_unless_asked_for():
    s, _ = ref.make_scene(n_images=2, n_points=10, track=(2, 2), noise=0.05, wrong=0.0, seed=4)
    out = ref.retriangulate_pairs(s)
    assert out["pair_status"] == [ref.PROCESSED] and out["re_num_trials"] == [1] and out["num_tris"] == 0
    assert out["counts"]["two_view_skipped"] == 10 and out["counts"]["create_tried"] == 0
    out = ref.retriangulate_pairs(s, options=dict(ignore_two_view_tracks=0))
    assert out["counts"]["create_tried"] == 10 and out["counts"]["create_taken"] == 10 and out["num_tris"] == 20
    assert out["pair_num_tri_corrs"] == [10]


def test_a_pair_written_in_the_other_order_gives_the_same_result():
    s, _ = ref.make_scene(n_images=5, n_points=40, track=(3, 5), noise=0.3, wrong=0.1, existing=0.3, seed=8)
    base = ref.retriangulate_pairs(s)
    assert base["counts"]["continue_taken"] > 0 and base["counts"]["create_taken"] > 0
    t = dict(s, pairs=s["pairs"].copy(), matches=s["matches"].copy())
    lo, hi = int(s["match_offsets"][1]), int(s["match_offsets"][2])
    t["pairs"][1] = s["pairs"][1][::-1]
    t["matches"][lo:hi] = s["matches"][lo:hi, ::-1]
    out = ref.retriangulate_pairs(t)
    for key in ("new_point_ids", "new_xyz", "new_tracks", "continued", "touched", "pair_status", "pair_num_total_corrs",
                "pair_num_tri_corrs", "re_num_trials", "num_tris"):
        assert out[key] == base[key], key


def test_ratio_gate_bounds():
    s = three_views()
    assert ref.retriangulate_pairs(s, options=dict(re_min_ratio=0.0))["pair_status"] == [ref.NOT_UNDER_RECONSTRUCTED] * 3
    out = ref.retriangulate_pairs(s, options=dict(re_min_ratio=1.5))
    assert out["pair_status"] == [ref.PROCESSED] * 3 and out["counts"]["both"] == 12


def test_option_defaults_match_reference():
    # the reference: src/sfm/incremental_triangulator.h:65-73
    o = capi.default_pair_retriangulation_options()
    assert (o.re_max_angle_error, o.re_min_ratio, o.re_max_trials) == (5.0, 0.2, 1)
    assert (o.tri.create_max_angle_error, o.tri.continue_max_angle_error, o.tri.min_angle, o.tri.ignore_two_view_tracks) == (2.0, 2.0, 1.5, 1)
    assert ref.RE_DEFAULTS == dict(re_max_angle_error=5.0, re_min_ratio=0.2, re_max_trials=1)
    o = capi.default_pair_retriangulation_options(re_min_ratio=0.5, min_angle=3.0)
    assert o.re_min_ratio == 0.5 and o.tri.min_angle == 3.0
