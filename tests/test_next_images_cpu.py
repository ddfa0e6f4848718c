"""dsm_find_next_images without a GPU: the restatement (tests/next_images_ref.py) against the expectations of the
reference's own pyramid test and against itself -- the reference's incremental bookkeeping against the stateless definition --
and the host build of csrc/next_images.h (libdsm_next_images_host.so: the text the kernels are built from) against the
restatement, bit for bit, on every scene of tests/next_images_scenes.py."""
import copy
import ctypes
import json
import os

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import next_images_ref as ref
from tests import next_images_scenes as scenes

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "visibility_pyramid_scores.json")


def same(got, exp):
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g["next_image_ids"] == e["next_image_ids"]
        for key in ("num_visible", "num_observations", "score"):
            assert [int(x) for x in g[key]] == [int(x) for x in e[key]], key


def test_binding_and_switch_exist():
    assert hasattr(capi.Context, "find_next_images") and "DSM_NEXT_IMAGES_SERIAL" in capi.CHECK_OPTION_KEYS
    o = capi.NextImagesOptions()
    capi.next_images_host_lib().dsm_ni_host_default_options(ctypes.byref(o))
    assert (o.image_selection_method, o.abs_pose_min_num_inliers, o.max_reg_trials) == (2, 30, 3)  # incremental_mapper.h:87-131
    d = ref.default_options()
    assert (d["image_selection_method"], d["abs_pose_min_num_inliers"], d["max_reg_trials"]) == (2, 30, 3)


def test_pyramid_reproduces_the_reference_tests_expectations():
    """visibility_pyramid_test.cc's TestScore: the score after each SetPoint / ResetPoint on a 4 x 4 image, for 1 .. 7 levels;
    for six levels the host build's score of the occupancy (the points set and not yet reset) is the same number."""
    L = capi.next_images_host_lib()
    cases = json.load(open(GOLDEN))["cases"]
    assert sorted(c["num_levels"] for c in cases) == list(range(1, 8))
    for c in cases:
        pyr = ref.VisibilityPyramid(c["num_levels"], c["width"], c["height"])
        assert pyr.score == 0 and pyr.max_score == c["max_score"]
        live = []
        for st in c["steps"]:
            if st["op"] == "set":
                pyr.set_point(st["x"], st["y"])
                live.append((st["x"], st["y"]))
            else:
                pyr.reset_point(st["x"], st["y"])
                live.remove((st["x"], st["y"]))
            if st["score"] is not None:
                assert pyr.score == st["score"]
            if c["num_levels"] == ref.NUM_LEVELS:
                xy = np.array(live, np.float64).reshape(-1, 2)
                assert L.dsm_ni_host_score(xy.ctypes.data, len(xy), c["width"], c["height"]) == pyr.score


def test_cell_and_rank_pieces():
    L = capi.next_images_host_lib()
    pyr = ref.VisibilityPyramid(6, 1000, 333)
    xs = [0.0, 1000 / 64, np.nextafter(1000 / 64, 0), 999.999, 1000.0, 1000.5, 1e300, 1.7e308, 5e-324, 333 * 63 / 64, 15.625 * 63]
    for x in xs:
        cx, cy = pyr.cell_for_point(x, x)
        assert L.dsm_ni_host_cell(x, 1000) == cx and L.dsm_ni_host_cell(x, 333) == cy
    full = np.stack(np.meshgrid(np.arange(64) + 0.5, np.arange(64) + 0.5), -1).reshape(-1, 2)
    assert L.dsm_ni_host_score(full.ctypes.data, len(full), 64, 64) == 17895696 == ref.VisibilityPyramid(6, 64, 64).max_score
    assert L.dsm_ni_host_score(full.ctypes.data, 1, 64, 64) == 4 + 16 + 64 + 256 + 1024 + 4096
    # the ratio is the one rank that rounds: float / float in float
    for nv, no in ((1, 3), (10, 30), (262144, 262143), (7, 9), (30, 31)):
        assert L.dsm_ni_host_rank(1, nv, no, 0) == np.float32(nv) / np.float32(no)
    assert L.dsm_ni_host_rank(0, 262144, 1, 0) == 262144.0 and L.dsm_ni_host_rank(2, 0, 0, 17895696) == 17895696.0
    # the key orders as (bucket, rank descending, id ascending)
    key = lambda second, rank, i: L.dsm_ni_host_key(2 if second else 0, 1, rank, i)
    assert key(0, 5.0, 9) < key(0, 4.5, 1) < key(0, 4.5, 2) < key(1, 1e9, 0) < key(1, 0.25, 0xFFFFFFFE) < L.dsm_ni_host_key(0, 0, 9.0, 1)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_incremental_bookkeeping_equals_the_stateless_definition(seed):
    """Random sequences of registrations, added and removed observations: after every step the reference's counters and
    pyramids equal the stateless definition of the same state, and so does FindNextImages over them."""
    rng = np.random.default_rng(seed)
    s, problems, kw = scenes.random_case(200 + seed, n_images=7, n_problems=2)
    for pr in problems:
        pr = copy.deepcopy(pr)
        ids = pr["image_ids"]
        pr["registered"] = [0] * len(ids)
        pr["obs_point3D"] = [np.full(len(a), -1, np.int32) for a in pr["obs_point3D"]]
        recon = ref.Reconstruction(s, pr)
        for step in range(60):
            k = int(rng.integers(0, len(ids)))
            i, n = ids[k], len(pr["obs_point3D"][k])
            if not pr["registered"][k]:
                if rng.random() < 0.3:
                    pr["registered"][k] = 1
                    recon.register(i)
                continue
            if n == 0:
                continue
            f = int(rng.integers(0, n))
            if pr["obs_point3D"][k][f] >= 0:
                recon.delete_observation(i, f)
                pr["obs_point3D"][k][f] = -1
            else:
                recon.add_observation(i, f, int(rng.integers(0, 9)))
                pr["obs_point3D"][k][f] = recon.point3D[(i, f)]
            if step % 3:
                continue
            for kk, (nv, no, score) in enumerate(ref.stateless(s, pr)):
                im = recon.images[ids[kk]]
                assert (im.num_visible_points3D, im.num_observations) == (nv, no)
                if not pr["registered"][kk]:
                    assert im.pyramid.score == score
            o = ref.default_options(**kw)
            assert ref.find_next_images_from(recon, pr, o) == ref.find_next_images(s, [pr], **kw)[0]["next_image_ids"]


CASES = [(n, m) for n in scenes.NAMES for m in (scenes.METHODS if n in ("ranks", "many_slots", "shared_images") else (None,))]


@pytest.mark.parametrize("name,method", CASES)
@pytest.mark.parametrize("sorted_schedule", [False, True])
def test_host_build_equals_the_restatement(name, method, sorted_schedule):
    s, problems, kw = scenes.get(name)
    kw = dict(kw) if method is None else dict(kw, image_selection_method=method)
    exp = ref.find_next_images(s, problems, **kw)
    same(capi.next_images_host(s, problems, sorted_schedule=sorted_schedule, **kw), exp)


def test_scenes_hold_what_they_are_for():
    """The properties the scenes were built for, under the restatement, so that no case silently tests nothing."""
    r = lambda name, **kw: ref.find_next_images(scenes.get(name)[0], scenes.get(name)[1], **dict(scenes.get(name)[2], **kw))
    e = r("word_edges")[0]
    assert [int(x) for x in e["num_visible"]] == [0, 0, 1, 31, 32, 33, 63, 64, 65, 257] and e["next_image_ids"][0] == 9 and 1 not in e["next_image_ids"]
    e = r("full_and_single")[0]
    assert [int(x) for x in e["score"]] == [0, 17895696, 5460] and e["next_image_ids"] == [1, 2]
    e = r("duplicates")[0]
    assert [int(x) for x in e["num_visible"]] == [0, 0, 3] and [int(x) for x in e["num_observations"]] == [2, 2, 4]
    e = r("no_point_correspondences")[0]
    assert int(e["num_visible"][2]) == 3 and int(e["num_observations"][2]) == 6 and int(e["num_visible"][3]) == 0 and e["next_image_ids"] == [1]
    a, b, c = r("shared_images")
    assert a["next_image_ids"] != b["next_image_ids"] and set(a["next_image_ids"]) <= {11, 12, 13} and set(b["next_image_ids"]) <= {10, 11}
    by = [r("ranks", image_selection_method=m)[0]["next_image_ids"] for m in scenes.METHODS]
    assert by[0] == [4, 1, 2, 3, 5, 6, 7] and by[1] == [1, 3, 5, 2, 4, 6, 7] and by[2] == [1, 2, 3, 5, 4, 6, 7]
    assert all(x[-2:] == [6, 7] for x in by)  # the second bucket: tried before, filtered before; equal ranks in id order
    assert r("boundaries")[0]["next_image_ids"] == [5, 1, 4]  # 2 sees one point too few, 3 has no trial left, 4 has one left
    e = r("nothing_eligible")
    assert [x["next_image_ids"] for x in e] == [[], [2], [], [], []]
    e = r("many_slots")[0]
    assert len(e["num_visible"]) == 300 and len(e["next_image_ids"]) > 256


def invalid_cases():
    """(name, a function that breaks a deep copy of (scene, problems, kw)).  All of these need no device to be refused."""
    def neg(s, p, kw):
        k = list(s["image_ids"]).index(1)
        s["points2D_xy"][int(s["points2D_offsets"][k])] = [-0.5, 3.0]

    def point_on_unregistered(s, p, kw):
        p[0]["obs_point3D"][p[0]["image_ids"].index(1)][0] = 4

    def set_(key, value):
        return lambda s, p, kw: kw.__setitem__(key, value)

    def below(s, p, kw):
        p[0]["obs_point3D"][0][0] = -2

    def offsets(s, p, kw):
        total = sum(len(a) for a in p[0]["obs_point3D"])
        p[0]["obs_offsets"] = [0] + [1] * (len(p[0]["image_ids"]) - 1) + [total]

    def registered2(s, p, kw):
        p[0]["registered"][0] = 2

    def nonfinite(s, p, kw):
        s["points2D_xy"][0] = [np.nan, 1.0]

    def no_size(s, p, kw):
        s["cameras"] = [capi.simple_pinhole(500.0, 1.0, 1.0, 0, 480, True)]

    def unknown_image(s, p, kw):
        p[0]["image_ids"][1] = 77

    def repeated(s, p, kw):
        p[0]["image_ids"][2] = p[0]["image_ids"][1]
        p[0]["obs_point3D"][2] = p[0]["obs_point3D"][1].copy()
        p[0]["registered"][2] = p[0]["registered"][1]

    def match_range(s, p, kw):
        s["matches"][0] = [0, 99]

    return [("negative xy on a candidate", neg), ("a point on an unregistered slot", point_on_unregistered), ("method 3", set_("image_selection_method", 3)),
            ("method -1", set_("image_selection_method", -1)), ("min inliers 0", set_("abs_pose_min_num_inliers", 0)),
            ("max_reg_trials 0", set_("max_reg_trials", 0)), ("a point index of -2", below), ("obs offsets", offsets), ("registered 2", registered2),
            ("non-finite xy", nonfinite), ("a camera without width", no_size), ("an unknown image", unknown_image), ("a repeated image", repeated),
            ("a match out of range", match_range)]


def broken(fn):
    s, problems, kw = copy.deepcopy(scenes.get("duplicates"))
    fn(s, problems, kw)
    return s, problems, kw


@pytest.mark.parametrize("label,fn", invalid_cases(), ids=[c[0] for c in invalid_cases()])
def test_host_build_refuses_invalid_arguments_and_leaves_the_outputs_untouched(label, fn):
    s, problems, kw = broken(fn)
    with pytest.raises(capi.DsmError) as e:
        capi.next_images_host(s, problems, **kw)
    assert e.value.code == 1  # DSM_ERR_INVALID_ARGUMENT
    assert all(not np.asarray(a).any() for a in e.value.outputs)


def test_a_negative_coordinate_on_a_registered_image_is_accepted():
    s, problems, kw = copy.deepcopy(scenes.get("duplicates"))
    s["points2D_xy"][0] = [-5.0, -7.0]  # image 100: registered, its pyramid is not evaluated
    same(capi.next_images_host(s, problems, **kw), ref.find_next_images(s, problems, **kw))


def test_too_small_a_capacity_is_out_of_range():
    s, problems, kw = scenes.get("ranks")
    with pytest.raises(capi.DsmError) as e:
        capi.next_images_host(s, problems, capacity=6, **kw)
    assert e.value.code == 4 and all(not np.asarray(a).any() for a in e.value.outputs)
    same(capi.next_images_host(s, problems, capacity=7, **kw), ref.find_next_images(s, problems, **kw))


# ================================================================== dsm_find_local_bundles
def same_bundles(got, exp):
    """Everything for equality: the lists and counts exactly, tri_angle bit for bit."""
    assert len(got) == len(exp)
    for g, e in zip(got, exp):
        assert g["bundle_image_ids"] == e["bundle_image_ids"]
        assert g["overlap_image_ids"] == e["overlap_image_ids"] and g["overlap_shared"] == e["overlap_shared"]
        assert np.asarray(g["overlap_tri_angle"], np.float64).tobytes() == np.asarray(e["overlap_tri_angle"], np.float64).tobytes()


_lb_expected = {}


def lb_expected(name):
    """The restatement's results of a named scene (and its smallest margin), computed once and left unchanged."""
    if name not in _lb_expected:
        s, problems, queries, kw = scenes.lb_get(name)
        _lb_expected[name] = ref.find_local_bundles(problems, queries, **kw)
    return _lb_expected[name]


def test_local_bundle_binding_and_defaults():
    assert hasattr(capi.Context, "find_local_bundles")
    o = capi.LocalBundleSelectionOptions()
    capi.next_images_host_lib().dsm_lb_host_default_options(ctypes.byref(o))
    assert (o.local_ba_num_images, o.local_ba_min_tri_angle) == (6, 6.0)  # incremental_mapper.h:98-102
    d = ref.default_local_bundle_options()
    assert (d["local_ba_num_images"], d["local_ba_min_tri_angle"]) == (6, 6.0)


def test_percentile_index_and_select():
    L = capi.next_images_host_lib()
    for n in list(range(1, 70)) + [257, 1000, 262144]:
        x = 0.75 * (n - 1)
        want = int(np.floor(x + 0.5))  # std::round: halves away from zero
        assert L.dsm_lb_host_percentile_index(n) == max(0, min(n - 1, want))
    assert [L.dsm_lb_host_percentile_index(n) for n in (1, 2, 3, 4, 7)] == [0, 1, 2, 2, 5]  # 0.75, 1.5 and 4.5 round up
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 4, 5, 63, 64, 65, 257):
        a = rng.uniform(0, 1.5, n)
        a[rng.integers(0, n, n // 3)] = a[0]  # ties
        assert L.dsm_lb_host_percentile(a.ctypes.data, n) == ref.percentile(list(a), 75)
    a = np.array([0.5, np.nan, 0.25, 0.75])  # a NaN orders behind every number
    assert L.dsm_lb_host_percentile(a.ctypes.data, 4) == 0.75 == ref.percentile(list(a), 75)


@pytest.mark.parametrize("name", scenes.LB_NAMES)
def test_local_bundle_host_build_equals_the_restatement(name):
    s, problems, queries, kw = scenes.lb_get(name)
    exp, margin = lb_expected(name)
    got, got_margin = capi.local_bundles_host(s, problems, queries, **kw)
    same_bundles(got, exp)
    assert got_margin == margin


@pytest.mark.parametrize("name", scenes.LB_NAMES)
def test_local_bundle_scenes_keep_their_margins(name):
    """A condition on the inputs: no tri_angle of a scene sits within 1e-9 (relative) of a threshold it is compared with, so
    the GPU tests can ask for equality."""
    assert lb_expected(name)[1] >= 1e-9


def test_local_bundle_scenes_hold_what_they_are_for():
    e = lb_expected("copy_and_chain")[0]
    assert e[0]["accepted_at"] == [] and len(e[0]["overlap_image_ids"]) == 5 and all(a == -1.0 for a in e[0]["overlap_tri_angle"])
    assert len(e[1]["overlap_image_ids"]) == 6 and e[1]["accepted_at"] and len(e[1]["bundle_image_ids"]) == 5
    assert lb_expected("thresholds")[0][0]["accepted_at"] == [0, 1, 4, 7, 8]
    t = lb_expected("thresholds")[0][0]
    assert t["overlap_tri_angle"][-1] == -1.0 and t["overlap_shared"][-1] == 3  # below the loosest threshold: never reached
    a, b = lb_expected("overlap_edge")[0]
    assert (a["overlap_shared"][1], b["overlap_shared"][1]) == (12, 11) and 0.6 * 20 == 12.0
    assert a["bundle_image_ids"] == [16, 13] and a["accepted_at"] == [0, 2] and b["bundle_image_ids"] == [43, 46] and b["accepted_at"] == [2, 2]
    assert [x["num_points3D"] for x in lb_expected("sizes")[0]] == [1, 2, 3, 4, 64, 65, 257]
    d = lb_expected("degenerate")[0]
    assert d[0]["num_points3D"] == 14 and d[0]["overlap_shared"][d[0]["overlap_image_ids"].index(13)] == 14  # the repeats count twice
    assert d[0]["overlap_tri_angle"][d[0]["overlap_image_ids"].index(13)] == 0.0  # the twin's centre is the query's
    assert d[2]["overlap_shared"][d[2]["overlap_image_ids"].index(10)] == 14 and 25 not in d[0]["overlap_image_ids"]
    assert len(lb_expected("options")[0][0]["bundle_image_ids"]) == 1 and lb_expected("zero_angle")[0][0]["accepted_at"] == [0] * 5
    q = lb_expected("queries")[0]
    assert q[2]["bundle_image_ids"] == [] and q[0]["bundle_image_ids"] != q[2]["bundle_image_ids"] and q[3] != q[4]


def lb_invalid_cases():
    def set_(key, value):
        return lambda s, p, q, kw: kw.__setitem__(key, value)

    def point_range(s, p, q, kw):
        p[0]["obs_point3D"][0][np.argmax(p[0]["obs_point3D"][0] >= 0)] = len(p[0]["point_xyz"])

    def unregistered_query(s, p, q, kw):
        q[0] = (0, 25)

    def unregistered_point(s, p, q, kw):
        p[0]["obs_point3D"][5][0] = 1

    def outside(s, p, q, kw):
        q[0] = (0, 9999)

    def problem_range(s, p, q, kw):
        q[0] = (7, 10)

    def pose(s, p, q, kw):
        p[0]["tvec"][2][1] = np.inf

    def point(s, p, q, kw):
        p[0]["point_xyz"][3][0] = np.nan

    def offsets(s, p, q, kw):
        total = sum(len(a) for a in p[0]["obs_point3D"])
        p[0]["obs_offsets"] = [0] + [1] * (len(p[0]["image_ids"]) - 1) + [total]

    return [("num_images 1", set_("local_ba_num_images", 1)), ("a negative angle", set_("local_ba_min_tri_angle", -1.0)),
            ("a NaN angle", set_("local_ba_min_tri_angle", float("nan"))), ("a point index out of range", point_range),
            ("a query that is not registered", unregistered_query), ("a point on an unregistered slot", unregistered_point),
            ("a query outside its problem", outside), ("a query on an unknown problem", problem_range), ("a non-finite pose", pose),
            ("a non-finite point", point), ("obs offsets", offsets)]


def lb_broken(fn):
    s, problems, queries, kw = copy.deepcopy(scenes.lb_get("degenerate"))
    fn(s, problems, queries, kw)
    return s, problems, queries, kw


@pytest.mark.parametrize("label,fn", lb_invalid_cases(), ids=[c[0] for c in lb_invalid_cases()])
def test_local_bundle_host_build_refuses_invalid_arguments(label, fn):
    s, problems, queries, kw = lb_broken(fn)
    with pytest.raises(capi.DsmError) as e:
        capi.local_bundles_host(s, problems, queries, **kw)
    assert e.value.code == 1 and all(not np.asarray(a).any() for a in e.value.outputs)


def test_local_bundle_capacities():
    s, problems, queries, kw = scenes.lb_get("degenerate")
    exp = lb_expected("degenerate")[0]
    nb, no = sum(len(e["bundle_image_ids"]) for e in exp), sum(len(e["overlap_image_ids"]) for e in exp)
    for caps in ((nb - 1, no), (nb, no - 1)):
        with pytest.raises(capi.DsmError) as e:
            capi.local_bundles_host(s, problems, queries, bundle_capacity=caps[0], overlap_capacity=caps[1], **kw)
        assert e.value.code == 4 and all(not np.asarray(a).any() for a in e.value.outputs)
    same_bundles(capi.local_bundles_host(s, problems, queries, bundle_capacity=nb, overlap_capacity=no, **kw)[0], exp)
