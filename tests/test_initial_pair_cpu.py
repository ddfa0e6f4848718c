"""CPU-only checks of dsm_find_initial_pairs: the host build of csrc/initial_pair.h against the sequential
restatement (tests/initial_pair_ref.py) -- the candidate order against the literal loops and a hand-written four-image answer,
the angle, Median and the gates bit for bit -- the margins of every scene the GPU tests use, and the exported symbols."""
import ctypes
import math
import os

import numpy as np
import pytest

from dagsfm_amd import capi
from tests import initial_pair_ref as ref
from tests import initial_pair_scenes as scenes

ACCEPT_MARGIN = 1e-3  # a thousand times the pose tolerance the GPU tests compare qvec, tvec and tri_angle with
POINT_MARGIN = 1e-9   # the project's MARGIN (tests/test_retriangulation_gpu.py)


def tiny_scene(counts, priors, n_points=200, duplicates=None):
    """Images `id: prior` and pairs `(id1, id2): n` of n distinct matches (k, k); duplicates[(id1, id2)] further matches repeat
    feature 0 of id1 (the duplicate rule drops them)."""
    ids = list(priors)
    cams = [capi.simple_pinhole(800.0, 500.0, 375.0, 1000, 750, True), capi.simple_pinhole(800.0, 500.0, 375.0, 1000, 750, False)]
    pairs, moff, m = [], [0], []
    for (a, b), n in counts.items():
        pairs.append((a, b))
        m += [(k, k) for k in range(n)] + [(0, n + k) for k in range((duplicates or {}).get((a, b), 0))]
        moff.append(len(m))
    return dict(camera_ids=np.array([1, 2], np.uint32), cameras=cams, image_ids=np.array(ids, np.uint32),
                image_camera_ids=np.array([1 if priors[i] else 2 for i in ids], np.uint32),
                points2D_offsets=np.arange(len(ids) + 1, dtype=np.uint32) * n_points, points2D_xy=np.zeros((len(ids) * n_points, 2)),
                pairs=np.array(pairs, np.uint32).reshape(-1, 2), match_offsets=np.array(moff, np.uint64),
                matches=np.array(m, np.uint32).reshape(-1, 2))


def orders(scene, problem, **kw):
    """The candidate list by the restatement's loops, the host build's loops and the host build's sorted schedule."""
    o = capi.default_initial_pair_options(**kw)
    loops, _ = capi.initial_pair_host_candidates(scene, [problem], o)
    keys, _ = capi.initial_pair_host_candidates(scene, [problem], o, sorted_schedule=True)
    want = [(int(a), int(b)) for a, b in ref.candidate_order(scene, problem, **kw)]
    assert loops[0] == want and keys[0] == want, (loops[0], keys[0], want)
    return want


FOUR = dict(counts={(3, 5): 45, (9, 5): 30, (7, 3): 45, (9, 7): 55, (5, 7): 29}, priors={5: True, 3: True, 9: True, 7: False},
            duplicates={(5, 7): 4})


def test_candidate_order_known_answer():
    """NumCorrespondences 5: 104, 3: 90, 9: 85, 7 (no prior): 129; (9, 5) keeps exactly init_min_num_inliers = 30, (5, 7) keeps 29
    of its 33 matches.  First images 5, 3, 9, 7; 5 -> 3 (45), 9 (30); 3 -> 5 (seen), 7; 9 -> 5 (seen), 7; 7 -> nothing new."""
    s = tiny_scene(**FOUR)
    every = dict(image_ids=[3, 5, 7, 9])
    assert orders(s, every, init_min_num_inliers=30) == [(5, 3), (5, 9), (3, 7), (9, 7)]
    assert orders(s, every, init_min_num_inliers=31) == [(5, 3), (3, 7), (9, 7)]  # the threshold: 30 no longer passes
    assert orders(s, every, init_min_num_inliers=29) == [(5, 3), (5, 9), (5, 7), (3, 7), (9, 7)]
    assert orders(s, dict(every, tried_pairs=[(7, 9), (3, 5)]), init_min_num_inliers=30) == [(5, 9), (3, 7)]
    assert orders(s, dict(every, num_registrations=[1, 0, 0, 0]), init_min_num_inliers=30) == [(5, 9), (9, 7)]
    assert orders(s, dict(every, init_num_reg_trials=[0, 2, 0, 0]), init_min_num_inliers=30) == [(3, 5), (3, 7), (9, 5), (9, 7)]
    assert orders(s, dict(every, init_num_reg_trials=[0, 2, 0, 0]), init_min_num_inliers=30, init_max_reg_trials=3)[0] == (5, 3)
    assert orders(s, dict(every, seed_image1=7), init_min_num_inliers=30) == [(7, 9), (7, 3)]
    assert orders(s, dict(every, seed_image2=7, init_num_reg_trials=[0, 0, 5, 0]), init_min_num_inliers=30) == [(7, 9), (7, 3)]
    assert orders(s, dict(every, seed_image1=5, seed_image2=7, tried_pairs=[(5, 7)]), init_min_num_inliers=30) == [(5, 7)]
    assert orders(s, dict(every, seed_image1=9, seed_image2=3), init_min_num_inliers=30) == [(9, 3)]  # a pair without matches
    assert orders(s, dict(image_ids=[9, 7, 5]), init_min_num_inliers=30) == [(9, 5), (9, 7)]  # a subset sees its own pairs only; the prior goes first
    _, kept = capi.initial_pair_host_candidates(s, [every], capi.default_initial_pair_options())
    assert list(kept) == [45, 30, 45, 55, 29]


def test_candidate_order_ties_go_to_the_smaller_id():
    s = tiny_scene(counts={(4, 2): 40, (2, 8): 40, (8, 6): 40, (6, 4): 40, (2, 6): 40}, priors={2: True, 4: True, 6: True, 8: True})
    # sums 2: 120, 6: 120, 4: 80, 8: 80; all counts equal: the second images of an image run in ascending id
    assert orders(s, dict(image_ids=[8, 6, 4, 2]), init_min_num_inliers=30) == [(2, 4), (2, 6), (2, 8), (6, 4), (6, 8)]


def test_candidate_order_random_scenes():
    rng = np.random.default_rng(3)
    for trial in range(60):
        n = int(rng.integers(2, 10))
        ids = [int(x) for x in rng.permutation(np.arange(1, 40))[:n]]
        priors = {i: bool(rng.random() < 0.75) for i in ids}
        counts, dups = {}, {}
        for a in range(n):
            for b in range(a + 1, n):
                if rng.random() < 0.7:
                    key = (ids[a], ids[b]) if rng.random() < 0.5 else (ids[b], ids[a])
                    counts[key] = int(rng.integers(28, 33))
                    dups[key] = int(rng.integers(0, 3))
        s = tiny_scene(counts, priors, n_points=64, duplicates=dups)
        sub = [i for i in ids if rng.random() < 0.8] or ids[:1]
        p = dict(image_ids=sub, num_registrations=[int(rng.random() < 0.15) for _ in sub],
                 init_num_reg_trials=[int(rng.integers(0, 3)) for _ in sub])
        if len(sub) >= 2 and rng.random() < 0.3:
            p["tried_pairs"] = [(sub[0], sub[1])]
        if rng.random() < 0.2:
            p["seed_image1"] = sub[int(rng.integers(0, len(sub)))]
        orders(s, p, init_min_num_inliers=int(rng.integers(28, 32)))


def test_candidate_order_argument_errors():
    s = tiny_scene(**FOUR)
    for problem in (dict(image_ids=[3, 5, 4]), dict(image_ids=[3, 5, 3]), dict(image_ids=[3, 5], seed_image1=9),
                    dict(image_ids=[3, 5], seed_image1=3, seed_image2=3)):
        with pytest.raises(capi.DsmError):
            capi.initial_pair_host_candidates(s, [problem])
    for kw in (dict(init_min_num_inliers=-1), dict(init_max_reg_trials=0), dict(init_max_error=0.0), dict(init_max_forward_motion=1.5),
               dict(init_min_tri_angle=-1.0), dict(speculation_window=0), dict(init_max_error=math.nan)):
        with pytest.raises(capi.DsmError):
            capi.initial_pair_host_candidates(s, [dict(image_ids=[3, 5])], capi.default_initial_pair_options(**kw))


def ptr(a):
    return a.ctypes.data


def test_angle_median_and_gates_bit_for_bit():
    L = capi.initial_pair_host_lib()
    acos = lambda q: float(L.dsm_ip_host_acos(q))
    rng = np.random.default_rng(11)
    for trial in range(300):
        q = rng.normal(size=4) * (10.0 ** rng.integers(-2, 3))
        t = rng.normal(size=3)
        X = rng.normal(size=3) * (10.0 ** rng.integers(-1, 3))
        P, C, C2 = np.zeros(12), np.zeros(3), np.zeros(3)
        L.dsm_ip_host_pose(ptr(q), ptr(t), ptr(P), ptr(C), ptr(C2))
        assert list(P) == ref.compose_P(q, t) and list(C) == ref.projection_center(q, t) and list(C2) == ref.minus_Rt_t(ref.quat_to_R(q), list(t))
        zero = np.zeros(3)
        a = float(L.dsm_ip_host_tri_angle(ptr(zero), ptr(C), ptr(X)))
        assert a == ref.tri_angle([0.0, 0.0, 0.0], list(C), list(X), acos)
        assert abs(a - ref.tri_angle([0.0, 0.0, 0.0], list(C), list(X))) <= 4e-16 * max(a, 1e-3)  # the host libm: within an ulp or two
        mg, angle = np.zeros(2), ctypes.c_double()
        deg = float(rng.choice([1.5, 16.0, 40.0]))
        ok = L.dsm_ip_host_point_gates(ptr(q), ptr(t), ptr(X), deg, ctypes.addressof(angle), ptr(mg))
        m = ref.Margins()
        want = ref.point_gates(ref.tri_angle([0.0, 0.0, 0.0], ref.projection_center(q, t), list(X), acos), deg * ref.DEG, ref.I34,
                               ref.compose_P(q, t), list(X), m)
        assert bool(ok) == want and list(mg) == [m.point_angle, m.point_depth] and angle.value == a
    for n in (1, 2, 3, 4, 63, 64, 65, 129, 1000):
        a = rng.random(n) * (rng.random(n) < 0.9)  # ties at zero
        assert float(L.dsm_ip_host_median(ptr(a), n)) == ref.median([float(x) for x in a])
    o = capi.default_initial_pair_options()
    thr = o.init_min_tri_angle * ref.DEG
    assert float(L.dsm_ip_host_min_tri_angle_rad(o.init_min_tri_angle)) == thr
    for inl, tz, ang in ((100, 0.5, 0.3), (99, 0.5, 0.3), (100, -0.95, 0.3), (100, 0.9499999, thr), (100, -0.3, math.nextafter(thr, 1.0)),
                         (100, 0.0, 0.0), (4000000000, 0.1, 1.0)):
        mg = np.zeros(2)
        m = ref.Margins()
        want = ref.accept(inl, tz, ang, ref.default_options(), m)
        assert bool(L.dsm_ip_host_accept(inl, tz, ang, ctypes.byref(o), ptr(mg))) == want and list(mg) == [m.forward, m.tri_angle]


@pytest.mark.parametrize("name", sorted(scenes.SCENES))
def test_every_gpu_scene_is_clear(name, oracle):
    """Every scene of tests/test_initial_pair_gpu.py decides with margins the device's tolerances cannot flip: tri_angle and
    |tvec.z| at least 1e-3 relative, the per-point gates at least 1e-9.  No scene is excluded; a scene that fails here is changed."""
    s, problems, kw = scenes.get(name)
    for r in ref.find_initial_pairs(s, problems, oracle, **kw):
        assert r["margins"].acceptance() >= ACCEPT_MARGIN, (name, r["margins"].tri_angle, r["margins"].forward)
        assert r["margins"].points() >= POINT_MARGIN, (name, r["margins"].point_angle, r["margins"].point_depth)
    counts = np.diff(np.asarray(s["match_offsets"], np.int64))
    assert 2 <= len(s["image_ids"]) <= 10 and counts.min() >= 40 and counts.max() <= 300, (len(s["image_ids"]), counts)  # the tiny shapes


def test_scene_outcomes(oracle):
    """What the scenes were built to show, on the restatement alone."""
    def run(name):
        s, problems, kw = scenes.get(name)
        return ref.find_initial_pairs(s, problems, oracle, **kw)
    r = run("ring")[0]
    assert r["found"] and len(r["tried"]) == 1
    r = run("forward_motion")[0]
    assert r["found"] and len(r["tried"]) == 2 and abs(r["records"][0]["tvec"][2]) > 0.95
    r = run("small_baseline")[0]
    assert r["found"] and len(r["tried"]) == 6 and all(0 < x["tri_angle"] < 16 * ref.DEG for x in r["records"][:5])
    r = run("planar")[0]
    assert r["found"] and r["estimate"]["config"] == capi_config("PLANAR")
    r = run("pure_rotation")[0]
    assert not r["found"] and r["records"][0]["config"] == capi_config("PANORAMIC") and r["records"][0]["tri_angle"] == 0.0
    r = run("watermark")[0]
    assert r["found"] and r["records"][0]["config"] == capi_config("WATERMARK") and len(r["tried"]) == 2
    r = run("nothing_found")[0]
    s, problems, kw = scenes.get("nothing_found")
    assert not r["found"] and len(r["tried"]) == 6 and r["tried"] == ref.candidate_order(s, problems[0], **kw)
    assert all(x["found"] for x in run("batching"))
    for n in (63, 64, 65, 257):
        r = run("triangulation_%d" % n)[0]
        m = r["estimate"]["matches"]
        assert r["found"] and len(m) == n and 0 < len(r["points"]) < n


def capi_config(name):
    return {"PLANAR": 4, "PANORAMIC": 5, "WATERMARK": 7}[name]


def test_new_symbols_are_exported_and_bound():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dagsfm_mi355x.h")).read()
    for sym in ("dsm_find_initial_pairs", "dsm_default_initial_pair_options"):
        assert sym + "(" in header
        for path in (capi.LIB_PATH, capi.CHECK_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), sym), (path, sym)
        assert getattr(capi.lib(), sym).argtypes is not None
    assert ctypes.sizeof(capi.InitialPairOptions) == 40 and ctypes.sizeof(capi.InitialPairResult) == 24 + ctypes.sizeof(capi.TwoViewGeometry)
    assert ctypes.sizeof(capi.InitialPairReport) == 32 + 11 * 8
    o = capi.default_initial_pair_options()
    assert (o.init_min_num_inliers, o.init_max_error, o.init_max_forward_motion, o.init_min_tri_angle, o.init_max_reg_trials, o.user_seed) == \
        (100, 4.0, 0.95, 16.0, 2, 0) and o.speculation_window >= 1  # incremental_mapper.h:68-81
    assert hasattr(capi.Context, "find_initial_pairs") and "DSM_INITIAL_PAIR_SERIAL" in capi.CHECK_OPTION_KEYS
    assert os.path.exists(capi.INITIAL_PAIR_HOST_LIB_PATH)
