"""Scenes of the track-update tests: hand-built known answers, one per branch of the reference's Complete and
Merge, and random reconstructions with observations stripped and points split.  Every scene is checked here, with the
restatement alone, to have all of the reference's decision margins clear of 1e-9 relative; a random scene that fails the check
is rebuilt with another seed (checked_random_scene), never skipped.

The hand-built scenes share one geometry, so their answers follow by hand: SIMPLE_PINHOLE f = 500, every camera looks along
+z from (0.5 i, 0, -8) with the identity rotation, the points lie at z = 0.  A point moved by d along x moves by 62.5 d pixels in
every image; a feature is the exact projection of its point, plus a stated offset in pixels."""
import numpy as np

from dagsfm_amd import capi
from tests import retriangulation_ref as rt
from tests import track_update_ref as ref

MERGE, COMPLETE = ref.MERGE, ref.COMPLETE
MIN_MARGIN = 1e-9


class Tiny:
    def __init__(self, n_images, unregistered=(), bogus=(), behind=()):
        self.n = n_images
        self.reg = [0 if i in unregistered else 1 for i in range(n_images)]
        self.cam = [1 if i in bogus else 0 for i in range(n_images)]
        self.centre = [np.array([0.5 * i, 0.0, 8.0 if i in behind else -8.0]) for i in range(n_images)]
        self.feats = [[] for _ in range(n_images)]
        self.pairs, self.matches = [], {}
        self.points = []

    def image_id(self, i):
        return 3 * i + 1

    def feat(self, img, X, dx=0.0, dy=0.0):
        p = np.asarray(X, np.float64) - self.centre[img]
        self.feats[img].append((500.0 * p[0] / p[2] + 320.0 + dx, 500.0 * p[1] / p[2] + 240.0 + dy))
        return (img, len(self.feats[img]) - 1)

    def link(self, a, b):
        if a[0] > b[0]:
            a, b = b, a
        key = (a[0], b[0])
        if key not in self.matches:
            self.pairs.append(key)
            self.matches[key] = []
        self.matches[key].append((a[1], b[1]))

    def point(self, pid, X, elems):
        self.points.append((pid, np.asarray(X, np.float64), list(elems)))

    def obs(self, elems):
        return [(self.image_id(i), k) for i, k in elems]

    def scene(self):
        good = capi.simple_pinhole(500.0, 320.0, 240.0, 640, 480)
        bad = capi.simple_pinhole(1.0e5, 320.0, 240.0, 640, 480)  # focal / max size = 156 > 10: HasBogusParams
        offs = np.concatenate([[0], np.cumsum([len(f) for f in self.feats])]).astype(np.uint32)
        xy = np.array([p for f in self.feats for p in f], np.float64).reshape(-1, 2)
        moff, m = [0], []
        for key in self.pairs:
            m.extend(self.matches[key])
            moff.append(len(m))
        toff, tobs = [0], []
        for _, _, elems in self.points:
            tobs.extend(self.obs(elems))
            toff.append(len(tobs))
        return dict(camera_ids=np.array([7, 8], np.uint32), cameras=[good, bad],
                    image_ids=np.array([self.image_id(i) for i in range(self.n)], np.uint32),
                    image_camera_ids=np.array([7 + c for c in self.cam], np.uint32), registered=np.array(self.reg, np.uint8),
                    qvec=np.tile([1.0, 0.0, 0.0, 0.0], (self.n, 1)), tvec=np.array([-c for c in self.centre]),
                    points2D_offsets=offs, points2D_xy=xy,
                    pairs=np.array([(self.image_id(a), self.image_id(b)) for a, b in self.pairs], np.uint32).reshape(-1, 2),
                    match_offsets=np.array(moff, np.uint64), matches=np.array(m, np.uint32).reshape(-1, 2),
                    point3D_ids=np.array([p for p, _, _ in self.points], np.uint64),
                    point3D_xyz=np.array([x for _, x, _ in self.points], np.float64).reshape(-1, 3),
                    track_offsets=np.array(toff, np.uint64), track_obs=np.array(tobs, np.uint32).reshape(-1, 2))


def _case(t, steps, tracks, counts, modified, selected=None, xyz=None, complete_trials=None, merge_trials=None, **options):
    """tracks: {id: [(image index, point2D_idx)]}; xyz: {id: array} where the answer is not an input point's."""
    return dict(scene=t.scene(), steps=list(steps), selected=selected, options=options,
                tracks={int(p): t.obs(e) for p, e in tracks.items()}, counts=list(counts), modified=sorted(modified), xyz=xyz or {},
                complete_trials=complete_trials, merge_trials=merge_trials)


O = np.zeros(3)


def mean(n1, x1, n2, x2):
    return (float(n1) * np.asarray(x1, np.float64) + float(n2) * np.asarray(x2, np.float64)) / float(n1 + n2)


def _chain(n_links, max_t):
    """a0, a1 in the track; f2 .. f(n_links + 1) each reachable through the one before only"""
    t = Tiny(2 + n_links)
    a0, a1 = t.feat(0, O), t.feat(1, O)
    t.link(a0, a1)
    f, prev = [], a1
    for i in range(n_links):
        f.append(t.feat(2 + i, O))
        t.link(prev, f[-1])
        prev = f[-1]
    t.point(10, O, [a0, a1])
    got = min(n_links, max_t)
    return _case(t, [COMPLETE], {10: [a0, a1] + f[:got]}, [got], [10] if got else [], complete_trials=got, complete_max_transitivity=max_t)


def _contest(k):
    """k points with the same xyz contest f; g is reachable through f only.  The lowest id takes both."""
    t = Tiny(2 * k + 2)
    f, g = t.feat(2 * k, O), t.feat(2 * k + 1, O)
    t.link(f, g)
    tracks = {}
    for p in range(k):
        a, b = t.feat(2 * p, O), t.feat(2 * p + 1, O)
        t.link(b, f)
        pid = 5 + 4 * (k - 1 - p)  # input order descending in id: the rank is the id's, not the input position's
        t.point(pid, O, [a, b])
        tracks[pid] = [a, b] + ([f, g] if p == k - 1 else [])
    return _case(t, [COMPLETE], tracks, [2], [5], complete_trials=2)


def _merge_scene(n_images=4, bad_b3=False, xb=0.02):
    t = Tiny(n_images)
    XA, XB = O, np.array([xb, 0.0, 0.0])
    a0, a1 = t.feat(0, XA), t.feat(1, XA)
    b2, b3 = t.feat(2, XB), t.feat(3, XB, dx=50.0 if bad_b3 else 0.0)
    t.point(3, XA, [a0, a1])
    t.point(8, XB, [b2, b3])
    return t, XA, XB, a0, a1, b2, b3


def cases():
    """name -> case.  Every answer is worked out in the comment above its scene."""
    out = {}
    # level 0 reaches f2 through a1, level 1 reaches f3 through f2
    out["two_levels"] = _chain(2, 5)
    # max_transitivity 1: f2 is added at level 0 = max - 1 and not enqueued, f3 is never tested
    out["cap_1"] = _chain(2, 1)
    # max_transitivity 5: levels 0 .. 4 add f2 .. f6; f6 (level 4 = max - 1) is not enqueued, f7 is never tested
    out["cap_5"] = _chain(6, 5)
    # a1 -> u (unregistered image, skipped; w behind it is lost), b (bogus camera, skipped without a test),
    # h (behind its camera: tested, DBL_MAX, rejected), g (added)
    t = Tiny(7, unregistered=(2,), bogus=(4,), behind=(5,))
    a0, a1 = t.feat(0, O), t.feat(1, O)
    u, w, b, h, g = t.feat(2, O), t.feat(3, O), t.feat(4, O), t.feat(5, O), t.feat(6, O)
    for x in (u, b, h, g):
        t.link(a1, x)
    t.link(u, w)
    t.point(10, O, [a0, a1])
    out["filters"] = _case(t, [COMPLETE], {10: [a0, a1, g]}, [1], [10], complete_trials=2)
    # f2 corresponds to a0 and to a1: added through a0, then it has a point
    t = Tiny(3)
    a0, a1, f2 = t.feat(0, O), t.feat(1, O), t.feat(2, O)
    t.link(a0, f2)
    t.link(a1, f2)
    t.point(10, O, [a0, a1])
    out["two_elements"] = _case(t, [COMPLETE], {10: [a0, a1, f2]}, [1], [10], complete_trials=1)
    out["contest_2"] = _contest(2)
    out["contest_3"] = _contest(3)
    # A (id 3) and B (id 8) 1.25 px apart: every element is 0.625 px from the mean; Merge(3) takes B, the new point is 9
    t, XA, XB, a0, a1, b2, b3 = _merge_scene()
    t.link(a1, b2)
    out["merge_ok"] = _case(t, [MERGE], {9: [a0, a1, b2, b3]}, [4], [9], xyz={9: mean(2, XA, 2, XB)}, merge_trials=1)
    # b3 is 50 px off: the second track's second element refuses; Merge(8) finds {8, 3} in the memo
    t, XA, XB, a0, a1, b2, b3 = _merge_scene(bad_b3=True)
    t.link(a1, b2)
    out["merge_refused"] = _case(t, [MERGE], {3: [a0, a1], 8: [b2, b3]}, [0], [], merge_trials=1)
    # Merge(3) takes B (-> 13, count 4), the recursion Merge(13) takes C through b3 (-> 14, count 6), Merge(14) finds nothing
    # and returns 0, so Merge(13) returns 6 and Merge(3) returns 6; 8 and 12 no longer exist at their turns
    t, XA, XB, a0, a1, b2, b3 = _merge_scene(6)
    XC = np.array([0.01, 0.0, 0.0])
    c4, c5 = t.feat(4, XC), t.feat(5, XC)
    t.point(12, XC, [c4, c5])
    t.link(a1, b2)
    t.link(b3, c4)
    m1 = mean(2, XA, 2, XB)
    out["merge_recursion"] = _case(t, [MERGE], {14: [a0, a1, b2, b3, c4, c5]}, [6], [14], xyz={14: mean(4, m1, 2, XC)}, merge_trials=2)
    # two links between A and B, B refusing: one trial at a0, the memo at a1, and at both links at B's turn
    t, XA, XB, a0, a1, b2, b3 = _merge_scene(bad_b3=True)
    t.link(a0, b2)
    t.link(a1, b3)
    out["second_link"] = _case(t, [MERGE], {3: [a0, a1], 8: [b2, b3]}, [0], [], merge_trials=1)
    # component {1, 4, 5}: Merge(1) tries 4 and fails (12.5 px apart); Merge(4) skips 1 (memo), takes 5 (-> id 7), and the
    # recursion tries 1 again (a new point, a new pair) and fails.  Component {2, 3}: Merge(2) takes 3 (-> id 6) in between.
    t = Tiny(10)
    X1, X4, X5, X2, X3 = np.array([0.2, 0, 0]), O, np.array([0.02, 0, 0]), np.array([1.0, 0, 0]), np.array([1.02, 0, 0])
    p1, p4, p5 = [t.feat(0, X1), t.feat(1, X1)], [t.feat(2, X4), t.feat(3, X4)], [t.feat(4, X5), t.feat(5, X5)]
    p2, p3 = [t.feat(6, X2), t.feat(7, X2)], [t.feat(8, X3), t.feat(9, X3)]
    t.link(p1[1], p4[0])
    t.link(p4[1], p5[0])
    t.link(p2[1], p3[0])
    for pid, X, e in ((4, X4, p4), (2, X2, p2), (5, X5, p5), (1, X1, p1), (3, X3, p3)):
        t.point(pid, X, e)
    out["interleave"] = _case(t, [MERGE], {1: p1, 6: p2 + p3, 7: p4 + p5}, [8], [6, 7],
                              xyz={6: mean(2, X2, 2, X3), 7: mean(2, X4, 2, X5)}, merge_trials=4)
    # MERGE then COMPLETE over {3, 8}: 8 is merged away at its MERGE turn, both are gone at their COMPLETE turns, and the merged
    # point 9 is not in the set: f (a correspondence of a0, 0.625 px from the mean) stays free
    t, XA, XB, a0, a1, b2, b3 = _merge_scene(5)
    f = t.feat(4, XA)
    t.link(a1, b2)
    t.link(a0, f)
    out["selected_merged_away"] = _case(t, [MERGE, COMPLETE], {9: [a0, a1, b2, b3]}, [4, 0], [9], selected=[8, 3],
                                        xyz={9: mean(2, XA, 2, XB)}, merge_trials=1, complete_trials=0)
    # the same without a selection: COMPLETE's snapshot holds 9, which takes f
    out["all_after_merge"] = _case(t, [MERGE, COMPLETE], {9: [a0, a1, b2, b3, f]}, [4, 1], [9], xyz={9: mean(2, XA, 2, XB)},
                                   merge_trials=1, complete_trials=1)
    # A and B 3.75 px apart, f 3 px from A on the far side.  COMPLETE first: A takes f (3 px); then the mean of (3 A, 2 B) is
    # 1.5 px from A and f 4.5 px from it: Merge refuses.  MERGE first: the mean is 1.875 px from both, the merge succeeds, and
    # f is 4.875 px from the merged point: Complete refuses.
    t, XA, XB, a0, a1, b2, b3 = _merge_scene(5, xb=0.06)
    f = t.feat(4, XA, dx=-3.0)
    t.link(a1, b2)
    t.link(a0, f)
    out["complete_then_merge"] = _case(t, [COMPLETE, MERGE], {3: [a0, a1, f], 8: [b2, b3]}, [1, 0], [3], complete_trials=1, merge_trials=1)
    out["merge_then_complete"] = _case(t, [MERGE, COMPLETE], {9: [a0, a1, b2, b3]}, [4, 0], [9], xyz={9: mean(2, XA, 2, XB)},
                                       complete_trials=1, merge_trials=1)
    # The two orders of Merge's memo inside a component of 66 points (done[b] against born[a]).  R (id 1, 12.5 px
    # from the others) is linked to Q_1 and to Q_65 and refuses everyone; Q_1 .. Q_65 share one xyz and are linked in a chain.
    # Merge(R) tries Q_1 and Q_65 and ends without a merge (2 trials).  Merge(Q_1) meets R, whose loop ended while Q_1 existed:
    # the pair is in the memo, no trial; it takes Q_2 (1 trial), and the recursion's new point was born after R's loop ended, so
    # it must try R (a new pair: 1 trial, refused) before it takes Q_3, and so on: 64 merges and 64 refused trials of R by the
    # 64 merged points; the last one holds Q_65's link to R as well and skips it (tried in this loop).  130 trials in all.
    n = 65
    t = Tiny(2 * n + 2)
    XR = np.array([0.2, 0.0, 0.0])
    r = [t.feat(2 * n, XR), t.feat(2 * n + 1, XR)]
    t.point(1, XR, r)
    q, prev = [], None
    for j in range(n):
        a_, b_ = t.feat(2 * j, O), t.feat(2 * j + 1, O)
        t.point(50 + 2 * j, O, [a_, b_])
        q += [a_, b_]
        if prev is not None:
            t.link(prev, a_)
        prev = b_
    t.link(q[0], r[0])
    t.link(q[-1], r[1])
    last = 50 + 2 * (n - 1) + (n - 1)
    out["memo_orders"] = _case(t, [MERGE], {1: r, last: q}, [2 * n], [last], xyz={last: O}, merge_trials=2 * n)
    return out


def long_track(L):
    """A of L elements over L images, B of two elements 0.625 px from the mean with A, a free correspondence f of A's first
    element, and a free correspondence g of B's last one: COMPLETE adds both, MERGE joins A and B."""
    t = Tiny(L + 4)
    XB = np.array([0.01, 0.0, 0.0])
    a = [t.feat(i, O) for i in range(L)]
    b = [t.feat(L, XB), t.feat(L + 1, XB)]
    f, g = t.feat(L + 2, O), t.feat(L + 3, XB)
    t.link(a[-1], b[0])
    t.link(a[0], f)
    t.link(b[1], g)
    t.point(21, O, a)
    t.point(22, XB, b)
    return t.scene()


def wide_level(K, track=2):
    """A track of `track` elements whose last one has K free correspondences, one per image, all within the threshold: K
    candidates in level 0, and behind each a second one for level 1.  track = 2 walks on a lane of the device, track = 17 on a
    wave (csrc/track_update.hip TU_LANE_CUT = 16), where 64 candidates fill one ballot and 65 leave a tail of one."""
    t = Tiny(track + 2 * K)
    a = [t.feat(i, O) for i in range(track)]
    t.point(10, O, a)
    for k in range(K):
        f, g = t.feat(track + k, O), t.feat(track + K + k, O, dx=1.0)
        t.link(a[-1], f)
        t.link(f, g)
    return t.scene()


def claim_chain(k):
    """k points with one xyz; c_j is a correspondence of p_j and of p_(j + 1).  p_j (the lower id) takes c_j, and p_(j + 1) can
    only commit once p_j has: the claim rounds of the device equal k."""
    t = Tiny(3 * k)
    second = []
    for j in range(k):
        a, b = t.feat(2 * j, O), t.feat(2 * j + 1, O)
        t.point(100 + j, O, [a, b])
        second.append(b)
    for j in range(k - 1):
        c = t.feat(2 * k + j, O)
        t.link(second[j], c)
        t.link(second[j + 1], c)
    return t.scene()


def merge_chain(n):
    """n points with one xyz linked in a chain: one component; Merge of the first takes all the others by recursion."""
    t = Tiny(2 * n)
    prev = None
    for j in range(n):
        a, b = t.feat(2 * j, O), t.feat(2 * j + 1, O)
        t.point(50 + 2 * j, O, [a, b])
        if prev is not None:
            t.link(prev, a)
        prev = b
    return t.scene()


def check_case(case, got):
    """got (the dict of update_tracks) against the hand-computed answer."""
    ids = sorted(case["tracks"])
    assert [int(i) for i in got["point_ids"]] == ids
    toff = [int(x) for x in got["track_offsets"]]
    sc = case["scene"]
    for k, pid in enumerate(ids):
        assert [tuple(int(v) for v in o) for o in got["track_obs"][toff[k]:toff[k + 1]]] == case["tracks"][pid], pid
        if pid in case["xyz"]:
            want = case["xyz"][pid]
        else:
            want = np.asarray(sc["point3D_xyz"])[[int(i) for i in sc["point3D_ids"]].index(pid)]
        assert np.asarray(got["xyz"][k], np.float64).tobytes() == np.asarray(want, np.float64).tobytes(), pid
    assert [int(c) for c in got["step_counts"]] == case["counts"]
    assert [int(i) for i in got["modified"]] == case["modified"]


def trial_counts(got):
    """(complete_trials, merge_trials) of a restatement result or of a library result"""
    if "report" in got:
        return int(got["report"].complete_trials), int(got["report"].merge_trials)
    return int(got["complete_trials"]), int(got["merge_trials"])


def same_result(a, b):
    """Exact: ids, track order, modified, step counts, trial counts, xyz bit for bit."""
    for key in ("point_ids", "track_offsets", "track_obs", "modified", "step_counts"):
        assert np.array_equal(np.asarray(a[key], np.int64), np.asarray(b[key], np.int64)), key
    assert np.asarray(a["xyz"], np.float64).tobytes() == np.asarray(b["xyz"], np.float64).tobytes(), "xyz"
    assert trial_counts(a) == trial_counts(b), "trial counts"


def random_scene(n_images, n_points, seed, strip=1.0 / 3.0, split=0.3, wrong=0.08, unregistered=()):
    """A reconstruction over retriangulation_ref.make_scene's images and matches: every ground-truth point is a point3D seen by
    all its images; then a fraction `strip` of the observations is taken out of the tracks (at least two stay) and a fraction
    `split` of the points with four or more observations is split in two (both halves near the true position)."""
    scene, _ = rt.make_scene(n_images=n_images, n_points=n_points, track=(3, 7), noise=0.4, wrong=wrong, existing=1.0, seed=seed,
                             unregistered=unregistered)
    rng = np.random.default_rng(seed + 7919)
    off = np.asarray(scene["points2D_offsets"], np.int64)
    p3 = np.asarray(scene["points2D_point3D"], np.int64)
    img_of_feat = np.repeat(np.arange(n_images), off[1:] - off[:-1])
    tracks = [[] for _ in range(len(scene["point3D_ids"]))]
    for f, q in enumerate(p3):
        if q >= 0 and scene["registered"][img_of_feat[f]]:
            tracks[q].append((int(scene["image_ids"][img_of_feat[f]]), int(f - off[img_of_feat[f]])))
    xyz = np.asarray(scene["point3D_xyz"], np.float64)
    out_xyz, out_tracks = [], []
    for q, tr in enumerate(tracks):
        keep = [e for e in tr if rng.random() >= strip]
        if len(keep) < 2:
            keep = tr[:2]
        if len(keep) < 2:
            continue
        if len(keep) >= 4 and rng.random() < split:
            h = len(keep) // 2
            for part in (keep[:h], keep[h:]):
                out_xyz.append(xyz[q] + rng.normal(0, 0.002, 3))
                out_tracks.append(part)
        else:
            out_xyz.append(xyz[q])
            out_tracks.append(keep)
    ids = rng.choice(1 << 40, len(out_tracks), replace=False).astype(np.uint64) + 1
    s = {k: v for k, v in scene.items() if k not in ("points2D_point3D", "point3D_ids", "point3D_xyz")}
    s["point3D_ids"], s["point3D_xyz"] = ids, np.array(out_xyz, np.float64).reshape(-1, 3)
    s["track_offsets"] = np.concatenate([[0], np.cumsum([len(t) for t in out_tracks])]).astype(np.uint64)
    s["track_obs"] = np.array([e for t in out_tracks for e in t], np.uint32).reshape(-1, 2)
    return s


STEP_ORDERS = ([COMPLETE, MERGE], [MERGE, COMPLETE])


def margins_clear(scene, step_orders=STEP_ORDERS, selected=None, **options):
    return all(ref.min_margin(ref.update_tracks(scene, steps, selected, **options)) >= MIN_MARGIN for steps in step_orders)


def checked_random_scene(n_images, n_points, seed, **kw):
    """The first seed from `seed` on whose scene has every margin of both step orders clear of MIN_MARGIN."""
    for s in range(seed, seed + 50):
        scene = random_scene(n_images, n_points, s, **kw)
        if margins_clear(scene):
            return scene
    raise AssertionError("no clear scene in 50 seeds")


def shuffled_points(scene, seed):
    """The same scene with its points3D in another input order."""
    rng = np.random.default_rng(seed)
    toff = np.asarray(scene["track_offsets"], np.int64)
    perm = rng.permutation(len(toff) - 1)
    tobs = np.asarray(scene["track_obs"]).reshape(-1, 2)
    s = dict(scene)
    s["point3D_ids"] = np.asarray(scene["point3D_ids"])[perm]
    s["point3D_xyz"] = np.asarray(scene["point3D_xyz"]).reshape(-1, 3)[perm]
    s["track_offsets"] = np.concatenate([[0], np.cumsum((toff[1:] - toff[:-1])[perm])]).astype(np.uint64)
    s["track_obs"] = np.concatenate([tobs[toff[p]:toff[p + 1]] for p in perm] + [np.zeros((0, 2), tobs.dtype)]).reshape(-1, 2)
    return s


def shuffled_matches(scene, seed):
    """The same scene with the matches of every pair in another order (make_scene's lists are one-to-one: the duplicate rule
    drops none, so the correspondence lists do not change)."""
    rng = np.random.default_rng(seed)
    moff = np.asarray(scene["match_offsets"], np.int64)
    m = np.array(scene["matches"], np.uint32, copy=True).reshape(-1, 2)
    for k in range(len(moff) - 1):
        m[moff[k]:moff[k + 1]] = m[moff[k]:moff[k + 1]][rng.permutation(moff[k + 1] - moff[k])]
    s = dict(scene)
    s["matches"] = m
    return s


def synthetic_scene(n_images, seed, strip=1.0 / 3.0, split=0.3, n_feats=160, n_obs=110, n_pool=480):
    """A reconstruction over dagsfm_amd/synthetic.py's Scene: cameras on a shell with general rotations, every image observing
    n_obs of the n_pool points (a fifth of those keypoints thrown elsewhere: geometric outliers) plus clutter features.  Two
    features of two images that observe the same pool point match (every pair of images, in (i, j) order); a pool point seen
    twice or more is a point3D whose track holds its observations, outliers included.  Then a fraction `strip` of the
    observations is taken out of the tracks (two stay) and a fraction `split` of the points with four or more is split in two."""
    from dagsfm_amd import synthetic
    syn = synthetic.Scene(n_images, n_feats, seed=seed, n_obs=n_obs, n_pool=n_pool)
    rng = np.random.default_rng([seed, 4242])
    ims = [syn.image(i) for i in range(n_images)]
    image_ids = np.arange(n_images, dtype=np.uint32) * 3 + 1
    where = [{int(p): k for k, p in enumerate(im[3]) if p >= 0} for im in ims]
    pairs, moff, matches = [], [0], []
    for i in range(n_images):
        for j in range(i + 1, n_images):
            common = [(where[i][p], where[j][p]) for p in where[i] if p in where[j]]
            if common:
                pairs.append((image_ids[i], image_ids[j]))
                matches.extend(sorted(common))
                moff.append(len(matches))
    seen = {}
    for i in range(n_images):
        for p, k in sorted(where[i].items(), key=lambda x: x[1]):
            seen.setdefault(p, []).append((int(image_ids[i]), k))
    xyz, tracks = [], []
    for p in sorted(seen):
        tr = seen[p]
        if len(tr) < 2:
            continue
        keep = [e for e in tr if rng.random() >= strip]
        if len(keep) < 2:
            keep = tr[:2]
        if len(keep) >= 4 and rng.random() < split:
            h = len(keep) // 2
            for part in (keep[:h], keep[h:]):
                xyz.append(syn.points[p] + rng.normal(0, 0.003, 3))
                tracks.append(part)
        else:
            xyz.append(syn.points[p] + rng.normal(0, 0.001, 3))
            tracks.append(keep)
    ids = rng.choice(1 << 40, len(tracks), replace=False).astype(np.uint64) + 1
    f, cx, cy = syn.camera_params()
    return dict(camera_ids=np.array([7], np.uint32), cameras=[capi.simple_pinhole(f, cx, cy, syn.width, syn.height)], image_ids=image_ids,
                image_camera_ids=np.full(n_images, 7, np.uint32), registered=np.ones(n_images, np.uint8),
                qvec=np.array([rt.rot_to_quat(im[2][0]) for im in ims]), tvec=np.array([im[2][1] for im in ims]),
                points2D_offsets=(np.arange(n_images + 1) * n_feats).astype(np.uint32),
                points2D_xy=np.concatenate([im[1].astype(np.float64) for im in ims]).reshape(-1, 2),
                pairs=np.array(pairs, np.uint32).reshape(-1, 2), match_offsets=np.array(moff, np.uint64),
                matches=np.array(matches, np.uint32).reshape(-1, 2), point3D_ids=ids, point3D_xyz=np.array(xyz, np.float64).reshape(-1, 3),
                track_offsets=np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint64),
                track_obs=np.array([e for t in tracks for e in t], np.uint32).reshape(-1, 2))


def checked_synthetic_scene(n_images, seed):
    for s in range(seed, seed + 50):
        scene = synthetic_scene(n_images, s)
        if margins_clear(scene):
            return scene
    raise AssertionError("no clear scene in 50 seeds")


CASES = cases()
_random = {}


def named_random_scene(name):
    """The random scenes of both suites, built once (each the first seed whose margins are clear)."""
    if name not in _random:
        n_images, n_points, seed, kw = {"small": (8, 60, 1, {}), "medium": (12, 150, 3, {}),
                                         "unregistered": (10, 100, 5, {"unregistered": (4,)}), "forty": (40, 0, 11, {})}[name]
        _random[name] = checked_synthetic_scene(n_images, seed) if name == "forty" else checked_random_scene(n_images, n_points, seed, **kw)
    return _random[name]


def broken(scene, **changes):
    s = dict(scene)
    for k, v in changes.items():
        s[k] = v
    return s


def invalid_cases():
    """(name, scene, steps, selected, next_point3D_id, options): every call dsm_update_tracks refuses."""
    base = CASES["merge_recursion"]["scene"]
    ids, xyz = np.asarray(base["point3D_ids"]), np.asarray(base["point3D_xyz"], np.float64)
    tobs, pairs, m = np.asarray(base["track_obs"]), np.asarray(base["pairs"]), np.asarray(base["matches"])

    def edit(a, index, value):
        a = np.array(a, copy=True)
        a[index] = value
        return a

    S = [MERGE, COMPLETE]
    return [("transitivity_0", base, S, None, 0, dict(complete_max_transitivity=0)),
            ("negative_threshold", base, S, None, 0, dict(merge_max_reproj_error=-1.0)),
            ("nan_threshold", base, S, None, 0, dict(complete_max_reproj_error=float("nan"))),
            ("unknown_step", base, [MERGE, 2], None, 0, {}),
            ("feature_in_two_tracks", broken(base, track_obs=edit(tobs, 2, tobs[0])), S, None, 0, {}),
            ("track_unknown_image", broken(base, track_obs=edit(tobs, (1, 0), 999)), S, None, 0, {}),
            ("track_index_out_of_range", broken(base, track_obs=edit(tobs, (1, 1), 7)), S, None, 0, {}),
            ("track_unregistered_image", broken(base, registered=edit(base["registered"], 1, 0)), S, None, 0, {}),
            ("repeated_point_id", broken(base, point3D_ids=edit(ids, 1, ids[0])), S, None, 0, {}),
            ("next_id_too_small", base, S, None, int(ids.max()), {}),
            ("non_finite_xyz", broken(base, point3D_xyz=edit(xyz, (0, 1), np.inf)), S, None, 0, {}),
            ("selected_no_point", base, S, [3, 4], 0, {}),
            ("selected_repeated", base, S, [3, 3], 0, {}),
            ("self_pair", broken(base, pairs=edit(pairs, (0, 1), pairs[0, 0])), S, None, 0, {}),
            ("repeated_pair", broken(base, pairs=edit(pairs, 1, pairs[0][::-1])), S, None, 0, {}),
            ("match_out_of_range", broken(base, matches=edit(m, (0, 0), 5)), S, None, 0, {}),
            ("track_offsets_descend", broken(base, track_offsets=np.array([0, 4, 2, 6], np.uint64)), S, None, 0, {})]
