"""Sequential restatement of IncrementalTriangulator::CompleteTracks / CompleteAllTracks and MergeTracks / MergeAllTracks
(src/sfm/incremental_triangulator.cc:231-287, Merge :588-677, Complete :679-746) with Reconstruction::MergePoints3D
(src/base/reconstruction.cc:215-241), what dsm_update_tracks and libdsm_track_update_host.so are compared with.

The reference's loops are kept as they are: Complete's level queue with complete_max_transitivity and the
`transitivity < max - 1` enqueue rule; Merge's merge_trials_ memo (cleared per MergeTracks call), the weighted mean, the
all-elements test with its early break, MergePoints3D's track concatenation (track 1, then track 2), the recursion on the
merged point and the return rule "the recursive count if > 0, else the own count".  The correspondence graph with its
(pair, match) append order is tests/retriangulation_ref.py's; the reprojection error with its z < epsilon -> DBL_MAX case and
HasBogusParams are tests/point_filter_ref.py's.

Rulings, where the reference iterates unordered containers or leaves a choice:
  * points run in ascending point3D id; a step without a selection (*AllTracks) takes a snapshot of the ids at its start;
  * a merged point gets the id AddPoint3D would hand out (++num_added_points3D_, starting at next_point3D_id; 0 = the largest
    id + 1), in the order of the merge events of the sequential run -- an intermediate merged point that is merged again
    consumes an id too;
  * Complete does not read the camera-bogus cache across calls: the verdict is computed per camera;
  * Complete rotates by qvec / tvec (CalculateSquaredReprojectionError's quaternion overload), as point_filter restates it;
  * a selected id that is merged away earlier in the same call is skipped (ExistsPoint3D); merged ids are never in a selection;
  * invalid input follows DESIGN.md 13; a feature in two tracks and complete_max_transitivity < 1 are invalid as well.

Counts.  step_counts are num_completed / num_merged as the reference returns them.  complete_trials counts the reprojection
tests Complete evaluates (a candidate in a registered image, without a point, on a camera that passes), merge_trials the pairs
Merge enters into merge_trials_.  Margins are relative, as point_filter's report: every compared value against its threshold."""
import math

import numpy as np

from tests import point_filter_ref as pf
from tests import retriangulation_ref as rt

MERGE, COMPLETE = 0, 1
EPS, DBL_MAX = pf.EPS, pf.DBL_MAX


def default_options(**kw):
    o = dict(complete_max_reproj_error=4.0, merge_max_reproj_error=4.0, complete_max_transitivity=5, min_focal_length_ratio=0.1,
             max_focal_length_ratio=10.0, max_extra_param=1.0)
    o.update(kw)
    return o


class State:
    """The reconstruction as the two functions see it."""

    def __init__(self, scene, next_point3D_id=0, **options):
        self.o = default_options(**options)
        if self.o["complete_max_transitivity"] < 1:
            raise ValueError("complete_max_transitivity < 1")
        sc = rt.Scene(scene)
        self.sc = sc
        self.corrs = rt.build_graph(sc)
        self.image_ids = [int(i) for i in scene["image_ids"]]
        self.reg = [bool(r) for r in scene["registered"]]
        self.R, _ = pf.image_poses(scene["qvec"], scene["tvec"])
        self.t = np.asarray(scene["tvec"], np.float64).reshape(-1, 3)
        self.mg = {"error": math.inf, "depth": math.inf, "bogus": math.inf}
        bm = [math.inf]
        self.cam = []
        self.cam_bogus = []
        for i in range(len(self.image_ids)):
            c = sc.camera(i)
            tup = (int(c.model_id), np.array(c.params[:pf.NUM_PARAMS[c.model_id]], np.float64), int(c.width), int(c.height))
            self.cam.append(tup)
            self.cam_bogus.append(pf.has_bogus_params(tup, self.o, bm))
        self.mg["bogus"] = bm[0]
        ids = [int(i) for i in np.asarray(scene["point3D_ids"], np.uint64).reshape(-1)]
        xyz = np.asarray(scene["point3D_xyz"], np.float64).reshape(-1, 3)
        toff = np.asarray(scene["track_offsets"], np.int64).reshape(-1)
        tobs = np.asarray(scene["track_obs"], np.int64).reshape(-1, 2)
        if len(set(ids)) != len(ids):
            raise ValueError("a repeated point3D id")
        self.points = {}
        self.f2p = {}
        for k, pid in enumerate(ids):
            track = []
            for im, idx in tobs[toff[k]:toff[k + 1]]:
                f = (sc.img_of_id[int(im)], int(idx))
                if f in self.f2p:
                    raise ValueError("a feature in two tracks")
                self.f2p[f] = pid
                track.append(f)
            self.points[pid] = [xyz[k].copy(), track]
        self.next_id = int(next_point3D_id) if next_point3D_id else (max(ids) + 1 if ids else 1)
        if ids and self.next_id <= max(ids):
            raise ValueError("next_point3D_id at or below an existing id")
        self.modified = set()
        self.complete_trials = 0
        self.merge_trials = 0
        self.merge_memo = {}

    # CalculateSquaredReprojectionError (projection.cc:119-136), the quaternion overload, in point_filter's operation order
    def sq_error(self, f, X):
        i, k = f
        T, t = self.R[i], self.t[i]
        px = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + t[0]
        py = ((T[3] * X[0] + T[4] * X[1]) + T[5] * X[2]) + t[1]
        pz = ((T[6] * X[0] + T[7] * X[1]) + T[8] * X[2]) + t[2]
        self.mg["depth"] = min(self.mg["depth"], pf.margin(float(pz), EPS))
        if pz < EPS:
            return DBL_MAX
        m, pr, _, _ = self.cam[i]
        x, y = pf.world_to_image(m, pr, np.float64(px / pz), np.float64(py / pz))
        xy = self.sc.xy[self.sc.off[i] + k]
        dx, dy = np.float64(x) - xy[0], np.float64(y) - xy[1]
        return float(dx * dx + dy * dy)

    def within(self, f, X, thr2):
        e = self.sq_error(f, X)
        if e != DBL_MAX:
            self.mg["error"] = min(self.mg["error"], pf.margin(e, thr2))
        return not e > thr2

    def complete(self, pid):
        num_completed = 0
        if pid not in self.points:
            return 0
        thr2 = self.o["complete_max_reproj_error"] * self.o["complete_max_reproj_error"]
        X, track = self.points[pid]
        queue = list(track)
        max_t = self.o["complete_max_transitivity"]
        for transitivity in range(max_t):
            if not queue:
                break
            prev_queue, queue = queue, []
            for el in prev_queue:
                for corr in self.corrs.get(el, []):
                    if not self.reg[corr[0]]:
                        continue
                    if corr in self.f2p:
                        continue
                    if self.cam_bogus[corr[0]]:
                        continue
                    self.complete_trials += 1
                    if not self.within(corr, X, thr2):
                        continue
                    track.append(corr)
                    self.f2p[corr] = pid
                    self.modified.add(pid)
                    if transitivity < max_t - 1:
                        queue.append(corr)
                    num_completed += 1
        return num_completed

    def merge(self, pid):
        if pid not in self.points:
            return 0
        thr2 = self.o["merge_max_reproj_error"] * self.o["merge_max_reproj_error"]
        X1, track1 = self.points[pid]
        for el in track1:
            for corr in self.corrs.get(el, []):
                if not self.reg[corr[0]]:
                    continue
                qid = self.f2p.get(corr)
                if qid is None or qid == pid or qid in self.merge_memo.setdefault(pid, set()):
                    continue
                X2, track2 = self.points[qid]
                self.merge_memo[pid].add(qid)
                self.merge_memo.setdefault(qid, set()).add(pid)
                self.merge_trials += 1
                n1, n2 = float(len(track1)), float(len(track2))
                merged = (n1 * X1 + n2 * X2) / float(len(track1) + len(track2))
                ok = True
                for tr in (track1, track2):
                    for f in tr:
                        if not self.within(f, merged, thr2):
                            ok = False
                            break
                    if not ok:
                        break
                if ok:
                    num_merged = len(track1) + len(track2)
                    mid = self.next_id  # MergePoints3D: the same mean again, track 1 then track 2, AddPoint3D's id
                    self.next_id += 1
                    del self.points[pid], self.points[qid]
                    self.points[mid] = [merged, track1 + track2]
                    for f in track1 + track2:
                        self.f2p[f] = mid
                    self.modified.discard(pid)
                    self.modified.discard(qid)
                    self.modified.add(mid)
                    rec = self.merge(mid)
                    return rec if rec > 0 else num_merged
        return 0

    def step(self, kind, selected=None):
        ids = sorted(self.points) if selected is None else sorted(int(s) for s in selected)
        if kind == MERGE:
            self.merge_memo = {}
            return sum(self.merge(p) for p in ids)
        if kind == COMPLETE:
            return sum(self.complete(p) for p in ids)
        raise ValueError("an unknown step")


def update_tracks(scene, steps, selected=None, next_point3D_id=0, **options):
    """The steps in order over one state.  Returns a dict: point_ids (ascending), xyz [n, 3], track_offsets [n + 1], track_obs
    [m, 2] ((image_id, point2D_idx) in track order), modified (ascending ids), step_counts, complete_trials, merge_trials, and
    margins (error, depth, bogus: the smallest relative margin of every decision taken)."""
    if selected is not None:
        selected = [int(s) for s in np.asarray(selected, np.uint64).reshape(-1)]
        if len(set(selected)) != len(selected):
            raise ValueError("a repeated selected id")
    st = State(scene, next_point3D_id, **options)
    if selected is not None and any(s not in st.points for s in selected):
        raise ValueError("a selected id that is no point")
    counts = [st.step(int(k), selected) for k in steps]
    ids = sorted(st.points)
    toff, obs = [0], []
    for p in ids:
        for i, k in st.points[p][1]:
            obs.append((st.image_ids[i], k))
        toff.append(len(obs))
    return {"point_ids": np.array(ids, np.uint64), "xyz": np.array([st.points[p][0] for p in ids], np.float64).reshape(-1, 3),
            "track_offsets": np.array(toff, np.uint64), "track_obs": np.array(obs, np.uint32).reshape(-1, 2),
            "modified": np.array(sorted(st.modified), np.uint64), "step_counts": np.array(counts, np.uint64),
            "complete_trials": st.complete_trials, "merge_trials": st.merge_trials, "margins": dict(st.mg)}


def min_margin(out):
    return min(out["margins"].values())
