// track_update.h -- the exact pieces of IncrementalTriangulator::Complete and Merge (src/sfm/incremental_triangulator.cc:588-746)
// and Reconstruction::MergePoints3D (src/base/reconstruction.cc:215-241), once, for the kernels of track_update.hip and for the
// host build libdsm_track_update_host.so.  The includer defines TU_HD (the function qualifier), TU_HD_MEMBER (the same for a member function) and
// TU_FETCH_INC(ptr) (a counter handed out: an integer atomic on the device, a plain increment on the host), and includes
// ba_project.h first (the forward camera model).
//
// State.  Every feature (point2D) is in at most one track, so a track is a linked list through the features: fnext[f] is the
// next element, a point keeps head, tail and length.  AddObservation appends one link, MergePoints3D links track 2 behind
// track 1: no allocation grows with the number of completions or merges.  A point is a slot: the input points in ascending id
// are the slots 0 .. P - 1, a merge event takes the next free slot (at most P - 1 of them: every event leaves one point less).
//
// Merge's memo without a table.  merge_trials_ (cleared per MergeTracks call) only ever answers "was {a, b} tried before",
// and inside one call no existing point changes (points are created and deleted, never edited).  A point is the outer point of
// Merge at most once per call (selected ids are unique, a merged point is entered once, by the recursion).  So when Merge(a)
// meets b, {a, b} is in the memo exactly when (i) a itself tried b earlier in this loop (stamp[b] == a), or (ii) b has run its
// own loop to the end without a merge while a already existed (done[b] > born[a], on the component's event clock): that loop
// met a over the same links and tried it, or skipped it because the memo held the pair.  O(1) per point, no bound to exceed.
#ifndef DAGSFM_AMD_CSRC_TRACK_UPDATE_H_
#define DAGSFM_AMD_CSRC_TRACK_UPDATE_H_

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dagsfm_mi355x.h"

#define TU_NIL 0xffffffffu
#define TU_POSE 12  // doubles per image: R (row-major) of the normalised quaternion, then tvec

struct TuMargins {
  double complete_error, merge_error, depth;
};

// what the walks read and write; one copy of the pointers goes to every kernel
struct TuView {
  uint32_t N, P, S;  // images, input points, slots (2 P - 1, at least 1)
  uint64_t F;        // features
  // the scene, read only
  const dsm_camera* cams;
  const uint32_t* img_cam;    // [N] camera index
  const uint8_t* img_reg;     // [N] Image::IsRegistered
  const uint8_t* img_bogus;   // [N] the camera's HasBogusParams verdict
  const double* pose;         // [N][TU_POSE]
  const uint32_t* feat_img;   // [F]
  const double* xy;           // [F][2]
  const uint32_t* goff;       // [F + 1] the correspondence lists (CSR, the reference's append order)
  const uint32_t* gval;
  double thr2_complete, thr2_merge;
  int32_t max_transitivity;
  // the state
  int32_t* f2p;      // [F] the slot of the feature's point, or -1
  uint32_t* fnext;   // [F]
  double* xyz;       // [S][3]
  uint32_t* head;    // [S]
  uint32_t* tail;
  uint32_t* len;
  uint8_t* alive;    // ExistsPoint3D
  uint8_t* modified; // modified_point3D_ids_ as these steps change it
  uint32_t* stamp;   // [S] the memo of one MERGE step, see above
  uint32_t* born;
  uint32_t* done;
  uint32_t* num_slots;  // slots handed out so far (starts at P)
  uint32_t* ev_pos;     // [S] per merged slot: the position of the outer point in the step's list, and the recursion depth
  uint32_t* ev_depth;
};

TU_HD double tu_margin(double a, double thr) {
  if (!isfinite(a)) return INFINITY;
  const double den = fmax(fabs(a), fabs(thr));
  return den > 0.0 ? fabs(a - thr) / den : 0.0;
}

// CalculateSquaredReprojectionError (projection.cc:119-136, the quaternion overload) of feature f against X, in
// point_filter.hip's operation order; the verdict `not above thr2`
TU_HD bool tu_within(const TuView& v, uint32_t f, const double* X, double thr2, double* mg_err, double* mg_depth) {
  const uint32_t img = v.feat_img[f];
  const double* T = v.pose + (size_t)TU_POSE * img;
  const double px = ((T[0] * X[0] + T[1] * X[1]) + T[2] * X[2]) + T[9];
  const double py = ((T[3] * X[0] + T[4] * X[1]) + T[5] * X[2]) + T[10];
  const double pz = ((T[6] * X[0] + T[7] * X[1]) + T[8] * X[2]) + T[11];
  *mg_depth = fmin(*mg_depth, tu_margin(pz, DBL_EPSILON));
  if (pz < DBL_EPSILON) return !(DBL_MAX > thr2);
  const dsm_camera* cam = v.cams + v.img_cam[img];
  double x, y;
  ba_world_to_image<double>(cam->model_id, cam->params, px / pz, py / pz, &x, &y);
  const double dx = x - v.xy[2 * (size_t)f], dy = y - v.xy[2 * (size_t)f + 1];
  const double e2 = dx * dx + dy * dy;
  *mg_err = fmin(*mg_err, tu_margin(e2, thr2));
  return !(e2 > thr2);
}

// AddObservation: f behind the track of slot
TU_HD void tu_append(const TuView& v, uint32_t slot, uint32_t f) {
  v.fnext[f] = TU_NIL;
  if (v.len[slot] == 0)
    v.head[slot] = f;
  else
    v.fnext[v.tail[slot]] = f;
  v.tail[slot] = f;
  v.len[slot] += 1;
  v.f2p[f] = (int32_t)slot;
  v.modified[slot] = 1;
}

// Complete(slot) straight on the state: the reference's loops.  The queue of a level is a run of the track's own list -- the
// elements the level before appended (all of them while transitivity < max - 1, none at the last level).
TU_HD uint32_t tu_complete(const TuView& v, uint32_t slot, TuMargins* mg, uint64_t* trials) {
  if (!v.alive[slot]) return 0;
  const double X[3] = {v.xyz[3 * (size_t)slot], v.xyz[3 * (size_t)slot + 1], v.xyz[3 * (size_t)slot + 2]};
  uint32_t qbeg = v.head[slot], qcount = v.len[slot], num_completed = 0;
  for (int32_t t = 0; t < v.max_transitivity; ++t) {
    if (qcount == 0) break;
    uint32_t nbeg = TU_NIL, ncount = 0, e = qbeg;
    for (uint32_t i = 0; i < qcount; ++i) {
      for (uint32_t c = v.goff[e]; c < v.goff[e + 1]; ++c) {
        const uint32_t g = v.gval[c], img = v.feat_img[g];
        if (!v.img_reg[img]) continue;
        if (v.f2p[g] >= 0) continue;
        if (v.img_bogus[img]) continue;
        ++*trials;
        if (!tu_within(v, g, X, v.thr2_complete, &mg->complete_error, &mg->depth)) continue;
        tu_append(v, slot, g);
        if (t < v.max_transitivity - 1) {
          if (ncount == 0) nbeg = g;
          ++ncount;
        }
        ++num_completed;
      }
      e = v.fnext[e];
    }
    qbeg = nbeg;
    qcount = ncount;
  }
  return num_completed;
}

// The all-elements test of Merge with its early break, one element after the other: track 1, then track 2
struct TuSerialTest {
  TU_HD_MEMBER bool operator()(const TuView& v, uint32_t cur, uint32_t q, const double* M, TuMargins* mg) const {
    bool ok = true;
    for (uint32_t f = v.head[cur]; f != TU_NIL && ok; f = v.fnext[f]) ok = tu_within(v, f, M, v.thr2_merge, &mg->merge_error, &mg->depth);
    for (uint32_t f = v.head[q]; f != TU_NIL && ok; f = v.fnext[f]) ok = tu_within(v, f, M, v.thr2_merge, &mg->merge_error, &mg->depth);
    return ok;
  }
  TU_HD_MEMBER uint32_t take_slot(uint32_t* num_slots) const { return TU_FETCH_INC(num_slots); }
};

// Merge(slot) with its recursion unrolled into a loop: the outer point of pass d + 1 is the point pass d created.  pos: the
// position of slot in the step's list (the event key).  *clock: the event clock of the caller's run (one per component, or
// one for a serial run); it must start at 1.  all_inliers: the all-elements test and the hand-out of the new slot (TuSerialTest, or the wave's form).  Returns what the reference returns: the track length of the last merge.
template <class Tester>
TU_HD uint32_t tu_merge(const TuView& v, uint32_t slot, uint32_t pos, uint32_t* clock, TuMargins* mg, uint64_t* trials, uint64_t* events,
                        const Tester& all_inliers) {
  if (!v.alive[slot]) return 0;
  uint32_t cur = slot, depth = 0, result = 0;
  for (;;) {
    bool merged = false;
    const uint32_t n1 = v.len[cur];
    const double* X1 = v.xyz + 3 * (size_t)cur;
    for (uint32_t e = v.head[cur]; e != TU_NIL && !merged; e = v.fnext[e]) {
      for (uint32_t c = v.goff[e]; c < v.goff[e + 1]; ++c) {
        const uint32_t g = v.gval[c];
        if (!v.img_reg[v.feat_img[g]]) continue;
        const int32_t qs = v.f2p[g];
        if (qs < 0 || (uint32_t)qs == cur) continue;
        const uint32_t q = (uint32_t)qs;
        if (v.stamp[q] == cur || v.done[q] > v.born[cur]) continue;  // merge_trials_[cur].count(q) > 0
        v.stamp[q] = cur;
        ++*trials;
        const uint32_t n2 = v.len[q];
        const double* X2 = v.xyz + 3 * (size_t)q;
        double M[3];
        for (int k = 0; k < 3; ++k) M[k] = ((double)n1 * X1[k] + (double)n2 * X2[k]) / (double)(n1 + n2);
        if (!all_inliers(v, cur, q, M, mg)) continue;
        const uint32_t m = all_inliers.take_slot(v.num_slots);
        if (m >= v.S) return result;  // cannot happen: every event leaves one point less (kept as a bound on the stores)
        // MergePoints3D: the same mean, track 1 then track 2, both inputs deleted
        for (int k = 0; k < 3; ++k) v.xyz[3 * (size_t)m + k] = M[k];
        v.fnext[v.tail[cur]] = v.head[q];
        v.head[m] = v.head[cur];
        v.tail[m] = v.tail[q];
        v.len[m] = n1 + n2;
        for (uint32_t f = v.head[m]; f != TU_NIL; f = v.fnext[f]) v.f2p[f] = (int32_t)m;
        v.alive[cur] = v.alive[q] = 0;
        v.modified[cur] = v.modified[q] = 0;
        v.alive[m] = 1;
        v.modified[m] = 1;
        v.stamp[m] = TU_NIL;
        v.done[m] = 0;
        v.born[m] = ++*clock;
        v.ev_pos[m] = pos;
        v.ev_depth[m] = depth;
        ++*events;
        result = n1 + n2;
        cur = m;
        ++depth;
        merged = true;
        break;
      }
    }
    if (!merged) {
      v.done[cur] = ++*clock;
      break;
    }
  }
  return result;
}

#endif  // DAGSFM_AMD_CSRC_TRACK_UPDATE_H_
