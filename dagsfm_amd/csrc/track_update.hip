// track_update.hip -- IncrementalTriangulator::CompleteTracks / MergeTracks on the device: dsm_update_tracks.
// The exact pieces (the reprojection test, Complete's level walk, Merge with MergePoints3D) are track_update.h's, shared with the
// host build; the arguments are validated and laid out by track_update_load.h.  The state (feature -> point, the tracks as lists
// through the features, xyz, alive / modified per slot) stays on the device between the steps of a call.
//
//   graph       rt_graph.h: the duplicate rule and the CSR lists of dsm_retriangulate, unchanged
//   COMPLETE    rounds over the step's list (rank = position in the list); a pending point walks on one lane (k_tu_speculate)
//               up to TU_LANE_CUT track elements and on a wave above (k_tu_speculate_wave: a lane per (queue element,
//               correspondence) candidate, ballot / prefix compaction in the reference's order):
//     k_tu_speculate  the point's level walk against the committed state; what it tests goes to a list of its own in a shared
//                     pool, and every tested / accepted feature is marked with an integer atomicMin of (round tag, rank)
//     k_tu_commit     a point whose list meets no mark of a lower rank (see there) appends what it accepted to its track and
//                     is done; the others stay pending.  The host reads (pending, pool overflow) once per round.
//     A pool that runs out ends the claim rounds: the rest of the step runs in k_tu_complete_serial (one lane, the reference's
//     loops), counted in the report.  No floating-point atomics.
//   MERGE       k_tu_hook / k_tu_label  connected components of the points by integer hooking (compare-and-swap on a parent
//                     array, roots only decrease) over the links "an element of P has a correspondence in a registered image to a
//                     feature of Q"; the host buckets the step's list by component (a stable counting pass);
//     k_tu_merge      a component runs its points in list order through tu_merge: on one lane when its tracks hold at most
//                     TU_WAVE_ELEMS elements (k_tu_merge_lane), else on a wave with a lane per track element of the two
//                     tracks in the all-inlier test; every merge event records (position
//                     of its outer point, depth), and the host numbers the events in one ordered pass.
//   output      k_tu_emit writes the tracks out in ascending id.
// The check build's DSM_TRACK_UPDATE_SERIAL=1 runs both steps on one lane; =pool:<n> limits the claim pool to n entries.
//
// dsm_complete_images is the same driver with IncrementalTriangulator::CompleteImage of a list of images behind
// the steps, over the same state:
//   k_ci_find      per (listed image, point2D) item: is it a candidate for a new point, and how long is its estimation list
//   k_ci_estimate  EstimateTriangulation (rt_loransac.h with the reprojection residual) of every candidate, a lane each
//   k_ci_commit    the reference's loop in its order on one lane: Complete's walk, the skips, the estimates' results, AddPoint3D
// The check build's DSM_COMPLETE_IMAGE_SERIAL=1 leaves every estimate to the commit lane; =pool:<n> limits the estimates that
// run ahead to n list entries.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ba_project.h"
#include "ctx.h"
#include "rt_graph.h"
#include "rt_loransac.h"

#define TU_HD __device__ inline
#define TU_HD_MEMBER __device__ inline
#define TU_FETCH_INC(ptr) atomicAdd((ptr), 1u)
#include "track_update_load.h"
#include "wave_reduce.h"

namespace {

constexpr int TU_BLOCK = 256;
// Tracks up to this many elements walk their levels on one lane, longer ones on a wave (point_filter.hip's split and its value;
// not measured here).  The split reads the committed track length, which no kernel of a round changes before the commit.
constexpr uint32_t TU_LANE_CUT = 16;
constexpr uint32_t TU_WAVE_ELEMS = 32;  // a component's track elements up to which it runs on a lane (not measured finer than DESIGN.md 31)
constexpr uint32_t TU_OWN_CAP = 2048;  // features one wave walk can accept (its list in LDS); more ends the rounds like a full pool
constexpr uint32_t TU_REJECTED = 0x80000000u;  // a pool entry the walk tested and rejected (feature indices stay below 2^30)
enum { TU_C_PENDING = 0, TU_C_OVERFLOW = 1, TU_C_POOL = 2, TU_C_WORDS = 4 };                      // uint32 round counters
enum { TU_A_CTRIALS = 0, TU_A_MTRIALS = 1, TU_A_EVENTS = 2, TU_A_MG = 3, TU_A_STEPS = 6 };  // uint64 accumulators

struct TuDev {
  TuView v;
  // COMPLETE
  unsigned long long* claim;  // [F] (round tag << 32) | rank of the lowest rank that accepted the feature in the round; smaller wins
  unsigned long long* tested; // [F] the same of the lowest rank that tested it (accepted or rejected)
  uint32_t* pool_feat;        // [pool_cap] accepted features of the speculative walks
  uint32_t* pool_next;
  uint32_t pool_cap;
  uint32_t* spec_head;        // [list] per pending point: its list in the pool, its length, its trials
  uint32_t* spec_count;
  uint32_t* spec_trials;
  uint8_t* pending;           // [list]
  uint32_t* ctr;              // [TU_C_WORDS]
  unsigned long long* acc;    // [TU_A_STEPS + num_steps]
  // MERGE
  uint32_t* parent;           // [S]
};

__device__ inline void tu_fold_margins(unsigned long long* acc, const TuMargins& mg) {
  // non-negative doubles order like their bit patterns
  atomicMin(&acc[TU_A_MG + 0], (unsigned long long)__double_as_longlong(mg.complete_error));
  atomicMin(&acc[TU_A_MG + 1], (unsigned long long)__double_as_longlong(mg.merge_error));
  atomicMin(&acc[TU_A_MG + 2], (unsigned long long)__double_as_longlong(mg.depth));
}

// Complete's walk of one pending point against the committed state.  Every candidate it tests goes to a list of its own in the
// pool, in walk order: an accepted feature as it is, a rejected one with TU_REJECTED set.  The queue of a level is a run of the
// point's list: its track at level 0, the accepted pool entries of the level before afterwards.
__global__ void __launch_bounds__(TU_BLOCK) k_tu_speculate(TuDev d, const uint32_t* __restrict__ list, uint32_t n, uint32_t tag) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i >= n || !d.pending[i]) return;
  const TuView& v = d.v;
  const uint32_t slot = list[i];
  if (v.alive[slot] && v.len[slot] > TU_LANE_CUT) return;  // k_tu_speculate_wave's
  d.spec_head[i] = TU_NIL;
  d.spec_count[i] = 0;
  d.spec_trials[i] = 0;
  if (!v.alive[slot]) return;
  const double X[3] = {v.xyz[3 * (size_t)slot], v.xyz[3 * (size_t)slot + 1], v.xyz[3 * (size_t)slot + 2]};
  const unsigned long long mine = ((unsigned long long)tag << 32) | i;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  uint32_t qbeg = v.head[slot], qcount = v.len[slot], head = TU_NIL, last = TU_NIL, count = 0, trials = 0;
  bool in_pool = false, overflow = false;
  for (int32_t t = 0; t < v.max_transitivity && qcount && !overflow; ++t) {
    uint32_t nbeg = TU_NIL, ncount = 0, e = qbeg;
    for (uint32_t k = 0; k < qcount && !overflow;) {
      uint32_t f = e;
      if (in_pool) {
        f = d.pool_feat[e];
        if (f & TU_REJECTED) {  // not a queue element
          e = d.pool_next[e];
          continue;
        }
      }
      for (uint32_t c = v.goff[f]; c < v.goff[f + 1]; ++c) {
        const uint32_t g = v.gval[c], img = v.feat_img[g];
        if (!v.img_reg[img]) continue;
        if (v.f2p[g] >= 0) continue;
        bool own = false;  // AddObservation earlier in this walk: HasPoint3D
        for (uint32_t x = head; x != TU_NIL && !own; x = d.pool_next[x]) own = d.pool_feat[x] == g;
        if (own) continue;
        if (v.img_bogus[img]) continue;
        ++trials;
        const bool ok = tu_within(v, g, X, v.thr2_complete, &mg.complete_error, &mg.depth);
        const uint32_t at = atomicAdd(&d.ctr[TU_C_POOL], 1u);
        if (at >= d.pool_cap) {
          overflow = true;
          break;
        }
        atomicMin(&d.tested[g], mine);
        d.pool_feat[at] = ok ? g : (g | TU_REJECTED);
        d.pool_next[at] = TU_NIL;
        if (head == TU_NIL)
          head = at;
        else
          d.pool_next[last] = at;
        last = at;
        if (!ok) continue;
        ++count;
        atomicMin(&d.claim[g], mine);
        if (t < v.max_transitivity - 1) {
          if (ncount == 0) nbeg = at;
          ++ncount;
        }
      }
      e = in_pool ? d.pool_next[e] : v.fnext[e];
      ++k;
    }
    qbeg = nbeg;
    qcount = ncount;
    in_pool = true;
  }
  if (overflow) atomicExch(&d.ctr[TU_C_OVERFLOW], 1u);
  d.spec_head[i] = head;
  d.spec_count[i] = count;
  d.spec_trials[i] = trials;
  tu_fold_margins(d.acc, mg);
}

// the positions of the step's list whose points walk on a wave: alive, more than TU_LANE_CUT track elements.  Built once per
// COMPLETE step: a pending point's track does not change before it commits.  The order of the list does not matter (a point's
// rank is its position in the step's list, which is what the entry holds).
__global__ void __launch_bounds__(TU_BLOCK) k_tu_wave_list(TuDev d, const uint32_t* __restrict__ list, uint32_t n, uint32_t* __restrict__ wlist,
                                                           uint32_t* __restrict__ wcount) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i >= n) return;
  const uint32_t slot = list[i];
  if (d.v.alive[slot] && d.v.len[slot] > TU_LANE_CUT) wlist[atomicAdd(wcount, 1u)] = i;
}

// The same walk for a long track, one wave per point.  The 64 lanes take 64 correspondences of a queue element at a time: a lane
// per (queue element, correspondence) candidate runs the reference's tests in their order, the tested and the accepted
// candidates are compacted by ballot and prefix count, so the point's pool list and its accepted list (in LDS: the queue of the
// next level is a run of it) are in the reference's order.  The correspondences of one feature lie in different images, so a
// chunk holds no feature twice; a feature reached again through a later queue element meets the accepted list.
__global__ void __launch_bounds__(64) k_tu_speculate_wave(TuDev d, const uint32_t* __restrict__ list, const uint32_t* __restrict__ wlist,
                                                           uint32_t nw, uint32_t tag) {
  __shared__ uint32_t own[TU_OWN_CAP];
  if (blockIdx.x >= nw) return;
  const uint32_t i = wlist[blockIdx.x];
  const uint32_t lane = threadIdx.x;
  if (!d.pending[i]) return;
  const TuView& v = d.v;
  const uint32_t slot = list[i];
  if (!v.alive[slot] || v.len[slot] <= TU_LANE_CUT) return;  // k_tu_speculate's
  const double X[3] = {v.xyz[3 * (size_t)slot], v.xyz[3 * (size_t)slot + 1], v.xyz[3 * (size_t)slot + 2]};
  const unsigned long long mine = ((unsigned long long)tag << 32) | i;
  const unsigned long long lower = (1ull << lane) - 1ull;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  uint32_t head = TU_NIL, last = TU_NIL, count = 0, trials = 0, qlo = 0, qhi = 0;
  bool overflow = false;
  for (int32_t t = 0; t < v.max_transitivity && !overflow; ++t) {
    const uint32_t nq = t == 0 ? v.len[slot] : qhi - qlo, level_lo = count;
    if (nq == 0) break;
    uint32_t e = v.head[slot];
    for (uint32_t k = 0; k < nq && !overflow; ++k) {
      const uint32_t f = t == 0 ? e : own[qlo + k];
      const uint32_t c0 = v.goff[f], c1 = v.goff[f + 1];
      for (uint32_t base = c0; base < c1; base += 64) {
        const uint32_t c = base + lane;
        uint32_t g = 0, img = 0;
        bool cand = false, ok = false;
        if (c < c1) {
          g = v.gval[c];
          img = v.feat_img[g];
          cand = v.img_reg[img] && v.f2p[g] < 0;
        }
        if (cand)  // AddObservation earlier in this walk: HasPoint3D
          for (uint32_t x = 0; x < count; ++x)
            if (own[x] == g) {
              cand = false;
              break;
            }
        if (cand && v.img_bogus[img]) cand = false;
        if (cand) ok = tu_within(v, g, X, v.thr2_complete, &mg.complete_error, &mg.depth);
        const unsigned long long tmask = __ballot(cand), amask = __ballot(ok);
        const uint32_t nt = (uint32_t)__popcll(tmask), na = (uint32_t)__popcll(amask);
        if (nt == 0) continue;
        uint32_t at0 = 0;
        if (lane == 0) at0 = atomicAdd(&d.ctr[TU_C_POOL], nt);
        at0 = (uint32_t)__shfl((int)at0, 0);
        if ((uint64_t)at0 + nt > d.pool_cap || count + na > TU_OWN_CAP) {
          overflow = true;
          break;
        }
        if (cand) {
          const uint32_t at = at0 + (uint32_t)__popcll(tmask & lower);
          d.pool_feat[at] = ok ? g : (g | TU_REJECTED);
          if (at + 1 < at0 + nt) d.pool_next[at] = at + 1;  // the chunk's last entry is linked by the next chunk, or closed at the end
          atomicMin(&d.tested[g], mine);
          if (ok) {
            atomicMin(&d.claim[g], mine);
            own[count + (uint32_t)__popcll(amask & lower)] = g;
          }
        }
        if (lane == 0 && head != TU_NIL) d.pool_next[last] = at0;
        if (head == TU_NIL) head = at0;
        last = at0 + nt - 1;
        count += na;
        trials += nt;
        __syncthreads();  // the accepted list, before the next chunk's lanes read it
      }
      if (t == 0) e = v.fnext[e];
    }
    qlo = level_lo;
    qhi = t < v.max_transitivity - 1 ? count : level_lo;
  }
  mg.complete_error = wave_fmin(mg.complete_error);
  mg.depth = wave_fmin(mg.depth);
  if (lane != 0) return;
  if (head != TU_NIL) d.pool_next[last] = TU_NIL;
  if (overflow) atomicExch(&d.ctr[TU_C_OVERFLOW], 1u);
  d.spec_head[i] = head;
  d.spec_count[i] = count;
  d.spec_trials[i] = trials;
  tu_fold_margins(d.acc, mg);
}

// The issue's rule is "a point commits when it holds every claim of its list"; this is deliberately stronger, because the
// trial counts are compared too: a higher rank taking a feature a lower rank tested and rejected leaves the tracks right and that
// rank's trial count one short (DESIGN.md 31 has the proof for the rule as it stands).
// A point commits when no lower rank of the round tested a feature it accepted (taking it would change that rank's walk, or
// at least its trial count) and no lower rank accepted a feature it rejected (the sequential run would not have tested that
// one).  A round in which a walk ran out of pool commits nothing: a truncated list of a lower rank is not the superset the
// argument needs.
__global__ void __launch_bounds__(TU_BLOCK) k_tu_commit(TuDev d, const uint32_t* __restrict__ list, uint32_t n, uint32_t tag, uint32_t step) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i >= n || !d.pending[i]) return;
  if (d.ctr[TU_C_OVERFLOW]) return;
  const TuView& v = d.v;
  const unsigned long long mine = ((unsigned long long)tag << 32) | i;
  bool holds = true;
  for (uint32_t x = d.spec_head[i]; x != TU_NIL && holds; x = d.pool_next[x]) {
    const uint32_t g = d.pool_feat[x];
    holds = (g & TU_REJECTED) ? d.claim[g & ~TU_REJECTED] >= mine : d.tested[g] == mine;
  }
  if (!holds) {
    atomicAdd(&d.ctr[TU_C_PENDING], 1u);
    return;
  }
  const uint32_t slot = list[i];
  for (uint32_t x = d.spec_head[i]; x != TU_NIL; x = d.pool_next[x])
    if (!(d.pool_feat[x] & TU_REJECTED)) tu_append(v, slot, d.pool_feat[x]);
  d.pending[i] = 0;
  if (d.spec_count[i]) atomicAdd(&d.acc[TU_A_STEPS + step], (unsigned long long)d.spec_count[i]);
  if (d.spec_trials[i]) atomicAdd(&d.acc[TU_A_CTRIALS], (unsigned long long)d.spec_trials[i]);
}

// the reference's loops over what is still pending, on one lane
__global__ void k_tu_complete_serial(TuDev d, const uint32_t* __restrict__ list, uint32_t n, uint32_t step) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  uint64_t trials = 0, count = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!d.pending[i]) continue;
    count += tu_complete(d.v, list[i], &mg, &trials);
    d.pending[i] = 0;
  }
  atomicAdd(&d.acc[TU_A_STEPS + step], (unsigned long long)count);
  atomicAdd(&d.acc[TU_A_CTRIALS], (unsigned long long)trials);
  tu_fold_margins(d.acc, mg);
}

__device__ inline uint32_t tu_find(const uint32_t* parent, uint32_t x) {
  for (;;) {
    const uint32_t p = __atomic_load_n(&parent[x], __ATOMIC_RELAXED);
    if (p == x) return x;
    x = p;
  }
}

__global__ void __launch_bounds__(TU_BLOCK) k_tu_parent_init(uint32_t S, uint32_t* __restrict__ parent) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i < S) parent[i] = i;
}

// a lane per feature: its point hooked to the point of every correspondence in a registered image; the larger root goes
// under the smaller by compare-and-swap, so parents only decrease and no cycle can form
__global__ void __launch_bounds__(TU_BLOCK) k_tu_hook(TuDev d) {
  const TuView& v = d.v;
  const uint64_t f = (uint64_t)blockIdx.x * TU_BLOCK + threadIdx.x;
  if (f >= v.F) return;
  const int32_t p = v.f2p[f];
  if (p < 0) return;
  for (uint32_t c = v.goff[f]; c < v.goff[f + 1]; ++c) {
    const uint32_t g = v.gval[c];
    if (!v.img_reg[v.feat_img[g]]) continue;
    const int32_t q = v.f2p[g];
    if (q < 0 || q == p) continue;
    uint32_t a = (uint32_t)p, b = (uint32_t)q;
    for (;;) {
      a = tu_find(d.parent, a);
      b = tu_find(d.parent, b);
      if (a == b) break;
      if (a < b) {
        const uint32_t t = a;
        a = b;
        b = t;
      }
      if (atomicCAS(&d.parent[a], a, b) == a) break;
    }
  }
}

__global__ void __launch_bounds__(TU_BLOCK) k_tu_label(uint32_t S, const uint32_t* __restrict__ parent, uint32_t* __restrict__ label) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i < S) label[i] = tu_find(parent, i);
}

// The all-elements test of Merge on a wave: the lanes walk the two tracks together (the same loads in every lane), lane k keeps
// the k-th element of a run of 64 and tests it; the verdict is an AND over independent tests, so the reference's early break
// only decides which margins count: those up to the first failing element.
struct TuWaveTest {
  __device__ inline bool operator()(const TuView& v, uint32_t cur, uint32_t q, const double* M, TuMargins* mg) const {
    const uint32_t lane = threadIdx.x;
    uint32_t f = v.head[cur];
    int second = 0;
    for (;;) {
      uint32_t mine = TU_NIL, n = 0;
      while (n < 64) {
        if (f == TU_NIL) {
          if (second) break;
          second = 1;
          f = v.head[q];
          continue;
        }
        if (n == lane) mine = f;
        f = v.fnext[f];
        ++n;
      }
      if (n == 0) return true;
      double le = INFINITY, ld = INFINITY;
      bool in = true;
      if (mine != TU_NIL) in = tu_within(v, mine, M, v.thr2_merge, &le, &ld);
      const unsigned long long fail = __ballot(!in);
      const uint32_t stop = fail ? (uint32_t)__ffsll((long long)fail) - 1 : 63u;
      if (lane > stop) le = ld = INFINITY;
      mg->merge_error = fmin(mg->merge_error, wave_fmin(le));
      mg->depth = fmin(mg->depth, wave_fmin(ld));
      if (fail) return false;
      if (n < 64) return true;
    }
  }
  // every lane runs Merge with the same values: lane 0 takes the counter, the others get its answer
  __device__ inline uint32_t take_slot(uint32_t* num_slots) const {
    uint32_t m = 0;
    if (threadIdx.x == 0) m = atomicAdd(num_slots, 1u);
    return (uint32_t)__shfl((int)m, 0);
  }
};

// A lane per component, for the components whose tracks hold few elements: the reference's loops as the host build runs them
__global__ void __launch_bounds__(TU_BLOCK) k_tu_merge_lane(TuDev d, const uint32_t* __restrict__ list, const uint32_t* __restrict__ comp_off,
                                                            const uint32_t* __restrict__ comp_pos, uint32_t ncomp, uint32_t step) {
  const uint32_t c = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (c >= ncomp) return;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  uint64_t trials = 0, events = 0, count = 0;
  uint32_t clock = 1;
  for (uint32_t k = comp_off[c]; k < comp_off[c + 1]; ++k) {
    const uint32_t pos = comp_pos[k];
    count += tu_merge(d.v, list[pos], pos, &clock, &mg, &trials, &events, TuSerialTest());
  }
  if (count) atomicAdd(&d.acc[TU_A_STEPS + step], (unsigned long long)count);
  if (trials) atomicAdd(&d.acc[TU_A_MTRIALS], (unsigned long long)trials);
  if (events) atomicAdd(&d.acc[TU_A_EVENTS], (unsigned long long)events);
  tu_fold_margins(d.acc, mg);
}

// A wave per component, for the others (components c0 .. ncomp - 1): positions comp_pos[comp_off[c] .. comp_off[c + 1]) of the step's list, ascending.  Every lane runs
// tu_merge with the same values and writes the same stores (a lane reads back what it wrote itself, so no lane depends on
// another's store); the all-elements test is the part the lanes share out (TuWaveTest), and lane 0 takes the counters.
__global__ void __launch_bounds__(64) k_tu_merge(TuDev d, const uint32_t* __restrict__ list, const uint32_t* __restrict__ comp_off,
                                                  const uint32_t* __restrict__ comp_pos, uint32_t c0, uint32_t ncomp, uint32_t step) {
  const uint32_t c = c0 + blockIdx.x;
  if (c >= ncomp) return;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  uint64_t trials = 0, events = 0, count = 0;
  uint32_t clock = 1;
  for (uint32_t k = comp_off[c]; k < comp_off[c + 1]; ++k) {
    const uint32_t pos = comp_pos[k];
    count += tu_merge(d.v, list[pos], pos, &clock, &mg, &trials, &events, TuWaveTest());
  }
  if (threadIdx.x != 0) return;
  if (count) atomicAdd(&d.acc[TU_A_STEPS + step], (unsigned long long)count);
  if (trials) atomicAdd(&d.acc[TU_A_MTRIALS], (unsigned long long)trials);
  if (events) atomicAdd(&d.acc[TU_A_EVENTS], (unsigned long long)events);
  tu_fold_margins(d.acc, mg);
}

// the tracks of the output points, (image_id, point2D_idx) per element at the host's offsets
__global__ void __launch_bounds__(TU_BLOCK) k_tu_emit(TuDev d, const uint32_t* __restrict__ out_slot, const uint64_t* __restrict__ out_off,
                                                      uint32_t n, const uint32_t* __restrict__ img_ids, const uint32_t* __restrict__ foff,
                                                      uint32_t* __restrict__ obs) {
  const uint32_t i = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (i >= n) return;
  const TuView& v = d.v;
  const uint32_t s = out_slot[i];
  uint64_t at = out_off[i];
  const uint64_t end = out_off[i + 1];
  for (uint32_t f = v.head[s]; f != TU_NIL && at < end; f = v.fnext[f], ++at) {
    const uint32_t img = v.feat_img[f];
    obs[2 * at] = img_ids[img];
    obs[2 * at + 1] = f - foff[img];
  }
}

// ------------------------------------------------------------------ CompleteImage
// An item is one (listed image, point2D) in (list position, point2D_idx) order.  What an item does depends on the state its
// predecessors leave (has its point2D a point, has a correspondence one), but what a creating item ESTIMATES does not: its
// list is Find's at transitivity 1 over the graph and the images' verdicts, the views are the scene's, and the only carried
// value (RANSACOptions::min_num_trials of a list above 15 entries) is checked at the commit.  So the estimates of all
// candidates run ahead, a lane each (k_ci_estimate), and one ordered pass (k_ci_commit) takes the reference's decisions in the
// reference's order on one lane: Complete's walk for a point2D with a point, the three skips, the estimate's result, AddPoint3D.
constexpr uint32_t CI_MAX_LIST = 8192;  // entries of one estimation list (the trial table grows with its square)
enum : uint8_t { CI_NOT_RUN = 0, CI_FAILED = 1, CI_OK = 2 };
enum { CI_A_RTRIALS = 0, CI_A_POINTS, CI_A_OBS, CI_A_SERIAL, CI_A_COMPLETED, CI_A_CTRIALS, CI_A_AHEAD, CI_A_ERROR, CI_A_MG, CI_A_WORDS = CI_A_MG + 4 };

// the camera's WorldToImage, one copy out of line for the residual inside LORANSAC
__device__ __noinline__ void ci_world_to_image(const dsm_camera* cam, double u, double v, double* x, double* y) {
  ba_world_to_image<double>(cam->model_id, cam->params, u, v, x, y);
}

// ResidualType::REPROJECTION_ERROR: CalculateSquaredReprojectionError, the projection-matrix overload (projection.cc:138-157)
struct RtReproj {
  const dsm_camera* cams;
  const uint32_t* img_cam;
  const uint32_t* feat_img;
  const double* xy;
  __device__ inline double operator()(const RtView& w, uint32_t f, const double* X, double max_residual, double* mg) const {
    const double z = rt_row(w.P, 2, X);
    if (mg) {
      const double m = tu_margin(z, DBL_EPSILON);
      if (m < mg[3]) mg[3] = m;
    }
    if (z < DBL_EPSILON) return DBL_MAX;
    const double x = rt_row(w.P, 0, X), y = rt_row(w.P, 1, X);
    const double inv = 1.0 / z;
    double px, py;
    ci_world_to_image(cams + img_cam[feat_img[f]], inv * x, inv * y, &px, &py);
    const double dx = px - xy[2 * (size_t)f], dy = py - xy[2 * (size_t)f + 1];
    const double r = dx * dx + dy * dy;
    if (mg) {
      const double m = tu_margin(r, max_residual);
      if (m < mg[0]) mg[0] = m;
    }
    return r;
  }
};

struct CiDev {
  uint32_t Q;                   // items
  uint32_t pool_cap;            // list entries the estimates that run ahead may hold
  const uint32_t* item_feat;    // [Q] the item's point2D as a feature
  const uint32_t* item_first;   // [Q] the first item of its image
  uint32_t* n_list;             // [Q] entries of the estimation list (correspondences kept by Find, then the point2D), 0: no candidate
  const uint32_t* loff;         // [Q + 1] the lists in the pool
  const uint8_t* img_ok;        // [N] registered, camera without bogus parameters
  const double* img_P;          // [N][12]
  const double* img_C;          // [N][3]
  const double* uv;             // [F][2] ImageToWorld
  const uint32_t* tab;          // ComputeNumTrials by (n, inliers), the host's libm
  const uint32_t* tab_off;
  RtParams prm;
  int32_t* clist;               // [pool] the lists, the level's positions (0 .. n - 1) and the inlier masks of the estimates
  int32_t* lvl;
  uint8_t* mask;
  uint8_t* est_state;           // [Q]
  double* est_xyz;              // [Q][3]
  uint32_t* est_trials;         // [Q]
  unsigned long long* est_min;  // [Q] the carried min_num_trials the estimate ran with (lists above 15 entries)
  int32_t* ser_clist;           // [longest list] the same for an estimate on the commit lane
  int32_t* ser_lvl;
  uint8_t* ser_mask;
  unsigned long long* acc;      // [CI_A_WORDS]
  unsigned long long* tris;     // [listed images]
};

__device__ inline bool ci_two_view(const TuView& v, uint32_t f) {  // CorrespondenceGraph::IsTwoViewObservation
  if (v.goff[f + 1] - v.goff[f] != 1) return false;
  const uint32_t g = v.gval[v.goff[f]];
  return v.goff[g + 1] - v.goff[g] == 1;
}

// A candidate is an item that can still create: its point2D has no point, it is no ignored two-view observation, Find keeps a
// correspondence and none of the kept ones has a point.  Features only ever gain points, so an item that is no candidate
// against the state the steps leave is none at its turn either.
__global__ void __launch_bounds__(TU_BLOCK) k_ci_find(TuDev d, CiDev c) {
  const uint32_t q = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (q >= c.Q) return;
  const TuView& v = d.v;
  const uint32_t f = c.item_feat[q];
  uint32_t n = 0;
  bool cand = v.f2p[f] < 0 && !(c.prm.ignore_two_view && ci_two_view(v, f));
  for (uint32_t e = v.goff[f]; e < v.goff[f + 1] && cand; ++e) {
    const uint32_t g = v.gval[e];
    if (!c.img_ok[v.feat_img[g]]) continue;
    if (v.f2p[g] >= 0) cand = false;
    ++n;
  }
  c.n_list[q] = cand && n ? n + 1 : 0;
}

// EstimateTriangulation of item q into the given list storage (n entries): success, X, the inlier mask; trials and margins
// added to the caller's
__device__ __noinline__ bool ci_estimate_item(const TuView& v, const CiDev& c, uint32_t q, uint32_t n, int32_t* clist, int32_t* lvl,
                                              uint8_t* mask, uint64_t carried_min_trials, double* X, uint32_t* trials, double* mg) {
  const uint32_t f = c.item_feat[q];
  uint32_t m = 0;
  for (uint32_t e = v.goff[f]; e < v.goff[f + 1] && m + 1 < n; ++e) {
    const uint32_t g = v.gval[e];
    if (c.img_ok[v.feat_img[g]]) clist[m++] = (int32_t)g;
  }
  clist[m++] = (int32_t)f;
  for (uint32_t i = 0; i < m; ++i) lvl[i] = (int32_t)i;
  RtLaneT<RtReproj> L;
  L.feat_img = v.feat_img, L.img_P = c.img_P, L.img_C = c.img_C, L.uv = c.uv, L.clist = clist, L.idx = lvl, L.n = (int)m, L.prm = c.prm;
  L.res.cams = v.cams, L.res.img_cam = v.img_cam, L.res.feat_img = v.feat_img, L.res.xy = v.xy;
  for (int k = 0; k < kRtMargins; ++k) L.mg[k] = mg[k];
  const bool ok = m >= 2 && rt_loransac(L, c.tab, c.tab_off, X, trials, carried_min_trials);
  if (ok)
    for (uint32_t i = 0; i < m; ++i) {
      RtView w;
      rt_view(L, (int)i, &w);
      mask[i] = L.res(w, rt_feature(L, (int)i), X, c.prm.max_residual, nullptr) <= c.prm.max_residual;
    }
  for (int k = 0; k < kRtMargins; ++k) mg[k] = L.mg[k];
  return ok;
}

__device__ inline void ci_fold_margins(unsigned long long* acc, const double* mg) {
  for (int k = 0; k < 4; ++k) atomicMin(&acc[CI_A_MG + k], (unsigned long long)__double_as_longlong(mg[k]));  // non-negative doubles
}

// The estimates that run ahead: a lane per candidate whose list has room in the pool.  A list above 15 entries runs with the
// min_num_trials the nearest candidate before it in its image would leave (the commit checks it against the carried one).
__global__ void __launch_bounds__(TU_BLOCK) k_ci_estimate(TuDev d, CiDev c) {
  const uint32_t q = blockIdx.x * TU_BLOCK + threadIdx.x;
  if (q >= c.Q) return;
  const uint32_t n = c.n_list[q];
  if (n == 0 || c.loff[q + 1] > c.pool_cap) return;
  unsigned long long carried = 0;
  if (n > 15)
    for (uint32_t p = q; p-- > c.item_first[q];) {
      const uint32_t np = c.n_list[p];
      if (np >= 2 && np <= 15) {
        carried = (unsigned long long)np * (np - 1) / 2;
        break;
      }
    }
  const uint32_t at = c.loff[q];
  double X[3] = {0.0, 0.0, 0.0}, mg[kRtMargins];
  for (int k = 0; k < kRtMargins; ++k) mg[k] = INFINITY;
  uint32_t trials = 0;
  const bool ok = ci_estimate_item(d.v, c, q, n, c.clist + at, c.lvl + at, c.mask + at, carried, X, &trials, mg);
  for (int k = 0; k < 3; ++k) c.est_xyz[3 * (size_t)q + k] = X[k];
  c.est_trials[q] = trials;
  c.est_min[q] = carried;
  c.est_state[q] = ok ? CI_OK : CI_FAILED;
  ci_fold_margins(c.acc, mg);
  atomicAdd(&c.acc[CI_A_AHEAD], 1ull);
}

// The ordered pass, on one lane: the reference's loop over the listed images and their point2Ds.
__global__ void k_ci_commit(TuDev d, CiDev c, uint32_t num_listed, const uint32_t* __restrict__ item_off) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const TuView& v = d.v;
  TuMargins mg{INFINITY, INFINITY, INFINITY};
  double emg[kRtMargins];
  for (int k = 0; k < kRtMargins; ++k) emg[k] = INFINITY;
  uint64_t ctrials = 0, rtrials = 0, npoints = 0, nobs = 0, nserial = 0, ncompleted = 0;
  for (uint32_t a = 0; a < num_listed; ++a) {
    uint64_t tris = 0, carried = 0;  // tri_options is set up per image: min_num_trials starts at 0
    for (uint32_t q = item_off[a]; q < item_off[a + 1]; ++q) {
      const uint32_t f = c.item_feat[q];
      if (v.f2p[f] >= 0) {  // Complete existing track
        const uint32_t k = tu_complete(v, (uint32_t)v.f2p[f], &mg, &ctrials);
        tris += k;
        ncompleted += k;
        continue;
      }
      const uint32_t n = c.n_list[q];
      if (n == 0) continue;
      bool taken = false;  // Find's num_triangulated, against the state as it is now
      for (uint32_t e = v.goff[f]; e < v.goff[f + 1] && !taken; ++e) {
        const uint32_t g = v.gval[e];
        taken = c.img_ok[v.feat_img[g]] && v.f2p[g] >= 0;
      }
      if (taken) continue;
      if (n <= 15) carried = (uint64_t)n * (n - 1) / 2;
      const int32_t* cl = c.clist + c.loff[q];
      const uint8_t* mk = c.mask + c.loff[q];
      double X[3];
      uint32_t trials = 0;
      bool ok;
      if (c.est_state[q] != CI_NOT_RUN && (n <= 15 || c.est_min[q] == carried)) {
        ok = c.est_state[q] == CI_OK;
        trials = c.est_trials[q];
        for (int k = 0; k < 3; ++k) X[k] = c.est_xyz[3 * (size_t)q + k];
      } else {
        ok = ci_estimate_item(v, c, q, n, c.ser_clist, c.ser_lvl, c.ser_mask, carried, X, &trials, emg);
        cl = c.ser_clist, mk = c.ser_mask;
        ++nserial;
      }
      rtrials += trials;
      if (!ok) continue;
      const uint32_t m = TU_FETCH_INC(v.num_slots);  // AddPoint3D
      if (m >= v.S) {
        atomicExch(&c.acc[CI_A_ERROR], 1ull);
        return;
      }
      for (int k = 0; k < 3; ++k) v.xyz[3 * (size_t)m + k] = X[k];
      v.head[m] = v.tail[m] = TU_NIL;
      v.len[m] = 0;
      for (uint32_t i = 0; i < n; ++i)
        if (mk[i]) tu_append(v, m, (uint32_t)cl[i]);
      v.alive[m] = 1;
      v.modified[m] = 1;
      v.ev_pos[m] = q;
      v.ev_depth[m] = 0;
      tris += v.len[m];
      nobs += v.len[m];
      ++npoints;
    }
    c.tris[a] = tris;
  }
  atomicAdd(&c.acc[CI_A_RTRIALS], (unsigned long long)rtrials);
  atomicAdd(&c.acc[CI_A_POINTS], (unsigned long long)npoints);
  atomicAdd(&c.acc[CI_A_OBS], (unsigned long long)nobs);
  atomicAdd(&c.acc[CI_A_SERIAL], (unsigned long long)nserial);
  atomicAdd(&c.acc[CI_A_COMPLETED], (unsigned long long)ncompleted);
  atomicAdd(&c.acc[CI_A_CTRIALS], (unsigned long long)ctrials);
  ci_fold_margins(c.acc, emg);
  tu_fold_margins(d.acc, mg);
}

struct TuBufs {
  DevBuf img_ok, img_P, img_C, uv, tab, tab_off, item_feat, item_first, item_off, n_list, loff, clist, lvl, mask, est_state, est_xyz, est_trials,
      est_min, ser_clist, ser_lvl, ser_mask, ci_acc, tris;
  DevBuf pair_img, moff, matches, nfeat, foff, acc_m, cnt, goff, scan_s[4], scan_x[4], epair, gval;
  DevBuf cams, img_cam, img_reg, img_bogus, pose, feat_img, xy, img_ids;
  DevBuf f2p, fnext, xyz, head, tail, len, alive, modified, stamp, born, done, num_slots, ev_pos, ev_depth;
  DevBuf wlist, wcount, claim, tested, pool_feat, pool_next, spec_head, spec_count, spec_trials, pending, ctr, acc, parent, label, list, comp_off, comp_pos;
  DevBuf out_slot, out_off, out_obs;
};

// d.goff[0 .. n) = exclusive scan of d.cnt[0 .. n) in fixed blocks (the pattern of retriangulation.hip's rt_scan)
hipError_t tu_scan(TuBufs& d, uint32_t n, hipStream_t st) {
  const uint32_t B = RT_GRAPH_BLOCK * 4;
  hipError_t e = d.goff.reserve((size_t)n * 4 + 16);
  std::vector<uint32_t> lens{n};
  while (lens.back() > B) lens.push_back((lens.back() + B - 1) / B);
  if (lens.size() > 4) return hipErrorInvalidValue;
  for (size_t l = 0; l < lens.size() && e == hipSuccess; ++l) {
    e = d.scan_s[l].reserve(((size_t)(lens[l] + B - 1) / B) * 4 + 16);
    if (e == hipSuccess) e = d.scan_x[l].reserve((size_t)lens[l] * 4 + 16);
  }
  if (e != hipSuccess) return e;
  std::vector<uint32_t*> outs;
  const uint32_t* in = d.cnt.as<uint32_t>();
  for (size_t l = 0; l < lens.size(); ++l) {
    uint32_t* out = l == 0 ? d.goff.as<uint32_t>() : d.scan_x[l].as<uint32_t>();
    hipLaunchKernelGGL(k_rt_scan_block, dim3((lens[l] + B - 1) / B), dim3(RT_GRAPH_BLOCK), 0, st, lens[l], in, out, d.scan_s[l].as<uint32_t>());
    outs.push_back(out);
    in = d.scan_s[l].as<uint32_t>();
  }
  for (size_t l = outs.size(); l-- > 1;)
    hipLaunchKernelGGL(k_rt_scan_add, dim3((lens[l - 1] + RT_GRAPH_BLOCK - 1) / RT_GRAPH_BLOCK), dim3(RT_GRAPH_BLOCK), 0, st, lens[l - 1], outs[l - 1], outs[l]);
  return hipGetLastError();
}

inline double tu_ms(std::chrono::steady_clock::time_point a) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
}

// the listed images of dsm_complete_images, validated: their indices in list order
struct CiCall {
  bool on = false;  // dsm_complete_images (dsm_update_tracks otherwise)
  std::vector<uint32_t> img;
  uint64_t* image_num_tris = nullptr;
  dsm_complete_images_report* report = nullptr;
};

// CompleteImage of the listed images over the device-resident state of the driver (after its steps).  *first_slot .. the
// counter's new value are the points it adds, in the order of the sequential run.
int tu_complete_images(dsm_ctx* ctx, TuHost& H, TuBufs& b, TuDev& d, const CiCall& ci, dsm_complete_images_report& rep) {
  hipStream_t st = ctx->stream;
  const uint32_t N = H.N, A = (uint32_t)ci.img.size();
  const uint64_t F = H.F;
  bool serial = false;
  uint64_t pool_limit = 0;
#ifdef DSM_CHECK_BUILD
  if (const char* s = ctx->dbg("DSM_COMPLETE_IMAGE_SERIAL")) {
    if (strncmp(s, "pool:", 5) == 0)
      pool_limit = strtoull(s + 5, nullptr, 10) + 1;  // + 1: 0 means no limit
    else
      serial = atoi(s) != 0;
  }
#endif
  auto t0 = std::chrono::steady_clock::now();
  std::vector<uint32_t> item_off(A + 1, 0), item_feat, item_first;
  for (uint32_t a = 0; a < A; ++a) {
    const uint32_t i = ci.img[a];
    if (H.img_reg[i] && !H.img_bogus[i])  // the reference returns 0 for the others
      for (uint32_t k = H.foff[i]; k < H.foff[i + 1]; ++k) {
        item_feat.push_back(k);
        item_first.push_back(item_off[a]);
      }
    item_off[a + 1] = (uint32_t)item_feat.size();
  }
  const uint32_t Q = (uint32_t)item_feat.size();
  rep.num_items = Q;
  HIPCHK(ctx, dev_fill(b.tris, 0, (size_t)std::max(A, 1u) * 8, st));
  std::vector<unsigned long long> acc0(CI_A_WORDS, 0);
  {
    const double inf = INFINITY;
    for (int k = 0; k < 4; ++k) memcpy(&acc0[CI_A_MG + k], &inf, 8);
  }
  HIPCHK(ctx, dev_upload(b.ci_acc, acc0.data(), CI_A_WORDS * 8, st));
  std::vector<unsigned long long> acc1(acc0);
  if (Q) {
    // the views: [R | t], the centre -R^T t (retriangulation.hip's rt_load_scene), ImageToWorld of the usable images' features
    std::vector<uint8_t> img_ok(N);
    std::vector<double> img_P(12 * (size_t)N), img_C(3 * (size_t)N);
    for (uint32_t i = 0; i < N; ++i) {
      img_ok[i] = H.img_reg[i] && !H.img_bogus[i];
      const double* T = &H.pose[(size_t)TU_POSE * i];
      for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) img_P[12 * (size_t)i + 4 * r + k] = T[3 * r + k];
        img_P[12 * (size_t)i + 4 * r + 3] = T[9 + r];
      }
      for (int k = 0; k < 3; ++k) img_C[3 * (size_t)i + k] = -((T[k] * T[9] + T[3 + k] * T[10]) + T[6 + k] * T[11]);
    }
    HIPCHK(ctx, dev_upload(b.img_ok, img_ok.data(), N, st));
    HIPCHK(ctx, dev_upload(b.img_P, img_P.data(), img_P.size() * 8, st));
    HIPCHK(ctx, dev_upload(b.img_C, img_C.data(), img_C.size() * 8, st));
    HIPCHK(ctx, b.uv.reserve(std::max<size_t>((size_t)F * 16, 16)));
    hipLaunchKernelGGL(k_rt_normalize, dim3(dsm_grid(F, TU_BLOCK)), dim3(TU_BLOCK), 0, st, (uint32_t)F, d.v.feat_img, b.img_ok.as<uint8_t>(), d.v.img_cam,
                       d.v.cams, d.v.xy, b.uv.as<double>());
    HIPCHK(ctx, dev_upload(b.item_feat, item_feat.data(), (size_t)Q * 4, st));
    HIPCHK(ctx, dev_upload(b.item_first, item_first.data(), (size_t)Q * 4, st));
    HIPCHK(ctx, dev_upload(b.item_off, item_off.data(), item_off.size() * 4, st));
    HIPCHK(ctx, b.n_list.reserve((size_t)Q * 4));
    CiDev c{};
    c.Q = Q;
    c.item_feat = b.item_feat.as<uint32_t>(), c.item_first = b.item_first.as<uint32_t>(), c.n_list = b.n_list.as<uint32_t>();
    c.img_ok = b.img_ok.as<uint8_t>(), c.img_P = b.img_P.as<double>(), c.img_C = b.img_C.as<double>(), c.uv = b.uv.as<double>();
    c.prm.max_residual = H.o.complete_max_reproj_error * H.o.complete_max_reproj_error;
    c.prm.min_tri_angle = H.o.tri.min_angle * kRtDegToRad;
    c.prm.ignore_two_view = H.o.tri.ignore_two_view_tracks;
    c.prm.max_trials = H.o.tri.ransac_max_num_trials;
    c.acc = b.ci_acc.as<unsigned long long>(), c.tris = b.tris.as<unsigned long long>();
    hipLaunchKernelGGL(k_ci_find, dim3(dsm_grid(Q, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, c);
    HIPCHK(ctx, hipGetLastError());
    std::vector<uint32_t> n_list(Q), loff(Q + 1, 0);
    HIPCHK(ctx, hipMemcpyAsync(n_list.data(), b.n_list.p, (size_t)Q * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    uint32_t maxn = 2;
    uint64_t M = 0;
    for (uint32_t q = 0; q < Q; ++q) {
      loff[q] = (uint32_t)std::min<uint64_t>(M, 0xffffffffu);
      M += n_list[q];
      maxn = std::max(maxn, n_list[q]);
    }
    loff[Q] = (uint32_t)std::min<uint64_t>(M, 0xffffffffu);
    if (maxn > CI_MAX_LIST) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_complete_images: a correspondence list of more than 8192 entries");
    // the estimate pool: the lists of all candidates; a limit (the check build's pool:<n>, or 2^32 entries) leaves the lists
    // behind it to the commit lane
    const uint64_t pool_cap = serial ? 0 : std::min<uint64_t>(pool_limit ? pool_limit - 1 : M, 0xfffffff0u);
    const uint64_t pool_alloc = std::min<uint64_t>(pool_cap, M);
    c.pool_cap = (uint32_t)pool_cap;
    HIPCHK(ctx, dev_upload(b.loff, loff.data(), loff.size() * 4, st));
    // ComputeNumTrials for n <= maxn (the host's libm), as dsm_retriangulate
    std::vector<uint32_t> tab_off(maxn + 1, 0), tab;
    for (uint32_t n = 2; n <= maxn; ++n) {
      tab_off[n] = (uint32_t)tab.size();
      for (uint32_t k = 0; k <= n; ++k) tab.push_back(rt_num_trials(k, n, H.o.tri.ransac_confidence));
    }
    HIPCHK(ctx, dev_upload(b.tab, tab.data(), tab.size() * 4, st));
    HIPCHK(ctx, dev_upload(b.tab_off, tab_off.data(), tab_off.size() * 4, st));
    c.prm.tab_n = maxn;
    for (DevBuf* x : {&b.clist, &b.lvl}) HIPCHK(ctx, x->reserve(std::max<size_t>((size_t)pool_alloc * 4, 16)));
    HIPCHK(ctx, b.mask.reserve(std::max<size_t>((size_t)pool_alloc, 16)));
    for (DevBuf* x : {&b.ser_clist, &b.ser_lvl}) HIPCHK(ctx, x->reserve((size_t)maxn * 4));
    HIPCHK(ctx, b.ser_mask.reserve(maxn));
    HIPCHK(ctx, dev_fill(b.est_state, CI_NOT_RUN, Q, st));
    HIPCHK(ctx, b.est_xyz.reserve((size_t)Q * 24));
    HIPCHK(ctx, b.est_trials.reserve((size_t)Q * 4));
    HIPCHK(ctx, b.est_min.reserve((size_t)Q * 8));
    c.loff = b.loff.as<uint32_t>(), c.tab = b.tab.as<uint32_t>(), c.tab_off = b.tab_off.as<uint32_t>();
    c.clist = b.clist.as<int32_t>(), c.lvl = b.lvl.as<int32_t>(), c.mask = b.mask.as<uint8_t>(), c.est_state = b.est_state.as<uint8_t>();
    c.est_xyz = b.est_xyz.as<double>(), c.est_trials = b.est_trials.as<uint32_t>(), c.est_min = b.est_min.as<unsigned long long>();
    c.ser_clist = b.ser_clist.as<int32_t>(), c.ser_lvl = b.ser_lvl.as<int32_t>(), c.ser_mask = b.ser_mask.as<uint8_t>();
    if (pool_cap) {
      hipLaunchKernelGGL(k_ci_estimate, dim3(dsm_grid(Q, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, c);
      HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    rep.estimate_ms = tu_ms(t0);
    t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(k_ci_commit, dim3(1), dim3(64), 0, st, d, c, A, b.item_off.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(acc1.data(), b.ci_acc.p, CI_A_WORDS * 8, hipMemcpyDeviceToHost, st));
    if (ci.image_num_tris) HIPCHK(ctx, hipMemcpyAsync(ci.image_num_tris, b.tris.p, (size_t)A * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    rep.commit_ms = tu_ms(t0);
    rep.num_rounds = 1;
    if (acc1[CI_A_ERROR]) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_complete_images: more new points than slots");
  } else if (ci.image_num_tris) {
    for (uint32_t a = 0; a < A; ++a) ci.image_num_tris[a] = 0;
  }
  rep.ransac_trials = acc1[CI_A_RTRIALS], rep.num_new_points = acc1[CI_A_POINTS], rep.num_new_observations = acc1[CI_A_OBS];
  rep.num_serial_items = acc1[CI_A_SERIAL], rep.num_completed_observations = acc1[CI_A_COMPLETED], rep.complete_trials = acc1[CI_A_CTRIALS];
  rep.num_estimated_ahead = acc1[CI_A_AHEAD];
  double mg[4];
  memcpy(mg, &acc1[CI_A_MG], 32);
  rep.min_residual_margin = mg[0], rep.min_support_margin = mg[1], rep.min_angle_margin = mg[2], rep.min_depth_margin = mg[3];
  return DSM_OK;
}

// dsm_update_tracks, and dsm_complete_images with its listed images behind the steps
int tu_run(dsm_ctx* ctx, const char* entry, CiCall& ci, const uint32_t* complete_image_ids, uint32_t num_complete_images, uint32_t num_cameras,
           const uint32_t* camera_ids, const dsm_camera* cameras, uint32_t num_images, const uint32_t* image_ids,
           const uint32_t* image_camera_ids, const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
           const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs, const uint32_t* pair_image_ids,
           const uint64_t* match_offsets, const uint32_t* matches, uint32_t num_points3D, const uint64_t* point3D_ids,
           const double* point3D_xyz, const uint64_t* track_offsets, const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps,
           uint64_t num_selected, const uint64_t* selected_ids, uint64_t next_point3D_id, const dsm_track_update_options* options,
           uint64_t* out_num_points, uint64_t* out_point_ids, double* out_xyz, uint64_t* out_track_offsets, uint32_t* out_track_obs,
           uint64_t* out_num_modified, uint64_t* out_modified, uint64_t* step_counts, dsm_track_update_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx, entry](const char* msg) { return dsm_invalid(ctx, entry, msg); };
  const auto t_host0 = std::chrono::steady_clock::now();
  if (!out_num_points || !out_num_modified || (num_steps && !step_counts)) return fail("NULL argument");
  TuHost H;
  {
    const std::string msg = tu_load(H, num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids, image_registered,
                                    image_qvec, image_tvec, points2D_offsets, points2D_xy, num_pairs, pair_image_ids, match_offsets,
                                    matches, num_points3D, point3D_ids, point3D_xyz, track_offsets, track_obs, num_steps, steps,
                                    num_selected, selected_ids, next_point3D_id, options);
    if (!msg.empty()) return fail(msg.c_str());
  }
  if (ci.on) {
    const dsm_triangulation_options& t = H.o.tri;
    if (t.max_transitivity != 1) return fail("max_transitivity other than 1 is not supported");
    if (t.ransac_max_num_trials < 1 || !(t.ransac_confidence > 0 && t.ransac_confidence < 1) || !(t.min_angle >= 0) || !std::isfinite(t.min_angle))
      return fail("option out of range");
    if (num_complete_images && !complete_image_ids) return fail("NULL argument");
    std::vector<std::pair<uint32_t, uint32_t>> by_id(num_images);
    for (uint32_t i = 0; i < num_images; ++i) by_id[i] = {image_ids[i], i};
    std::sort(by_id.begin(), by_id.end());
    std::vector<uint8_t> listed(num_images, 0);
    uint64_t extra = 0;
    for (uint32_t a = 0; a < num_complete_images; ++a) {
      auto it = std::lower_bound(by_id.begin(), by_id.end(), std::make_pair(complete_image_ids[a], 0u));
      if (it == by_id.end() || it->first != complete_image_ids[a]) return fail("an unknown image id in complete_image_ids");
      if (listed[it->second]) return fail("a repeated image id in complete_image_ids");
      listed[it->second] = 1;
      ci.img.push_back(it->second);
      extra += H.nfeat[it->second];
    }
    // every item can add one point: that many slots behind the merge events'
    extra = std::min<uint64_t>(extra, H.F);
    if ((uint64_t)H.S + extra >= 0x80000000ull) return fail("too many points3D");
    H.S += (uint32_t)extra;
    H.xyz.resize(3 * (size_t)H.S, 0.0), H.head.resize(H.S, TU_NIL), H.tail.resize(H.S, TU_NIL), H.len.resize(H.S, 0), H.alive.resize(H.S, 0);
    H.slot_id.resize(H.S, 0);
  }
  bool serial = false;
  uint64_t pool_limit = 0;
#ifdef DSM_CHECK_BUILD
  if (const char* s = ctx->dbg("DSM_TRACK_UPDATE_SERIAL")) {
    if (strncmp(s, "pool:", 5) == 0)
      pool_limit = strtoull(s + 5, nullptr, 10) + 1;  // + 1: 0 means no limit
    else
      serial = atoi(s) != 0;
  }
#endif
  dsm_track_update_report rep{};
  rep.num_points = H.P, rep.num_steps = num_steps;
  rep.min_bogus_margin = H.bogus_margin;
  rep.setup_ms = tu_ms(t_host0);

  hipError_t he = hipSetDevice(ctx->device);
  if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
  hipStream_t st = ctx->stream;
  TuBufs b;
  const auto t_dev0 = std::chrono::steady_clock::now();
  const uint64_t F = H.F, NM = H.NM;
  const uint32_t P = H.P, S = H.S, N = H.N;
  const size_t F1 = std::max<uint64_t>(F, 1);

  // ------------------------------------------------------------ the correspondence graph (rt_graph.h, as dsm_retriangulate)
  HIPCHK(ctx, dev_upload(b.nfeat, H.nfeat.data(), H.nfeat.size() * 4, st));
  HIPCHK(ctx, dev_upload(b.foff, H.foff.data(), H.foff.size() * 4, st));
  HIPCHK(ctx, dev_fill(b.cnt, 0, (F1 + 1) * 4, st));
  uint32_t E = 0;
  if (NM) {
    HIPCHK(ctx, dev_upload(b.pair_img, H.pair_img.data(), H.pair_img.size() * 4, st));
    HIPCHK(ctx, dev_upload(b.moff, match_offsets, ((size_t)num_pairs + 1) * 8, st));
    HIPCHK(ctx, dev_upload(b.matches, matches, NM * 8, st));
    HIPCHK(ctx, b.acc_m.reserve(NM));
    hipLaunchKernelGGL(k_rt_dedup, dim3(num_pairs), dim3(RT_GRAPH_BLOCK), 0, st, num_pairs, b.pair_img.as<uint32_t>(), b.moff.as<uint64_t>(),
                       b.matches.as<uint32_t>(), b.nfeat.as<uint32_t>(), b.acc_m.as<uint8_t>());
    hipLaunchKernelGGL(k_rt_count, dim3(num_pairs), dim3(RT_GRAPH_BLOCK), 0, st, num_pairs, b.pair_img.as<uint32_t>(), b.moff.as<uint64_t>(),
                       b.matches.as<uint32_t>(), b.acc_m.as<uint8_t>(), b.foff.as<uint32_t>(), b.cnt.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  HIPCHK(ctx, tu_scan(b, (uint32_t)F + 1, st));
  HIPCHK(ctx, hipMemcpyAsync(&E, b.goff.as<uint32_t>() + F, 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  for (DevBuf* x : {&b.epair, &b.gval}) HIPCHK(ctx, x->reserve(std::max<size_t>((size_t)E * 4, 16)));
  if (E) {
    HIPCHK(ctx, hipMemsetAsync(b.cnt.p, 0, F1 * 4, st));  // reused as the fill counters
    hipLaunchKernelGGL(k_rt_emit, dim3(num_pairs), dim3(RT_GRAPH_BLOCK), 0, st, num_pairs, b.pair_img.as<uint32_t>(), b.moff.as<uint64_t>(),
                       b.matches.as<uint32_t>(), b.acc_m.as<uint8_t>(), b.foff.as<uint32_t>(), b.goff.as<uint32_t>(), b.cnt.as<uint32_t>(),
                       b.epair.as<uint32_t>(), b.gval.as<uint32_t>());
    hipLaunchKernelGGL(k_rt_segsort, dim3(dsm_grid(F, TU_BLOCK)), dim3(RT_GRAPH_BLOCK), 0, st, (uint32_t)F, b.goff.as<uint32_t>(), b.epair.as<uint32_t>(),
                       b.gval.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
  }
  rep.num_correspondences = E;

  // ------------------------------------------------------------ the scene and the state
  HIPCHK(ctx, dev_upload(b.cams, cameras, (size_t)num_cameras * sizeof(dsm_camera), st));
  HIPCHK(ctx, dev_upload(b.img_cam, H.img_cam.data(), (size_t)N * 4, st));
  HIPCHK(ctx, dev_upload(b.img_reg, H.img_reg.data(), N, st));
  HIPCHK(ctx, dev_upload(b.img_bogus, H.img_bogus.data(), N, st));
  HIPCHK(ctx, dev_upload(b.pose, H.pose.data(), H.pose.size() * 8, st));
  HIPCHK(ctx, dev_upload(b.feat_img, H.feat_img.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(b.xy, points2D_xy, F * 16, st));
  HIPCHK(ctx, dev_upload(b.img_ids, image_ids, (size_t)N * 4, st));
  HIPCHK(ctx, dev_upload(b.f2p, H.f2p.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(b.fnext, H.fnext.data(), F * 4, st));
  HIPCHK(ctx, dev_upload(b.xyz, H.xyz.data(), (size_t)S * 24, st));
  HIPCHK(ctx, dev_upload(b.head, H.head.data(), (size_t)S * 4, st));
  HIPCHK(ctx, dev_upload(b.tail, H.tail.data(), (size_t)S * 4, st));
  HIPCHK(ctx, dev_upload(b.len, H.len.data(), (size_t)S * 4, st));
  HIPCHK(ctx, dev_upload(b.alive, H.alive.data(), S, st));
  HIPCHK(ctx, dev_fill(b.modified, 0, S, st));
  for (DevBuf* x : {&b.stamp, &b.born, &b.done, &b.ev_pos, &b.ev_depth, &b.parent, &b.label}) HIPCHK(ctx, dev_fill(*x, 0, (size_t)S * 4, st));
  HIPCHK(ctx, dev_upload(b.num_slots, &P, 4, st));
  HIPCHK(ctx, dev_fill(b.claim, 0xff, F1 * 8, st));
  HIPCHK(ctx, dev_fill(b.tested, 0xff, F1 * 8, st));
  HIPCHK(ctx, dev_fill(b.ctr, 0, TU_C_WORDS * 4, st));
  const size_t n_acc = TU_A_STEPS + (size_t)num_steps;
  std::vector<unsigned long long> acc0(n_acc, 0);
  {
    const double inf = INFINITY;
    for (int k = 0; k < 3; ++k) memcpy(&acc0[TU_A_MG + k], &inf, 8);
  }
  HIPCHK(ctx, dev_upload(b.acc, acc0.data(), n_acc * 8, st));
  // the claim pool: every feature can be accepted by several pending walks of a round; four entries per feature cover what a
  // round of a real scene speculates, and a round that needs more ends in the serial form
  const uint64_t pool_cap64 = pool_limit ? pool_limit - 1 : std::min<uint64_t>(4 * F + 1024, 0x7fffffffu);
  const uint32_t pool_cap = (uint32_t)pool_cap64;
  HIPCHK(ctx, b.pool_feat.reserve(std::max<size_t>((size_t)pool_cap * 4, 16)));
  HIPCHK(ctx, b.pool_next.reserve(std::max<size_t>((size_t)pool_cap * 4, 16)));
  const size_t L1 = std::max<size_t>((size_t)S, 1);  // a step's list never holds more than the slots
  for (DevBuf* x : {&b.spec_head, &b.spec_count, &b.spec_trials, &b.list, &b.comp_off, &b.comp_pos, &b.wlist}) HIPCHK(ctx, x->reserve((L1 + 1) * 4));
  HIPCHK(ctx, b.pending.reserve(L1));

  TuDev d{};
  d.v.N = N, d.v.P = P, d.v.S = S, d.v.F = F;
  d.v.cams = b.cams.as<dsm_camera>(), d.v.img_cam = b.img_cam.as<uint32_t>(), d.v.img_reg = b.img_reg.as<uint8_t>();
  d.v.img_bogus = b.img_bogus.as<uint8_t>(), d.v.pose = b.pose.as<double>(), d.v.feat_img = b.feat_img.as<uint32_t>();
  d.v.xy = b.xy.as<double>(), d.v.goff = b.goff.as<uint32_t>(), d.v.gval = b.gval.as<uint32_t>();
  d.v.thr2_complete = H.o.complete_max_reproj_error * H.o.complete_max_reproj_error;
  d.v.thr2_merge = H.o.merge_max_reproj_error * H.o.merge_max_reproj_error;
  d.v.max_transitivity = H.o.complete_max_transitivity;
  d.v.f2p = b.f2p.as<int32_t>(), d.v.fnext = b.fnext.as<uint32_t>(), d.v.xyz = b.xyz.as<double>(), d.v.head = b.head.as<uint32_t>();
  d.v.tail = b.tail.as<uint32_t>(), d.v.len = b.len.as<uint32_t>(), d.v.alive = b.alive.as<uint8_t>(), d.v.modified = b.modified.as<uint8_t>();
  d.v.stamp = b.stamp.as<uint32_t>(), d.v.born = b.born.as<uint32_t>(), d.v.done = b.done.as<uint32_t>();
  d.v.num_slots = b.num_slots.as<uint32_t>(), d.v.ev_pos = b.ev_pos.as<uint32_t>(), d.v.ev_depth = b.ev_depth.as<uint32_t>();
  d.claim = b.claim.as<unsigned long long>(), d.tested = b.tested.as<unsigned long long>(), d.pool_feat = b.pool_feat.as<uint32_t>(), d.pool_next = b.pool_next.as<uint32_t>();
  d.pool_cap = pool_cap, d.spec_head = b.spec_head.as<uint32_t>(), d.spec_count = b.spec_count.as<uint32_t>();
  d.spec_trials = b.spec_trials.as<uint32_t>(), d.pending = b.pending.as<uint8_t>(), d.ctr = b.ctr.as<uint32_t>();
  d.acc = b.acc.as<unsigned long long>(), d.parent = b.parent.as<uint32_t>();
  HIPCHK(ctx, hipStreamSynchronize(st));
  rep.graph_ms = tu_ms(t_dev0);

  // ------------------------------------------------------------ the steps
  uint32_t tag = 0xffffffffu;  // the round tag counts down: a later round's claim beats every stale one
  uint32_t slots_used = P;
  std::vector<uint32_t> label(S), cur_len(S), ev_pos(S, 0), ev_depth(S, 0);
  for (uint32_t s = 0; s < num_steps; ++s) {
    const std::vector<uint32_t> list = tu_step_list(H);
    const uint32_t n = (uint32_t)list.size();
    if (n == 0) continue;
    HIPCHK(ctx, dev_upload(b.list, list.data(), (size_t)n * 4, st));
    const uint32_t* dl = b.list.as<uint32_t>();
    if (steps[s] == DSM_TRACKS_COMPLETE) {
      const auto t0 = std::chrono::steady_clock::now();
      HIPCHK(ctx, hipMemsetAsync(b.pending.p, 1, n, st));
      bool to_serial = serial;
      uint32_t nw = 0;
      if (!serial) {
        HIPCHK(ctx, dev_fill(b.wcount, 0, 16, st));
        hipLaunchKernelGGL(k_tu_wave_list, dim3(dsm_grid(n, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, dl, n, b.wlist.as<uint32_t>(), b.wcount.as<uint32_t>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(&nw, b.wcount.p, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        nw = std::min(nw, n);
      }
      while (!to_serial) {
        if (tag == 0) return dsm_fail(ctx, DSM_ERR_OUT_OF_RANGE, "dsm_update_tracks: more than 2^32 claim rounds");
        HIPCHK(ctx, hipMemsetAsync(b.ctr.p, 0, TU_C_WORDS * 4, st));
        hipLaunchKernelGGL(k_tu_speculate, dim3(dsm_grid(n, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, dl, n, tag);
        if (nw) hipLaunchKernelGGL(k_tu_speculate_wave, dim3(nw), dim3(64), 0, st, d, dl, b.wlist.as<uint32_t>(), nw, tag);
        hipLaunchKernelGGL(k_tu_commit, dim3(dsm_grid(n, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, dl, n, tag, s);
        HIPCHK(ctx, hipGetLastError());
        uint32_t c[TU_C_WORDS];
        HIPCHK(ctx, hipMemcpyAsync(c, b.ctr.p, sizeof(c), hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));  // the one read of the round
        --tag;
        ++rep.complete_rounds;
        if (c[TU_C_OVERFLOW])
          to_serial = true;
        else if (c[TU_C_PENDING] == 0)
          break;
      }
      if (to_serial) {
        hipLaunchKernelGGL(k_tu_complete_serial, dim3(1), dim3(64), 0, st, d, dl, n, s);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(st));
        ++rep.complete_serial_steps;
      }
      rep.complete_ms += tu_ms(t0);
    } else {
      auto t0 = std::chrono::steady_clock::now();
      for (DevBuf* x : {&b.born, &b.done}) HIPCHK(ctx, hipMemsetAsync(x->p, 0, (size_t)S * 4, st));
      HIPCHK(ctx, hipMemsetAsync(b.stamp.p, 0xff, (size_t)S * 4, st));
      std::vector<uint32_t> comp_off, comp_pos(n);
      uint32_t n_lane = 0;  // the components that run on a lane each come first
      if (serial) {
        n_lane = 1;
        comp_off = {0, n};
        for (uint32_t i = 0; i < n; ++i) comp_pos[i] = i;
        rep.num_components = 1, rep.largest_component = n;
      } else {
        hipLaunchKernelGGL(k_tu_parent_init, dim3(dsm_grid(S, TU_BLOCK)), dim3(TU_BLOCK), 0, st, S, d.parent);
        if (F) hipLaunchKernelGGL(k_tu_hook, dim3(dsm_grid(F, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d);
        hipLaunchKernelGGL(k_tu_label, dim3(dsm_grid(S, TU_BLOCK)), dim3(TU_BLOCK), 0, st, S, d.parent, b.label.as<uint32_t>());
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(label.data(), b.label.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(cur_len.data(), b.len.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        rep.components_ms += tu_ms(t0);
        t0 = std::chrono::steady_clock::now();
        // the list bucketed by component, positions ascending inside a bucket (a stable counting pass over the labels)
        // A component whose selected points hold at most TU_WAVE_ELEMS track elements runs on a lane, the others on a wave
        // each: the lanes of a wave share out the all-inlier test and nothing else, which pays by the elements tested.
        std::vector<uint32_t> cnt(S + 1, 0), comp_of(S, TU_NIL);
        std::vector<uint64_t> elems(S, 0);
        for (uint32_t i = 0; i < n; ++i) {
          ++cnt[label[list[i]]];
          elems[label[list[i]]] += cur_len[list[i]];
        }
        uint32_t ncomp = 0, largest = 0;
        comp_off.push_back(0);
        for (int wave = 0; wave < 2; ++wave) {
          for (uint32_t r = 0; r < S; ++r)
            if (cnt[r] && (elems[r] > TU_WAVE_ELEMS) == (wave == 1)) {
              comp_of[r] = ncomp++;
              comp_off.push_back(comp_off.back() + cnt[r]);
              largest = std::max(largest, cnt[r]);
            }
          if (wave == 0) n_lane = ncomp;
        }
        std::vector<uint32_t> at(comp_off.begin(), comp_off.end() - 1);
        for (uint32_t i = 0; i < n; ++i) comp_pos[at[comp_of[label[list[i]]]]++] = i;
        rep.num_components = ncomp, rep.largest_component = largest;
        rep.schedule_ms += tu_ms(t0);
        t0 = std::chrono::steady_clock::now();
      }
      const uint32_t ncomp = (uint32_t)comp_off.size() - 1;
      HIPCHK(ctx, dev_upload(b.comp_off, comp_off.data(), comp_off.size() * 4, st));
      HIPCHK(ctx, dev_upload(b.comp_pos, comp_pos.data(), (size_t)n * 4, st));
      if (n_lane)
        hipLaunchKernelGGL(k_tu_merge_lane, dim3(dsm_grid(n_lane, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, dl, b.comp_off.as<uint32_t>(), b.comp_pos.as<uint32_t>(), n_lane, s);
      if (ncomp > n_lane)
        hipLaunchKernelGGL(k_tu_merge, dim3(ncomp - n_lane), dim3(64), 0, st, d, dl, b.comp_off.as<uint32_t>(), b.comp_pos.as<uint32_t>(), n_lane, ncomp, s);
      HIPCHK(ctx, hipGetLastError());
      uint32_t now_used = 0;
      HIPCHK(ctx, hipMemcpyAsync(&now_used, b.num_slots.p, 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      now_used = std::min(now_used, S);
      if (now_used > slots_used) {  // the events of this step, numbered in one ordered pass
        HIPCHK(ctx, hipMemcpyAsync(ev_pos.data() + slots_used, b.ev_pos.as<uint32_t>() + slots_used, (size_t)(now_used - slots_used) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(ev_depth.data() + slots_used, b.ev_depth.as<uint32_t>() + slots_used, (size_t)(now_used - slots_used) * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        tu_assign_ids(H, slots_used, now_used, ev_pos.data(), ev_depth.data());
        slots_used = now_used;
      }
      rep.merge_ms += tu_ms(t0);
    }
  }

  // ------------------------------------------------------------ CompleteImage of the listed images
  dsm_complete_images_report crep{};
  std::vector<unsigned long long> acc_steps(n_acc);
  if (ci.on) {
    HIPCHK(ctx, hipMemcpyAsync(acc_steps.data(), b.acc.p, n_acc * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    crep.num_images = (uint32_t)ci.img.size();
    const int rc = tu_complete_images(ctx, H, b, d, ci, crep);
    if (rc != DSM_OK) return rc;
    uint32_t now_used = 0;
    HIPCHK(ctx, hipMemcpyAsync(&now_used, b.num_slots.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    now_used = std::min(now_used, S);
    if (now_used > slots_used) {  // the new points, numbered in item order behind the merge events
      HIPCHK(ctx, hipMemcpyAsync(ev_pos.data() + slots_used, b.ev_pos.as<uint32_t>() + slots_used, (size_t)(now_used - slots_used) * 4, hipMemcpyDeviceToHost, st));
      HIPCHK(ctx, hipStreamSynchronize(st));
      std::fill(ev_depth.begin() + slots_used, ev_depth.begin() + now_used, 0u);
      tu_assign_ids(H, slots_used, now_used, ev_pos.data(), ev_depth.data());
      slots_used = now_used;
    }
  }

  // ------------------------------------------------------------ the results
  const auto t_out = std::chrono::steady_clock::now();
  std::vector<uint8_t> alive(S), modified(S);
  std::vector<uint32_t> len(S);
  std::vector<unsigned long long> acc1(n_acc);
  HIPCHK(ctx, hipMemcpyAsync(alive.data(), b.alive.p, S, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(modified.data(), b.modified.p, S, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(len.data(), b.len.p, (size_t)S * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(H.xyz.data(), b.xyz.p, (size_t)S * 24, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipMemcpyAsync(acc1.data(), b.acc.p, n_acc * 8, hipMemcpyDeviceToHost, st));
  HIPCHK(ctx, hipStreamSynchronize(st));
  const std::vector<uint32_t> out = tu_output_slots(H, alive.data());
  const uint32_t n_out = (uint32_t)out.size();
  std::vector<uint64_t> off(n_out + 1, 0);
  for (uint32_t i = 0; i < n_out; ++i) off[i + 1] = off[i] + len[out[i]];
  const uint64_t total = off[n_out];
  if (total > F) return dsm_fail(ctx, DSM_ERR_HIP, "dsm_update_tracks: the tracks hold more elements than there are points2D");
  std::vector<uint32_t> obs(2 * (size_t)total);
  if (n_out && total && out_track_obs) {
    HIPCHK(ctx, dev_upload(b.out_slot, out.data(), (size_t)n_out * 4, st));
    HIPCHK(ctx, dev_upload(b.out_off, off.data(), ((size_t)n_out + 1) * 8, st));
    HIPCHK(ctx, b.out_obs.reserve((size_t)total * 8));
    hipLaunchKernelGGL(k_tu_emit, dim3(dsm_grid(n_out, TU_BLOCK)), dim3(TU_BLOCK), 0, st, d, b.out_slot.as<uint32_t>(), b.out_off.as<uint64_t>(), n_out,
                       b.img_ids.as<uint32_t>(), b.foff.as<uint32_t>(), b.out_obs.as<uint32_t>());
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(out_track_obs, b.out_obs.p, (size_t)total * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
  }
  uint64_t nmod = 0;
  for (uint32_t i = 0; i < n_out; ++i) {
    const uint32_t sl = out[i];
    if (out_point_ids) out_point_ids[i] = H.slot_id[sl];
    if (out_xyz)
      for (int k = 0; k < 3; ++k) out_xyz[3 * (size_t)i + k] = H.xyz[3 * (size_t)sl + k];
    if (modified[sl]) {
      if (out_modified) out_modified[nmod] = H.slot_id[sl];
      ++nmod;
    }
  }
  if (out_track_offsets)
    for (uint32_t i = 0; i <= n_out; ++i) out_track_offsets[i] = off[i];
  *out_num_points = n_out;
  *out_num_modified = nmod;
  for (uint32_t s = 0; s < num_steps; ++s) {
    step_counts[s] = acc1[TU_A_STEPS + s];
    (steps[s] == DSM_TRACKS_COMPLETE ? rep.num_completed : rep.num_merged) += step_counts[s];
  }
  rep.complete_trials = acc1[TU_A_CTRIALS];
  rep.merge_trials = acc1[TU_A_MTRIALS];
  rep.num_merge_events = acc1[TU_A_EVENTS];
  double mg[3];
  memcpy(mg, &acc1[TU_A_MG], 24);
  rep.min_complete_error_margin = mg[0], rep.min_merge_error_margin = mg[1], rep.min_depth_margin = mg[2];
  rep.download_ms = tu_ms(t_out);
  rep.device_ms = tu_ms(t_dev0);
  if (report) *report = rep;
  if (ci.on && ci.report) {
    // the Complete walks of the images fold their margins and trials into the steps' accumulators: the steps' own share is
    // what they held before the images ran
    crep.complete_trials += acc_steps[TU_A_CTRIALS];
    crep.min_complete_error_margin = mg[0];
    crep.min_depth_margin = std::min(crep.min_depth_margin, mg[2]);
    crep.min_bogus_margin = H.bogus_margin;
    crep.device_ms = rep.device_ms;
    crep.steps = rep;
    crep.steps.complete_trials = acc_steps[TU_A_CTRIALS];
    *ci.report = crep;
  }
  return DSM_OK;
}

}  // namespace

extern "C" void dsm_default_track_update_options(dsm_track_update_options* o) { tu_default_options(o); }

extern "C" int dsm_update_tracks(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                 uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                 const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                                 const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                                 const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                 uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz,
                                 const uint64_t* track_offsets, const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps,
                                 uint64_t num_selected, const uint64_t* selected_ids, uint64_t next_point3D_id,
                                 const dsm_track_update_options* options, uint64_t* out_num_points, uint64_t* out_point_ids,
                                 double* out_xyz, uint64_t* out_track_offsets, uint32_t* out_track_obs, uint64_t* out_num_modified,
                                 uint64_t* out_modified, uint64_t* step_counts, dsm_track_update_report* report) {
  CiCall ci;
  return tu_run(ctx, "dsm_update_tracks", ci, nullptr, 0, num_cameras, camera_ids, cameras, num_images, image_ids, image_camera_ids,
                image_registered, image_qvec, image_tvec, points2D_offsets, points2D_xy, num_pairs, pair_image_ids, match_offsets, matches,
                num_points3D, point3D_ids, point3D_xyz, track_offsets, track_obs, num_steps, steps, num_selected, selected_ids,
                next_point3D_id, options, out_num_points, out_point_ids, out_xyz, out_track_offsets, out_track_obs, out_num_modified,
                out_modified, step_counts, report);
}

extern "C" int dsm_complete_images(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                                   uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                                   const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                                   const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                                   const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                                   uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz,
                                   const uint64_t* track_offsets, const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps,
                                   uint64_t num_selected, const uint64_t* selected_ids, uint64_t next_point3D_id,
                                   uint32_t num_complete_images, const uint32_t* complete_image_ids,
                                   const dsm_track_update_options* options, uint64_t* out_num_points, uint64_t* out_point_ids,
                                   double* out_xyz, uint64_t* out_track_offsets, uint32_t* out_track_obs, uint64_t* out_num_modified,
                                   uint64_t* out_modified, uint64_t* step_counts, uint64_t* image_num_tris,
                                   dsm_complete_images_report* report) {
  CiCall ci;
  ci.on = true;
  ci.image_num_tris = image_num_tris;
  ci.report = report;
  return tu_run(ctx, "dsm_complete_images", ci, complete_image_ids, num_complete_images, num_cameras, camera_ids, cameras, num_images, image_ids,
                image_camera_ids, image_registered, image_qvec, image_tvec, points2D_offsets, points2D_xy, num_pairs, pair_image_ids,
                match_offsets, matches, num_points3D, point3D_ids, point3D_xyz, track_offsets, track_obs, num_steps, steps, num_selected,
                selected_ids, next_point3D_id, options, out_num_points, out_point_ids, out_xyz, out_track_offsets, out_track_obs,
                out_num_modified, out_modified, step_counts, nullptr);
}
