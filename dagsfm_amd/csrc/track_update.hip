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

struct TuBufs {
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
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  auto fail = [ctx](const char* msg) { return dsm_invalid(ctx, "dsm_update_tracks", msg); };
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
  return DSM_OK;
}
