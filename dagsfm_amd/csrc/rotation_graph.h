// rotation_graph.h -- the steps of GlobalRotationAveraging() that do not depend on the estimator
// (src/controllers/distributed_mapper_controller.cpp:945-1008), shared by rotation_averaging.hip (ROBUST_L1L2) and
// nonlinear_rotation.hip (NONLINEAR):
//   1. the argument checks, the unique edges and the largest component (ImageGraph::ExtractLargestCC, src/graph/image_graph.cpp:8-50)
//   3. FilterViewPairsFromOrientation (src/sfm/filter_view_pairs_from_orientation.cpp:22-90), a kernel
//   4. the largest component of the surviving edges, and the outputs
#ifndef DAGSFM_AMD_CSRC_ROTATION_GRAPH_H_
#define DAGSFM_AMD_CSRC_ROTATION_GRAPH_H_

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "ctx.h"
#include "graph_edges.h"
#include "rotation_ceres.h"

namespace {

constexpr int RA_BLOCK = 256;
constexpr double kRaDegToRad = 0.017453292519943295;  // M_PI / 180 (util.h DegToRad)

// ---------------------------------------------------------------- rotations (ceres' conversions, rotation_ceres.h)
__device__ inline void aa_to_R(const double* aa, double* R) { ceres_angle_axis_to_rotation(aa, R); }
__device__ inline void R_to_aa(const double* R, double* aa) {  // RotationMatrixToAngleAxis
  double q[4];
  ceres_rotation_to_quaternion(R, q);
  ceres_quaternion_to_angle_axis(q, aa);
}
__device__ inline void matmul3(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) C[i * 3 + j] = A[i * 3 + 0] * B[0 * 3 + j] + A[i * 3 + 1] * B[1 * 3 + j] + A[i * 3 + 2] * B[2 * 3 + j];
}
// MultiplyRotations (src/math/rotation.cpp:157-167): AngleAxis(R(a) * R(b))
__device__ inline void mul_rot(const double* a, const double* b, double* out) {
  double Ra[9], Rb[9], C[9];
  aa_to_R(a, Ra);
  aa_to_R(b, Rb);
  matmul3(Ra, Rb, C);
  R_to_aa(C, out);
}

// FilterViewPairsFromOrientation (filter_view_pairs_from_orientation.cpp:22-35, 71-80): keep iff
// |MultiplyRotations(-R12, MultiplyRotations(R_j, -R_i))|^2 <= theta^2; a kept edge gets RelativeRotationFromTwoRotations
// (util.h:97-106) = AngleAxis(R(R_j) * R(R_i)^T)
__global__ void __launch_bounds__(RA_BLOCK) k_ra_filter(uint32_t M, const uint32_t* __restrict__ ei, const uint32_t* __restrict__ ej,
                                                        const double* __restrict__ r12, const double* __restrict__ R, double sq_thr,
                                                        uint8_t* __restrict__ state, double* __restrict__ rel) {
  const uint32_t e = blockIdx.x * RA_BLOCK + threadIdx.x;
  if (e >= M) return;
  const double* Ri = R + 3 * (size_t)ei[e];
  const double* Rj = R + 3 * (size_t)ej[e];
  const double* a = r12 + 3 * (size_t)e;
  double mRi[3] = {-Ri[0], -Ri[1], -Ri[2]}, ma[3] = {-a[0], -a[1], -a[2]}, comp[3], loop[3];
  mul_rot(Rj, mRi, comp);
  mul_rot(ma, comp, loop);
  const bool ok = loop[0] * loop[0] + loop[1] * loop[1] + loop[2] * loop[2] <= sq_thr;
  state[e] = ok ? 3 : 2;
  double out[3] = {0.0, 0.0, 0.0};
  if (ok) {
    double M1[9], M2[9], T[9];
    aa_to_R(Ri, M1);
    aa_to_R(Rj, M2);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) T[i * 3 + j] = M2[i * 3 + 0] * M1[j * 3 + 0] + M2[i * 3 + 1] * M1[j * 3 + 1] + M2[i * 3 + 2] * M1[j * 3 + 2];
    R_to_aa(T, out);
  }
  for (int c = 0; c < 3; ++c) rel[3 * (size_t)e + c] = out[c];
}

// ---------------------------------------------------------------- host side
struct Uf {
  std::vector<uint32_t> p;
  explicit Uf(size_t n) : p(n) { std::iota(p.begin(), p.end(), 0u); }
  uint32_t find(uint32_t x) {
    while (p[x] != x) x = p[x] = p[p[x]];
    return x;
  }
  void join(uint32_t a, uint32_t b) {
    a = find(a);
    b = find(b);
    if (a != b) p[std::max(a, b)] = std::min(a, b);  // the root is the smallest member
  }
};

// the largest component of (verts 0..V-1, edges); ties: the one holding the smallest vertex (vertices ascend with image id).
// Returns the flag per vertex and the number of components.
uint32_t largest_component(uint32_t V, const std::vector<std::pair<uint32_t, uint32_t>>& edges, std::vector<uint8_t>& in_cc) {
  Uf uf(V);
  for (const auto& e : edges) uf.join(e.first, e.second);
  std::vector<uint32_t> size(V, 0);
  uint32_t n_comp = 0;
  for (uint32_t v = 0; v < V; ++v) {
    if (uf.find(v) == v) ++n_comp;
    ++size[uf.find(v)];
  }
  uint32_t best = 0;
  for (uint32_t v = 0; v < V; ++v)  // ascending roots = ascending smallest members: the first maximum wins
    if (size[v] > size[best]) best = v;
  in_cc.assign(V, 0);
  for (uint32_t v = 0; v < V; ++v) in_cc[v] = V && uf.find(v) == best;
  return n_comp;
}

// the first component as the device sees it: N images in ascending id order (cimg), M edges in canonical (lo, hi) order
struct RaGraph {
  uint32_t N = 0, M = 0, num_components = 0;
  std::vector<uint32_t> cimg;       // image id of component vertex v; cimg[0] is the smallest id
  std::vector<GraphEdge> ce_edges;  // vertices in component numbering
  std::vector<uint32_t> ei, ej;     // the edge's image 1 and image 2
  std::vector<uint32_t> off, nb, cev;  // CSR over images, entries sorted by neighbour; cev: 2 k + (the entry's image is edge k's image 2)
  std::vector<double> r12;          // M x 3: QuaternionToAngleAxis(qvec)
};

// Step 1.  The pointer and range checks of the arguments every estimator shares, the checks on every used edge before
// anything is written, edge_state / relative_rotations_out cleared, then the graph.  `who` prefixes the messages.  Returns
// DSM_OK with g.M == 0 where there is no used edge.
inline int ra_build_graph(dsm_ctx* ctx, const char* who, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs, const uint8_t* use,
                          uint8_t* edge_state, double* relative_rotations_out, RaGraph& g) {
  const std::string name(who);
  for (uint32_t e = 0; e < n_pairs; ++e) {
    if (use && !use[e]) continue;
    if (pairs[2 * e] == pairs[2 * e + 1]) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, (name + ": image_id1 == image_id2").c_str());
    const double* q = qvecs + 4 * (size_t)e;
    bool finite = true, zero = true;
    for (int c = 0; c < 4; ++c) {
      finite &= std::isfinite(q[c]);
      zero &= q[c] == 0.0;
    }
    if (!finite || zero) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, (name + ": non-finite or zero qvec").c_str());
  }
  for (uint32_t e = 0; e < n_pairs; ++e) {
    edge_state[e] = 0;
    for (int c = 0; c < 3; ++c) relative_rotations_out[3 * (size_t)e + c] = 0.0;
  }
  // host: unique used edges (the first occurrence of an unordered pair wins, ViewGraph::AddTwoViewGeometry), images renumbered
  // by ascending id, the first component (ImageGraph::ExtractLargestCC)
  std::vector<uint32_t> ids;
  const std::vector<GraphEdge> uniq = graph_unique_edges(n_pairs, pairs, use, ids);
  if (uniq.empty()) return DSM_OK;
  const uint32_t V = (uint32_t)ids.size();
  std::vector<std::pair<uint32_t, uint32_t>> ue;
  for (const GraphEdge& x : uniq) ue.emplace_back(x.lo, x.hi);
  std::vector<uint8_t> in1;
  g.num_components = largest_component(V, ue, in1);
  std::vector<uint32_t> cid(V, UINT32_MAX);  // component renumbering: ascending id
  for (uint32_t v = 0; v < V; ++v)
    if (in1[v]) {
      cid[v] = (uint32_t)g.cimg.size();
      g.cimg.push_back(ids[v]);
    }
  g.N = (uint32_t)g.cimg.size();
  for (const GraphEdge& x : uniq) {
    if (!in1[x.lo]) {
      edge_state[x.orig] = 1;
      continue;
    }
    g.ce_edges.push_back(GraphEdge{cid[x.lo], cid[x.hi], cid[x.i], cid[x.j], x.orig});
  }
  const uint32_t M = g.M = (uint32_t)g.ce_edges.size();
  g.ei.resize(M);
  g.ej.resize(M);
  graph_neighbour_csr(g.N, g.ce_edges, g.off, g.nb, g.cev);
  for (uint32_t v = 0; v < g.N; ++v)
    for (uint32_t p = g.off[v]; p < g.off[v + 1]; ++p) {
      const uint32_t k = g.cev[p];
      g.cev[p] = 2 * k + (g.ce_edges[k].j == v ? 1u : 0u);
    }
  g.r12.resize(3 * (size_t)M);
  for (uint32_t k = 0; k < M; ++k) {
    const GraphEdge& x = g.ce_edges[k];
    g.ei[k] = x.i;
    g.ej[k] = x.j;
    // QuaternionToAngleAxis (ceres) on the host, the formula of rotation_ceres.h
    const double* q = qvecs + 4 * (size_t)x.orig;
    const double q1 = q[1], q2 = q[2], q3 = q[3];
    const double s2 = q1 * q1 + q2 * q2 + q3 * q3;
    double kk = 2.0;
    if (s2 > 0.0) {
      const double st = sqrt(s2), ct = q[0];
      kk = 2.0 * ((ct < 0.0) ? atan2(-st, -ct) : atan2(st, ct)) / st;
    }
    g.r12[3 * (size_t)k] = q1 * kk;
    g.r12[3 * (size_t)k + 1] = q2 * kk;
    g.r12[3 * (size_t)k + 2] = q3 * kk;
  }
  return DSM_OK;
}

// Step 4.  From the filter's per-edge state and relative rotations (component order) and the orientations: the outputs of
// the call, the largest component of the surviving edges (:1000-1003, the same tie rule).
inline void ra_write_outputs(const RaGraph& g, const std::vector<uint8_t>& st8, const std::vector<double>& relh, const std::vector<double>& Rh,
                             uint32_t* image_ids_out, double* orientations_out, uint8_t* image_in_final_cc, uint32_t* n_images_out,
                             uint8_t* edge_state, double* relative_rotations_out, uint32_t* num_filtered_edges,
                             uint32_t* num_final_images) {
  std::vector<std::pair<uint32_t, uint32_t>> kept;
  for (uint32_t k = 0; k < g.M; ++k) {
    edge_state[g.ce_edges[k].orig] = st8[k];
    if (st8[k] == 3) {
      kept.emplace_back(g.ce_edges[k].lo, g.ce_edges[k].hi);
      for (int c = 0; c < 3; ++c) relative_rotations_out[3 * (size_t)g.ce_edges[k].orig + c] = relh[3 * (size_t)k + c];
    } else {
      ++*num_filtered_edges;
    }
  }
  std::vector<uint8_t> fin;
  largest_component(g.N, kept, fin);
  for (uint32_t v = 0; v < g.N; ++v) {
    image_ids_out[v] = g.cimg[v];
    for (int c = 0; c < 3; ++c) orientations_out[3 * (size_t)v + c] = Rh[3 * (size_t)v + c];
    image_in_final_cc[v] = fin[v];
    *num_final_images += fin[v];
  }
  *n_images_out = g.N;
}

}  // namespace

#endif  // DAGSFM_AMD_CSRC_ROTATION_GRAPH_H_
