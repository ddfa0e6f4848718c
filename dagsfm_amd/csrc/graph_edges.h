// graph_edges.h -- host-side edge setup of the view-graph stages (view_graph.hip, rotation_averaging.hip,
// view_graph_clustering.hip).
#ifndef DAGSFM_AMD_CSRC_GRAPH_EDGES_H_
#define DAGSFM_AMD_CSRC_GRAPH_EDGES_H_

#include <stdint.h>

#include <algorithm>
#include <vector>

// an edge between the renumbered images lo < hi; i, j: its images in the order of the input pair, orig: its index in the list
struct GraphEdge {
  uint32_t lo, hi, i, j, orig;
};

// The unique edges of the used pairs (use == NULL: all), in (lo, hi) order.  Images are renumbered by ascending id (ids: the
// sorted unique ids of the used pairs), the first occurrence of an unordered pair in list order wins
// (ViewGraph::AddTwoViewGeometry), and a pair of an image with itself is dropped.
static inline std::vector<GraphEdge> graph_unique_edges(uint32_t n_pairs, const uint32_t* pairs, const uint8_t* use,
                                                        std::vector<uint32_t>& ids) {
  ids.clear();
  for (uint32_t e = 0; e < n_pairs; ++e)
    if (!use || use[e]) {
      ids.push_back(pairs[2 * e]);
      ids.push_back(pairs[2 * e + 1]);
    }
  std::sort(ids.begin(), ids.end());
  ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
  auto vid = [&](uint32_t id) { return (uint32_t)(std::lower_bound(ids.begin(), ids.end(), id) - ids.begin()); };
  std::vector<GraphEdge> edges;
  for (uint32_t e = 0; e < n_pairs; ++e)
    if (!use || use[e]) {
      const uint32_t a = vid(pairs[2 * e]), b = vid(pairs[2 * e + 1]);
      if (a != b) edges.push_back(GraphEdge{std::min(a, b), std::max(a, b), a, b, e});
    }
  std::stable_sort(edges.begin(), edges.end(), [](const GraphEdge& l, const GraphEdge& r) { return l.lo != r.lo ? l.lo < r.lo : l.hi < r.hi; });
  std::vector<GraphEdge> uniq;
  for (const GraphEdge& x : edges)  // the first occurrence in list order wins (stable sort)
    if (uniq.empty() || uniq.back().lo != x.lo || uniq.back().hi != x.hi) uniq.push_back(x);
  return uniq;
}

// The CSR over n images of unique edges given in (lo, hi) order: row v holds the neighbours of v ascending, nb[off[v] ..
// off[v + 1]), and edge[p] is the index in `edges` of entry p.  Filling every row with its lower neighbours (the edges'
// lo, ascending in that order) before its upper ones (their hi, ascending) sorts it.
static inline void graph_neighbour_csr(uint32_t n, const std::vector<GraphEdge>& edges, std::vector<uint32_t>& off,
                                       std::vector<uint32_t>& nb, std::vector<uint32_t>& edge) {
  const uint32_t M = (uint32_t)edges.size();
  off.assign((size_t)n + 1, 0);
  for (const GraphEdge& x : edges) {
    off[x.lo + 1]++;
    off[x.hi + 1]++;
  }
  for (uint32_t v = 0; v < n; ++v) off[v + 1] += off[v];
  nb.resize(2 * (size_t)M);
  edge.resize(2 * (size_t)M);
  std::vector<uint32_t> fill(off.begin(), off.end() - 1);
  for (uint32_t k = 0; k < M; ++k) {
    nb[fill[edges[k].hi]] = edges[k].lo;
    edge[fill[edges[k].hi]++] = k;
  }
  for (uint32_t k = 0; k < M; ++k) {
    nb[fill[edges[k].lo]] = edges[k].hi;
    edge[fill[edges[k].lo]++] = k;
  }
}

#endif  // DAGSFM_AMD_CSRC_GRAPH_EDGES_H_
