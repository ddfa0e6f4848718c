// view_graph_clustering.hip -- partition of the view graph into overlapping clusters ("View-graph clustering").
//   DistributedMapperController::ClusteringScenes   src/controllers/distributed_mapper_controller.cpp:633-657
//   ImageClustering::Cut / Expand                  src/clustering/image_clustering.cpp:68-128, 159-199, 451-624
//   SpectralCluster::ComputeCluster                src/clustering/spectral_cluster.cpp:52-176
//   KMeans (k-means++ init, Lloyd)                 src/clustering/kmeans.h:158-235
// SPECTRAL: the k algebraically smallest eigenvectors of L = D_cnt - S (D_cnt counts edges, S holds the inlier counts; the
// reference's operator as it is) by a Chebyshev-filtered subspace iteration on a block of ncv = min(2k, N) vectors: every
// iteration filters the block with a polynomial in L that damps the Ritz interval above the block, orthonormalises it
// (shifted Cholesky QR, then Cholesky QR twice) and runs Rayleigh-Ritz.  The block lives on the device as [N][ncv] (row n = the image of the n-th
// smallest id); the products with L are gathers over a CSR sorted by neighbour, the tall-skinny products are per-chunk tiles
// summed in chunk order, so the result is the same bytes from run to run and for every order of the input list.  The
// ncv x ncv Cholesky factors and the Rayleigh-Ritz eigenproblem (cyclic Jacobi) run on the host, in a fixed order.
// k-means runs on the rows of the first k Ritz vectors: the device computes the distances, assignments and centroid sums,
// the host draws the k-means++ centres with the real std::mt19937_64 / std::discrete_distribution on those distances.
// Cut's bookkeeping and Expand run on the host.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "ctx.h"
#include "graph_edges.h"

namespace {

constexpr int CL_BLOCK = 256;
constexpr int CL_TILE = 16;          // Gram tiles: 16 x 16 outputs per block, 16 rows per step
constexpr int CL_MAX_CHUNKS = 64;    // row chunks of a Gram product (partials are [chunks][ncv][ncv])
constexpr double kClFilterGrowth = 1e7;  // largest amplification of one filter: keeps cond(Y^T Y) below 1e14
constexpr int kClMaxDegree = 24;
constexpr int kClDefaultMaxIterations = 1000;  // Spectra SymEigsSolver::compute(maxit = 1000)

struct KmCtl {
  int done;        // 1 once a Lloyd iteration changed no assignment: later iterations are no-ops
  int iters;       // Lloyd iterations run
  int changed[2];  // an assignment of iteration t changed, slot t & 1
};

// ---------------------------------------------------------------- block kernels (row-major [N][m])
__device__ inline uint64_t splitmix64(uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// the starting block: a hash of (image id, column) in [-1, 1), independent of the input order
__global__ void __launch_bounds__(CL_BLOCK) k_cl_start(uint32_t N, int m, const uint32_t* __restrict__ ids, double* __restrict__ X) {
  const size_t i = (size_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= (size_t)N * m) return;
  const uint32_t n = (uint32_t)(i / m), j = (uint32_t)(i % m);
  const uint64_t h = splitmix64(((uint64_t)ids[n] << 32) ^ (uint64_t)j ^ 0x5bd1e995ull);
  X[i] = (double)(h >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
}

// Y = alpha * (L X - c X) + beta * Xp  (Xp unused when beta == 0); (L x)_n = cnt_n x_n - sum_p w_p x_nb(p), the row in
// ascending neighbour order
__global__ void __launch_bounds__(CL_BLOCK) k_cl_spmm(uint32_t N, int m, const uint32_t* __restrict__ off, const uint32_t* __restrict__ nb,
                                                      const double* __restrict__ w, const double* __restrict__ X, double alpha, double c,
                                                      double beta, const double* __restrict__ Xp, double* __restrict__ Y) {
  const size_t i = (size_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= (size_t)N * m) return;
  const uint32_t n = (uint32_t)(i / m), j = (uint32_t)(i % m);
  double s = 0.0;
  for (uint32_t p = off[n]; p < off[n + 1]; ++p) s += w[p] * X[(size_t)nb[p] * m + j];
  const double x = X[i];
  const double lx = (double)(off[n + 1] - off[n]) * x - s;
  double y = alpha * (lx - c * x);
  if (beta != 0.0) y += beta * Xp[i];
  Y[i] = y;
}

// per-chunk partials of A^T B (both [N][m]): P[chunk][a][b] = sum over the chunk's rows, in row order
__global__ void __launch_bounds__(CL_BLOCK) k_cl_gram(uint32_t N, int m, uint32_t chunk_rows, const double* __restrict__ A,
                                                      const double* __restrict__ B, double* __restrict__ P) {
  __shared__ double sa[CL_TILE][CL_TILE + 1], sb[CL_TILE][CL_TILE + 1];
  const int tx = threadIdx.x % CL_TILE, ty = threadIdx.x / CL_TILE;
  const int a = blockIdx.y * CL_TILE + ty, b = blockIdx.x * CL_TILE + tx;
  const uint32_t r0 = blockIdx.z * chunk_rows, r1 = min(N, r0 + chunk_rows);
  double acc = 0.0;
  for (uint32_t r = r0; r < r1; r += CL_TILE) {
    const uint32_t row = r + ty;  // thread (ty, tx) loads row r + ty, column tx of both tiles
    const int ca = blockIdx.y * CL_TILE + tx, cb = blockIdx.x * CL_TILE + tx;
    sa[ty][tx] = (row < r1 && ca < m) ? A[(size_t)row * m + ca] : 0.0;
    sb[ty][tx] = (row < r1 && cb < m) ? B[(size_t)row * m + cb] : 0.0;
    __syncthreads();
    for (int rr = 0; rr < CL_TILE; ++rr) acc += sa[rr][ty] * sb[rr][tx];
    __syncthreads();
  }
  if (a < m && b < m) P[((size_t)blockIdx.z * m + a) * m + b] = acc;
}

// out[i] = sum over chunks of P[chunk][i], in chunk order
__global__ void __launch_bounds__(CL_BLOCK) k_cl_sum_chunks(size_t count, int n_chunks, const double* __restrict__ P, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= count) return;
  double s = 0.0;
  for (int c = 0; c < n_chunks; ++c) s += P[(size_t)c * count + i];
  out[i] = s;
}

// Y = X M (X [N][m], M [m][m] row-major), the inner sum in index order
__global__ void __launch_bounds__(CL_BLOCK) k_cl_rmul(uint32_t N, int m, const double* __restrict__ X, const double* __restrict__ M,
                                                      double* __restrict__ Y) {
  const size_t i = (size_t)blockIdx.x * CL_BLOCK + threadIdx.x;
  if (i >= (size_t)N * m) return;
  const size_t n = i / m;
  const int j = (int)(i % m);
  const double* x = X + n * m;
  double s = 0.0;
  for (int q = 0; q < m; ++q) s += x[q] * M[(size_t)q * m + j];
  Y[i] = s;
}

// per-chunk partials of ||LX_j - theta_j X_j||^2 for the first k columns: P[chunk][j]
__global__ void __launch_bounds__(CL_BLOCK) k_cl_resid(uint32_t N, int m, int k, uint32_t chunk_rows, const double* __restrict__ X,
                                                       const double* __restrict__ LX, const double* __restrict__ theta,
                                                       double* __restrict__ P) {
  const uint32_t r0 = blockIdx.x * chunk_rows, r1 = min(N, r0 + chunk_rows);
  for (int j = threadIdx.x; j < k; j += CL_BLOCK) {
    double s = 0.0;
    for (uint32_t r = r0; r < r1; ++r) {
      const double d = LX[(size_t)r * m + j] - theta[j] * X[(size_t)r * m + j];
      s += d * d;
    }
    P[(size_t)blockIdx.x * k + j] = s;
  }
}

// ---------------------------------------------------------------- k-means on the rows of the first k columns of X [N][m]
__device__ inline double sqdist(const double* __restrict__ x, const double* __restrict__ c, int k) {
  double s = 0.0;
  for (int j = 0; j < k; ++j) {
    const double d = x[j] - c[j];
    s += d * d;
  }
  return s;
}

// centre slot `slot` of C [k][k] = row `row` of X
__global__ void k_km_take(int m, int k, const double* __restrict__ X, uint32_t row, int slot, double* __restrict__ C) {
  for (int j = threadIdx.x; j < k; j += blockDim.x) C[(size_t)slot * k + j] = X[(size_t)row * m + j];
}

// MinimumDistanceToAnyCenter, incrementally: dist_n = min(dist_n, ||x_n - C_slot||^2) (std::min keeps dist_n on a tie)
__global__ void __launch_bounds__(CL_BLOCK) k_km_mindist(uint32_t N, int m, int k, const double* __restrict__ X, const double* __restrict__ C,
                                                         int slot, double* __restrict__ dist) {
  const uint32_t n = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (n >= N) return;
  const double d = sqdist(X + (size_t)n * m, C + (size_t)slot * k, k);
  const double o = slot == 0 ? DBL_MAX : dist[n];
  dist[n] = d < o ? d : o;
}

// NearestCenterID (strict <: the lower centre wins a tie, a NaN centre never wins); a change sets the iteration's flag
__global__ void __launch_bounds__(CL_BLOCK) k_km_assign(uint32_t N, int m, int k, const double* __restrict__ X, const double* __restrict__ C,
                                                        uint32_t* __restrict__ assign, KmCtl* ctl, int t) {
  if (ctl->done) return;
  const uint32_t n = blockIdx.x * CL_BLOCK + threadIdx.x;
  if (n >= N) return;
  const double* x = X + (size_t)n * m;
  double best = DBL_MAX;
  uint32_t arg = (uint32_t)k;
  for (int c = 0; c < k; ++c) {
    const double d = sqdist(x, C + (size_t)c * k, k);
    if (d < best) {
      best = d;
      arg = (uint32_t)c;
    }
  }
  if (assign[n] != arg) {
    assign[n] = arg;
    ctl->changed[t & 1] = 1;  // a flag, every writer writes 1
  }
}

// ComputeCenterOfMass: one block per centre, the sums in point order; an empty centre is 0 / 0 = NaN as in the reference
__global__ void __launch_bounds__(CL_BLOCK) k_km_centroids(uint32_t N, int m, int k, const double* __restrict__ X,
                                                           const uint32_t* __restrict__ assign, double* __restrict__ C, const KmCtl* ctl) {
  if (ctl->done) return;
  const uint32_t c = blockIdx.x;
  for (int j = threadIdx.x; j < k; j += CL_BLOCK) {
    double s = 0.0;
    uint32_t cnt = 0;
    for (uint32_t n = 0; n < N; ++n)
      if (assign[n] == c) {
        s += X[(size_t)n * m + j];
        ++cnt;
      }
    C[(size_t)c * k + j] = s / (double)cnt;
  }
}

// end of Lloyd iteration t (one thread): stop when nothing changed, clear the next iteration's flag
__global__ void k_km_check(KmCtl* ctl, int t) {
  if (ctl->done) return;
  ctl->iters = t + 1;
  if (!ctl->changed[t & 1]) ctl->done = 1;
  ctl->changed[(t + 1) & 1] = 0;
}

// ---------------------------------------------------------------- host linear algebra (ncv x ncv, fixed order)
// G = R^T R (R upper, row-major); false on a non-positive pivot
bool cholesky_upper(int m, const std::vector<double>& G, std::vector<double>& R) {
  R.assign((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) {
    double d = G[(size_t)i * m + i];
    for (int p = 0; p < i; ++p) d -= R[(size_t)p * m + i] * R[(size_t)p * m + i];
    if (!(d > 0.0)) return false;
    const double rii = std::sqrt(d);
    R[(size_t)i * m + i] = rii;
    for (int j = i + 1; j < m; ++j) {
      double s = G[(size_t)i * m + j];
      for (int p = 0; p < i; ++p) s -= R[(size_t)p * m + i] * R[(size_t)p * m + j];
      R[(size_t)i * m + j] = s / rii;
    }
  }
  return true;
}

// inverse of an upper-triangular R (upper-triangular, row-major)
void invert_upper(int m, const std::vector<double>& R, std::vector<double>& Ri) {
  Ri.assign((size_t)m * m, 0.0);
  for (int j = 0; j < m; ++j) {
    Ri[(size_t)j * m + j] = 1.0 / R[(size_t)j * m + j];
    for (int i = j - 1; i >= 0; --i) {
      double s = 0.0;
      for (int p = i + 1; p <= j; ++p) s += R[(size_t)i * m + p] * Ri[(size_t)p * m + j];
      Ri[(size_t)i * m + j] = -s / R[(size_t)i * m + i];
    }
  }
}

// cyclic Jacobi on the symmetric A (destroyed): eigenvalues ascending in theta, eigenvectors in the columns of Z (row-major);
// equal eigenvalues keep their diagonal order
void jacobi_eigen(int m, std::vector<double> A, std::vector<double>& theta, std::vector<double>& Z) {
  std::vector<double> V((size_t)m * m, 0.0);
  for (int i = 0; i < m; ++i) V[(size_t)i * m + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < m; ++i) {
      diag += A[(size_t)i * m + i] * A[(size_t)i * m + i];
      for (int j = i + 1; j < m; ++j) off += A[(size_t)i * m + j] * A[(size_t)i * m + j];
    }
    if (off <= 1e-34 * diag || off == 0.0) break;
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1; q < m; ++q) {
        const double apq = A[(size_t)p * m + q];
        const double app = A[(size_t)p * m + p], aqq = A[(size_t)q * m + q];
        if (apq == 0.0 || std::fabs(apq) <= 1e-300) continue;
        if (std::fabs(apq) < 1e-18 * std::sqrt(std::fabs(app * aqq))) {
          A[(size_t)p * m + q] = A[(size_t)q * m + p] = 0.0;
          continue;
        }
        const double tau = (aqq - app) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int r = 0; r < m; ++r) {  // A <- A J (columns p, q)
          const double arp = A[(size_t)r * m + p], arq = A[(size_t)r * m + q];
          A[(size_t)r * m + p] = c * arp - s * arq;
          A[(size_t)r * m + q] = s * arp + c * arq;
        }
        for (int r = 0; r < m; ++r) {  // A <- J^T A (rows p, q)
          const double apr = A[(size_t)p * m + r], aqr = A[(size_t)q * m + r];
          A[(size_t)p * m + r] = c * apr - s * aqr;
          A[(size_t)q * m + r] = s * apr + c * aqr;
        }
        A[(size_t)p * m + q] = A[(size_t)q * m + p] = 0.0;
        for (int r = 0; r < m; ++r) {
          const double vrp = V[(size_t)r * m + p], vrq = V[(size_t)r * m + q];
          V[(size_t)r * m + p] = c * vrp - s * vrq;
          V[(size_t)r * m + q] = s * vrp + c * vrq;
        }
      }
  }
  std::vector<int> ord(m);
  for (int i = 0; i < m; ++i) ord[i] = i;
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return A[(size_t)a * m + a] < A[(size_t)b * m + b]; });
  theta.resize(m);
  Z.assign((size_t)m * m, 0.0);
  for (int j = 0; j < m; ++j) {
    theta[j] = A[(size_t)ord[j] * m + ord[j]];
    for (int r = 0; r < m; ++r) Z[(size_t)r * m + j] = V[(size_t)r * m + ord[j]];
  }
}

// ---------------------------------------------------------------- Cut bookkeeping + Expand (host)
struct ClusterState {
  std::vector<std::vector<uint32_t>> members;  // images (vertex numbers) of each inter cluster, in insertion order
  std::vector<std::vector<uint32_t>> of;       // the clusters holding each image (ascending)
  std::vector<uint64_t> repeated;              // sum over j != i of CommonImagesNum(i, j), kept incrementally
  std::vector<uint8_t> sticky;                 // IsConditionSatisfy
  std::vector<uint64_t> n_edges;
  float completeness_ratio = 0.5f;

  bool has(uint32_t c, uint32_t v) const { return std::binary_search(of[v].begin(), of[v].end(), c); }
  void add(uint32_t c, uint32_t v) {
    for (uint32_t i : of[v]) ++repeated[i];
    repeated[c] += of[v].size();
    of[v].insert(std::upper_bound(of[v].begin(), of[v].end(), c), c);
    members[c].push_back(v);
  }
  uint32_t common(uint32_t a, uint32_t b) const {
    const uint32_t s = members[a].size() <= members[b].size() ? a : b, o = s == a ? b : a;
    uint32_t n = 0;
    for (uint32_t v : members[s]) n += has(o, v);
    return n;
  }
  // IsSatisfyCompletenessRatio (image_clustering.cpp:451-471): float ratio, sticky once above; an empty cluster is 0 / 0 = NaN
  bool satisfied(uint32_t c) {
    if (sticky[c]) return true;
    const float ratio = (float)repeated[c] / (float)members[c].size();
    if (ratio <= completeness_ratio) return false;
    sticky[c] = 1;
    return true;
  }
};

}  // namespace

extern "C" void dsm_default_clustering_options(dsm_clustering_options* o) {
  if (!o) return;
  *o = dsm_clustering_options{};
  o->num_images_ub = 100;
  o->image_overlap = 50;
  o->completeness_ratio = 0.5f;
  o->expand = 1;
  o->max_kmeans_iterations = 0;
  o->max_eigen_iterations = 0;
  o->eigen_tolerance = 1e-10;
}

extern "C" int dsm_get_clustering_spectrum(dsm_ctx* ctx, double* values, uint32_t values_capacity, double* vectors,
                                           uint64_t vectors_capacity, uint32_t* n_values, uint32_t* n_rows, uint32_t* n_cols) {
  if (!ctx || !n_values || !n_rows || !n_cols || (values_capacity && !values) || (vectors_capacity && !vectors))
    return DSM_ERR_INVALID_ARGUMENT;
  *n_values = (uint32_t)ctx->cluster_ritz.size();
  *n_rows = ctx->cluster_rows;
  *n_cols = ctx->cluster_cols;
  for (uint32_t i = 0; i < values_capacity && i < *n_values; ++i) values[i] = ctx->cluster_ritz[i];
  for (uint64_t i = 0; i < vectors_capacity && i < ctx->cluster_vectors.size(); ++i) vectors[i] = ctx->cluster_vectors[i];
  return DSM_OK;
}

extern "C" int dsm_view_graph_cluster(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const int32_t* weights, const uint8_t* use,
                                      const uint32_t* labels_in, const dsm_clustering_options* options, uint32_t* image_ids_out,
                                      uint32_t* labels_out, uint32_t* n_images_out, int32_t* edge_cluster, uint32_t* cluster_offsets,
                                      uint32_t* cluster_images, uint32_t* n_clusters_out, dsm_clustering_report* report) {
  if (!ctx) return DSM_ERR_INVALID_ARGUMENT;
  if (!n_images_out || !n_clusters_out || !cluster_offsets ||
      (n_pairs && (!pairs || !weights || !image_ids_out || !labels_out || !edge_cluster || !cluster_images)))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: NULL argument");
  if (n_pairs > (UINT32_MAX >> 2)) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: too many pairs");
  dsm_clustering_options o;
  if (options)
    o = *options;
  else
    dsm_default_clustering_options(&o);
  if (o.num_images_ub == 0 || o.image_overlap <= 2 || !(o.completeness_ratio <= 1.0f) || o.max_eigen_iterations < 0 ||
      !(o.eigen_tolerance > 0.0))
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: option out of range");
  dsm_clustering_report rep{};
  *n_images_out = 0;
  *n_clusters_out = 0;
  cluster_offsets[0] = 0;
  if (report) *report = rep;
  for (uint32_t e = 0; e < n_pairs; ++e) {
    if (use && !use[e]) continue;
    if (pairs[2 * e] == pairs[2 * e + 1]) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: image_id1 == image_id2");
    if (weights[e] < 0) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: negative weight");
  }
  // unique used edges (the first occurrence of an unordered pair wins), images renumbered by ascending id
  std::vector<uint32_t> ids;
  const std::vector<GraphEdge> uniq = graph_unique_edges(n_pairs, pairs, use, ids);  // canonical (lo, hi) order
  const uint32_t N = (uint32_t)ids.size();
  const uint32_t M = (uint32_t)uniq.size();
  const uint32_t k_ref = N / o.num_images_ub;
  const uint32_t k = std::max<uint32_t>(1u, k_ref);
  uint32_t n_clusters = k;
  if (labels_in) {
    for (uint32_t v = 0; v < N; ++v) {
      if (labels_in[v] >= N) return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: label >= number of images");
      n_clusters = std::max(n_clusters, labels_in[v] + 1);
    }
  } else if (k > 1 && k >= N) {
    return dsm_fail(ctx, DSM_ERR_INVALID_ARGUMENT, "dsm_view_graph_cluster: k >= images (Spectra needs nev < ncv <= n)");
  }
  for (uint32_t e = 0; e < n_pairs; ++e) edge_cluster[e] = -1;
  if (M == 0) return DSM_OK;
  rep.num_images = N;
  rep.num_edges = M;
  rep.num_clusters = n_clusters;
  ctx->cluster_ritz.clear();
  ctx->cluster_vectors.clear();
  ctx->cluster_rows = ctx->cluster_cols = 0;

  std::vector<uint32_t> label(N, 0);
  int rc = DSM_OK;
  if (labels_in) {
    for (uint32_t v = 0; v < N; ++v) label[v] = labels_in[v];
  } else if (k > 1) {
    // ---------------------------------------------------------- SPECTRAL on the device
    const int m = (int)std::min<uint32_t>(2 * k, N);
    rep.ncv = (uint32_t)m;
    // CSR over images, entries sorted by neighbour; Gershgorin's upper bound of L
    std::vector<uint32_t> off, nb, eidx;
    graph_neighbour_csr(N, uniq, off, nb, eidx);
    std::vector<double> wv(2 * (size_t)M);
    for (size_t p = 0; p < wv.size(); ++p) wv[p] = (double)weights[uniq[eidx[p]].orig];
    double bup = -DBL_MAX;
    for (uint32_t v = 0; v < N; ++v) {
      double s = (double)(off[v + 1] - off[v]);
      for (uint32_t p = off[v]; p < off[v + 1]; ++p) s += wv[p];
      bup = std::max(bup, s);
    }
    hipError_t he = hipSetDevice(ctx->device);
    if (he != hipSuccess) return dsm_fail(ctx, DSM_ERR_HIP, hipGetErrorString(he));
    hipStream_t st = ctx->stream;
    const size_t nm = (size_t)N * m, mm = (size_t)m * m;
    const int n_chunks = (int)std::min<uint32_t>(CL_MAX_CHUNKS, (N + 255) / 256);
    uint32_t chunk_rows = (N + n_chunks - 1) / n_chunks;
    chunk_rows = (chunk_rows + CL_TILE - 1) / CL_TILE * CL_TILE;
    const int grid_chunks = (int)((N + chunk_rows - 1) / chunk_rows);
    const unsigned nb_nm = (unsigned)((nm + CL_BLOCK - 1) / CL_BLOCK), nb_v = (N + CL_BLOCK - 1) / CL_BLOCK;
    DevBuf d_ids, d_off, d_nb, d_w, d_B[5], d_P, d_S, d_M, d_theta, d_C, d_dist, d_assign, d_ctl;
    DevEvent ev0, ev1;
    HIPTRY(d_ids.reserve((size_t)N * 4));
    HIPTRY(d_off.reserve(((size_t)N + 1) * 4));
    HIPTRY(d_nb.reserve((size_t)M * 8));
    HIPTRY(d_w.reserve((size_t)M * 16));
    for (DevBuf& b : d_B) HIPTRY(b.reserve(nm * 8));
    HIPTRY(d_P.reserve((size_t)grid_chunks * mm * 8));
    HIPTRY(d_S.reserve(mm * 8));
    HIPTRY(d_M.reserve(mm * 8));
    HIPTRY(d_theta.reserve((size_t)m * 8));
    HIPTRY(d_C.reserve((size_t)k * k * 8));
    HIPTRY(d_dist.reserve((size_t)N * 8));
    HIPTRY(d_assign.reserve((size_t)N * 4));
    HIPTRY(d_ctl.reserve(sizeof(KmCtl)));
    HIPTRY(hipEventCreate(&ev0.e));
    HIPTRY(hipEventCreate(&ev1.e));
    if (rc == DSM_OK) {
      HIPTRY(hipEventRecord(ev0, st));
      HIPTRY(hipMemcpyAsync(d_ids.p, ids.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
      HIPTRY(hipMemcpyAsync(d_off.p, off.data(), ((size_t)N + 1) * 4, hipMemcpyHostToDevice, st));
      HIPTRY(hipMemcpyAsync(d_nb.p, nb.data(), (size_t)M * 8, hipMemcpyHostToDevice, st));
      HIPTRY(hipMemcpyAsync(d_w.p, wv.data(), (size_t)M * 16, hipMemcpyHostToDevice, st));
    }
    const uint32_t* off_ = d_off.as<uint32_t>();
    const uint32_t* nb_ = d_nb.as<uint32_t>();
    const double* w_ = d_w.as<double>();
    double* B[5];
    for (int i = 0; i < 5; ++i) B[i] = d_B[i].as<double>();
    std::vector<double> G(mm), R, Ri, theta, Z, res2(k);
    // host copy of a Gram product A^T C
    auto gram = [&](const double* A, const double* Cm, std::vector<double>& out) {
      hipLaunchKernelGGL(k_cl_gram, dim3((m + CL_TILE - 1) / CL_TILE, (m + CL_TILE - 1) / CL_TILE, grid_chunks), dim3(CL_BLOCK), 0, st, N, m,
                         chunk_rows, A, Cm, d_P.as<double>());
      hipLaunchKernelGGL(k_cl_sum_chunks, dim3((unsigned)((mm + CL_BLOCK - 1) / CL_BLOCK)), dim3(CL_BLOCK), 0, st, mm, grid_chunks,
                         (const double*)d_P.as<double>(), d_S.as<double>());
      HIPTRY(hipGetLastError());
      HIPTRY(hipMemcpyAsync(out.data(), d_S.p, mm * 8, hipMemcpyDeviceToHost, st));
      HIPTRY(hipStreamSynchronize(st));
    };
    auto rmul = [&](const double* X, const std::vector<double>& Mh, double* Y) {
      HIPTRY(hipMemcpyAsync(d_M.p, Mh.data(), mm * 8, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_cl_rmul, dim3(nb_nm), dim3(CL_BLOCK), 0, st, N, m, X, (const double*)d_M.as<double>(), Y);
    };
    auto spmm = [&](const double* X, double alpha, double c, double beta, const double* Xp, double* Y) {
      hipLaunchKernelGGL(k_cl_spmm, dim3(nb_nm), dim3(CL_BLOCK), 0, st, N, m, off_, nb_, w_, X, alpha, c, beta, Xp, Y);
      rep.operator_applications += (uint64_t)m;
    };
    // Cholesky QR of the block in B[x] into B[y]: false on a breakdown.  shifted: G + s I with Fukaya et al.'s shift
    // s = 11 (N m + m (m + 1)) u ||G|| (trace as the norm bound), the first pass of shifted CholeskyQR3 for an ill-conditioned block
    auto cholqr = [&](int x, int y, bool shifted) {
      gram(B[x], B[x], G);
      if (rc != DSM_OK) return true;
      if (shifted) {
        double tr = 0.0;
        for (int i = 0; i < m; ++i) tr += G[(size_t)i * m + i];
        const double sh = 11.0 * ((double)N * m + (double)m * (m + 1)) * DBL_EPSILON * tr;
        for (int i = 0; i < m; ++i) G[(size_t)i * m + i] += sh;
      }
      if (!cholesky_upper(m, G, R)) return false;
      invert_upper(m, R, Ri);
      rmul(B[x], Ri, B[y]);
      return true;
    };
    // Rayleigh-Ritz of the orthonormal block B[q]: X = Q Z -> B[x], LX = (L Q) Z -> B[lx]; theta ascending
    auto rayleigh_ritz = [&](int q, int w, int x, int lx) {
      spmm(B[q], 1.0, 0.0, 0.0, nullptr, B[w]);
      gram(B[q], B[w], G);
      if (rc != DSM_OK) return;
      for (int i = 0; i < m; ++i)  // symmetrise the rounding of Q^T L Q
        for (int j = i + 1; j < m; ++j) G[(size_t)i * m + j] = G[(size_t)j * m + i] = 0.5 * (G[(size_t)i * m + j] + G[(size_t)j * m + i]);
      jacobi_eigen(m, G, theta, Z);
      rmul(B[q], Z, B[x]);
      rmul(B[w], Z, B[lx]);
    };
    const double eps23 = std::pow(DBL_EPSILON, 2.0 / 3.0);
    const int max_it = o.max_eigen_iterations > 0 ? o.max_eigen_iterations : kClDefaultMaxIterations;
    int X = 0, LX = 1;  // the current Ritz block and L times it
    bool converged = false, breakdown = false;
    if (rc == DSM_OK) {
      hipLaunchKernelGGL(k_cl_start, dim3(nb_nm), dim3(CL_BLOCK), 0, st, N, m, (const uint32_t*)d_ids.as<uint32_t>(), B[2]);
      if (!cholqr(2, 3, false) || !cholqr(3, 2, false)) breakdown = true;
      if (!breakdown && rc == DSM_OK) rayleigh_ritz(2, 3, X, LX);
    }
    for (int it = 0; rc == DSM_OK && !breakdown && !converged && it < max_it; ++it) {
      // Chebyshev filter of degree d on [a, bup] (Zhou & Saad's scaled three-term recurrence), scaled at a0
      const double a = theta[m - 1], a0 = theta[0];
      int fin = X;
      if (a < bup && m < (int)N) {
        const double e = 0.5 * (bup - a), c = 0.5 * (bup + a);
        const double t = std::max(1.0 + 1e-12, (c - a0) / e);
        const int deg = std::max(1, std::min(kClMaxDegree, (int)(std::acosh(kClFilterGrowth) / std::acosh(t))));
        double sigma = e / (a0 - c);
        const double sigma1 = sigma, gamma = 2.0 / sigma1;
        // three buffers in a cycle: X (no longer needed once filtered) and the two after it
        int p0 = X, p1 = (X + 1) % 5, p2 = (X + 2) % 5;
        spmm(B[p0], sigma1 / e, c, 0.0, nullptr, B[p1]);
        for (int i = 2; i <= deg; ++i) {
          const double sigma2 = 1.0 / (gamma - sigma);
          spmm(B[p1], 2.0 * sigma2 / e, c, -sigma * sigma2, B[p0], B[p2]);
          const int tmp = p0;
          p0 = p1;
          p1 = p2;
          p2 = tmp;
          sigma = sigma2;
        }
        fin = p1;
      }
      // orthonormalise (shifted CholeskyQR3) through two free buffers, then Rayleigh-Ritz into (X, LX) again
      int fr[4], nf = 0;
      for (int i = 0; i < 5; ++i)
        if (i != fin) fr[nf++] = i;
      if (!cholqr(fin, fr[0], true) || !cholqr(fr[0], fr[1], false) || !cholqr(fr[1], fr[0], false)) {
        breakdown = true;
        break;
      }
      if (rc != DSM_OK) break;
      // fr[0] = Q; the Ritz block goes to X / LX, both distinct from fr[0] and its L-product buffer
      int q = fr[0], wq = -1, nx = -1, nlx = -1;
      for (int i = 0; i < 5; ++i)
        if (i != q) {
          if (wq < 0) wq = i;
          else if (nx < 0) nx = i;
          else if (nlx < 0) nlx = i;
        }
      rayleigh_ritz(q, wq, nx, nlx);
      X = nx;
      LX = nlx;
      rep.eigen_iterations = (uint32_t)(it + 1);
      if (rc != DSM_OK) break;
      HIPTRY(hipMemcpyAsync(d_theta.p, theta.data(), (size_t)m * 8, hipMemcpyHostToDevice, st));
      hipLaunchKernelGGL(k_cl_resid, dim3(grid_chunks), dim3(CL_BLOCK), 0, st, N, m, (int)k, chunk_rows, (const double*)B[X],
                         (const double*)B[LX], (const double*)d_theta.as<double>(), d_P.as<double>());
      hipLaunchKernelGGL(k_cl_sum_chunks, dim3((k + CL_BLOCK - 1) / CL_BLOCK), dim3(CL_BLOCK), 0, st, (size_t)k, grid_chunks,
                         (const double*)d_P.as<double>(), d_S.as<double>());
      HIPTRY(hipGetLastError());
      HIPTRY(hipMemcpyAsync(res2.data(), d_S.p, (size_t)k * 8, hipMemcpyDeviceToHost, st));
      HIPTRY(hipStreamSynchronize(st));
      double worst = 0.0, worst_ratio = 0.0;
      for (uint32_t j = 0; j < k; ++j) {
        const double r = std::sqrt(res2[j]);
        worst = std::max(worst, r);
        worst_ratio = std::max(worst_ratio, r / std::max(eps23, std::fabs(theta[j])));
      }
      rep.max_eigen_residual = worst;
      rep.max_eigen_residual_ratio = worst_ratio;
      converged = worst_ratio <= o.eigen_tolerance;
    }
    if (!theta.empty()) {
      ctx->cluster_ritz = theta;
      rep.eigen_gap = m > (int)k ? theta[k] - theta[k - 1] : 0.0;
    }
    if (rc == DSM_OK && (breakdown || !converged)) {
      ctx->err = breakdown ? "dsm_view_graph_cluster: the Cholesky QR of the filtered block broke down"
                           : "dsm_view_graph_cluster: the eigen-solver ended at a relative residual of " +
                                 std::to_string(rep.max_eigen_residual_ratio);
      rc = DSM_ERR_NOT_CONVERGED;
    }
    // ---------------------------------------------------------- k-means on the rows of the first k Ritz vectors
    std::vector<double> dist(N);
    const int kk = (int)k;
    const double* Xk = B[X];
    if (rc == DSM_OK) {
      std::mt19937_64 rng(std::mt19937_64::default_seed);
      std::uniform_int_distribution<size_t> first(0, N - 1);
      hipLaunchKernelGGL(k_km_take, dim3(1), dim3(CL_BLOCK), 0, st, m, kk, Xk, (uint32_t)first(rng), 0, d_C.as<double>());
      for (int c = 1; c < kk && rc == DSM_OK; ++c) {
        hipLaunchKernelGGL(k_km_mindist, dim3(nb_v), dim3(CL_BLOCK), 0, st, N, m, kk, Xk, (const double*)d_C.as<double>(), c - 1,
                           d_dist.as<double>());
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(dist.data(), d_dist.p, (size_t)N * 8, hipMemcpyDeviceToHost, st));
        HIPTRY(hipStreamSynchronize(st));
        std::discrete_distribution<size_t> draw(dist.cbegin(), dist.cend());
        hipLaunchKernelGGL(k_km_take, dim3(1), dim3(CL_BLOCK), 0, st, m, kk, Xk, (uint32_t)draw(rng), c, d_C.as<double>());
      }
      HIPTRY(hipMemsetAsync(d_ctl.p, 0, sizeof(KmCtl), st));
      std::vector<uint32_t> init(N, k);
      HIPTRY(hipMemcpyAsync(d_assign.p, init.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
      KmCtl h{};
      const int batch = 8;
      for (int t0 = 0; rc == DSM_OK && !h.done; t0 += batch) {
        if (o.max_kmeans_iterations && (uint32_t)t0 >= o.max_kmeans_iterations) break;
        for (int t = t0; t < t0 + batch && (!o.max_kmeans_iterations || (uint32_t)t < o.max_kmeans_iterations); ++t) {
          hipLaunchKernelGGL(k_km_assign, dim3(nb_v), dim3(CL_BLOCK), 0, st, N, m, kk, Xk, (const double*)d_C.as<double>(),
                             d_assign.as<uint32_t>(), d_ctl.as<KmCtl>(), t);
          hipLaunchKernelGGL(k_km_centroids, dim3(kk), dim3(CL_BLOCK), 0, st, N, m, kk, Xk, (const uint32_t*)d_assign.as<uint32_t>(),
                             d_C.as<double>(), (const KmCtl*)d_ctl.as<KmCtl>());
          hipLaunchKernelGGL(k_km_check, dim3(1), dim3(1), 0, st, d_ctl.as<KmCtl>(), t);
        }
        HIPTRY(hipGetLastError());
        HIPTRY(hipMemcpyAsync(&h, d_ctl.p, sizeof(KmCtl), hipMemcpyDeviceToHost, st));
        HIPTRY(hipStreamSynchronize(st));
      }
      rep.kmeans_iterations = (uint32_t)h.iters;
      HIPTRY(hipEventRecord(ev1, st));
      HIPTRY(hipMemcpyAsync(label.data(), d_assign.p, (size_t)N * 4, hipMemcpyDeviceToHost, st));
      std::vector<double> Xh(nm);
      HIPTRY(hipMemcpyAsync(Xh.data(), Xk, nm * 8, hipMemcpyDeviceToHost, st));
      HIPTRY(hipStreamSynchronize(st));
      ctx->cluster_vectors.resize((size_t)N * k);
      for (uint32_t n = 0; n < N; ++n)
        for (uint32_t j = 0; j < k; ++j) ctx->cluster_vectors[(size_t)n * k + j] = Xh[(size_t)n * m + j];
      ctx->cluster_rows = N;
      ctx->cluster_cols = k;
      HIPTRY(dev_events_ms(ev0, ev1, &rep.device_ms));
    }
    if (rc != DSM_OK) (void)hipStreamSynchronize(st);
    if (rc != DSM_OK) {
      if (report) *report = rep;
      return rc;
    }
  }

  for (uint32_t v = 0; v < N; ++v)
    if (label[v] >= n_clusters) return dsm_fail(ctx, DSM_ERR_NOT_CONVERGED, "dsm_view_graph_cluster: a point without a nearest centre");
  // ------------------------------------------------------------ Cut (image_clustering.cpp:68-128): intra clusters, lost edges
  ClusterState cs;
  cs.completeness_ratio = o.completeness_ratio;
  cs.members.resize(n_clusters);
  cs.of.resize(N);
  cs.repeated.assign(n_clusters, 0);
  cs.sticky.assign(n_clusters, 0);
  cs.n_edges.assign(n_clusters, 0);
  for (uint32_t v = 0; v < N; ++v) cs.add(label[v], v);
  std::vector<GraphEdge> in_order(uniq);  // input order of the surviving occurrences
  std::sort(in_order.begin(), in_order.end(), [](const GraphEdge& l, const GraphEdge& r) { return l.orig < r.orig; });
  std::map<std::pair<uint32_t, uint32_t>, std::vector<GraphEdge>> lost;
  for (const GraphEdge& x : in_order) {
    const uint32_t c1 = label[x.i], c2 = label[x.j];
    if (c1 == c2) {
      edge_cluster[x.orig] = (int32_t)c1;
      ++cs.n_edges[c1];
    } else {
      edge_cluster[x.orig] = -2;
      lost[{std::min(c1, c2), std::max(c1, c2)}].push_back(x);
      ++rep.num_lost_edges;
    }
  }
  // ------------------------------------------------------------ Expand (:159-199, AddLostEdgesBetweenClusters :579-624)
  if (o.expand && n_clusters > 1) {
    for (auto& it : lost) {
      const uint32_t c1 = it.first.first, c2 = it.first.second;
      std::vector<GraphEdge>& le = it.second;
      if (cs.common(c1, c2) > o.image_overlap) continue;
      if (cs.satisfied(c1) && cs.satisfied(c2)) continue;
      std::stable_sort(le.begin(), le.end(), [&](const GraphEdge& l, const GraphEdge& r) { return weights[l.orig] > weights[r.orig]; });
      for (const GraphEdge& x : le) {
        const uint32_t src = x.i, dst = x.j;
        const uint32_t added1 = cs.has(c1, src) ? dst : src;
        const uint32_t added2 = cs.has(c2, src) ? dst : src;
        const bool pick2 = cs.members[c1].size() > cs.members[c2].size();
        const uint32_t c = pick2 ? c2 : c1, added = pick2 ? added2 : added1;
        if (!cs.satisfied(c) && !cs.has(c, added)) {
          cs.add(c, added);
          ++cs.n_edges[c];
          edge_cluster[x.orig] = (int32_t)c;
          ++rep.num_readded_edges;
        }
        if (cs.satisfied(c1) && cs.satisfied(c2)) break;
      }
    }
  }
  // ------------------------------------------------------------ outputs (AnalyzeStatistic :626-632)
  for (uint32_t v = 0; v < N; ++v) {
    image_ids_out[v] = ids[v];
    labels_out[v] = label[v];
  }
  *n_images_out = N;
  uint32_t pos = 0;
  for (uint32_t c = 0; c < n_clusters; ++c) {
    std::vector<uint32_t> mem = cs.members[c];
    std::sort(mem.begin(), mem.end());  // vertex order = id order
    for (uint32_t v : mem) cluster_images[pos++] = ids[v];
    cluster_offsets[c + 1] = pos;
    rep.clustered_images_num += mem.size();
    rep.clustered_edges_num += cs.n_edges[c];
  }
  *n_clusters_out = n_clusters;
  if (report) *report = rep;
  return DSM_OK;
}
