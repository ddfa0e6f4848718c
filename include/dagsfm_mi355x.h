/*
 * dagsfm_mi355x.h -- C-ABI of the MI355X-native matching + two-view verification path.
 *
 * This is the drop-in boundary for DAGSfM's data-parallel hot path
 * (SURVEY.md section 8b).  Every entry point is `extern "C"`, takes plain pointers
 * and sizes only, returns an int status (0 = DSM_OK) and never aborts.  The
 * reference interfaces each entry point replaces are cited as
 * `/root/reference/<file>:<line>`.
 *
 * Vocabulary follows the reference: images, features (keypoints + 128-D uint8
 * SIFT descriptors), image pairs, FeatureMatches, TwoViewGeometry.
 */
#ifndef DAGSFM_MI355X_H_
#define DAGSFM_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ status */
enum {
  DSM_OK = 0,
  DSM_ERR_INVALID_ARGUMENT = 1, /* reference: CHECK(...) fatal in matching.cc */
  DSM_ERR_NO_DEVICE = 2,        /* reference: Setup() returns false, matching.cc:732-742 */
  DSM_ERR_HIP = 3,              /* a HIP runtime call failed; see dsm_last_error */
  DSM_ERR_OUT_OF_RANGE = 4,
  DSM_ERR_NOT_READY = 5,        /* results requested before the producing call */
  DSM_ERR_NOT_CONVERGED = 6     /* an iterative solve ended above its tolerance; reference: a Cholesky
                                   factorisation fails, RobustRotationEstimator::EstimateRotations returns false */
};

/* ------------------------------------------------------------------ options */

/* Mirrors the matching half of SiftMatchingOptions, src/feature/sift.h:116-165.
 * max_ratio / max_distance are doubles there and are narrowed to float exactly
 * where the reference narrows them (FindBestMatches signature, sift.cc:164-166). */
typedef struct dsm_match_options {
  double max_ratio;        /* default 0.8  */
  double max_distance;     /* default 0.7  */
  int32_t cross_check;     /* default 1    */
  int32_t max_num_matches; /* default 32768; carried for ABI parity only: MatchSiftFeaturesCPU (sift.cc:810-822)
                              ignores it (the SiftGPU matcher alone clamps, sift.cc:200-209), and so does this library */
} dsm_match_options;

/* Mirrors TwoViewGeometry::Options (src/estimators/two_view_geometry.h:105-157)
 * with its embedded RANSACOptions (src/optim/ransac.h:47-72), filled from
 * SiftMatchingOptions exactly as TwoViewGeometryVerifier's ctor does
 * (src/feature/matching.cc:559-568). */
typedef struct dsm_two_view_options {
  uint64_t min_num_inliers;          /* 15   */
  double min_E_F_inlier_ratio;       /* 0.95 */
  double max_H_inlier_ratio;         /* 0.8  */
  double watermark_min_inlier_ratio; /* 0.7  */
  double watermark_border_size;      /* 0.1  */
  int32_t detect_watermark;          /* 1    */
  int32_t multiple_models;           /* 0; != 0: TwoViewGeometry::EstimateMultiple (two_view_geometry.cc:128-167) */
  /* RANSACOptions */
  double max_error;        /* 4.0   */
  double min_inlier_ratio; /* 0.25  */
  double confidence;       /* 0.999 */
  uint64_t min_num_trials; /* 30    */
  uint64_t max_num_trials; /* 10000 */
  int32_t multiple_ignore_watermark; /* 1 (two_view_geometry.h:140); only read when multiple_models != 0 */
  int32_t reserved;
} dsm_two_view_options;

/* Camera as used by the verification path (src/base/camera.h; models
 * src/base/camera_models.h:187-349).  model_id and the parameter order follow the reference:
 *   0 SIMPLE_PINHOLE f,cx,cy            1 PINHOLE fx,fy,cx,cy              2 SIMPLE_RADIAL f,cx,cy,k
 *   3 RADIAL f,cx,cy,k1,k2              4 OPENCV fx,fy,cx,cy,k1,k2,p1,p2   5 OPENCV_FISHEYE fx,fy,cx,cy,k1..k4
 *   6 FULL_OPENCV fx,fy,cx,cy,k1,k2,p1,p2,k3..k6   7 FOV fx,fy,cx,cy,omega
 *   8 SIMPLE_RADIAL_FISHEYE f,cx,cy,k   9 RADIAL_FISHEYE f,cx,cy,k1,k2
 *  10 THIN_PRISM_FISHEYE fx,fy,cx,cy,k1,k2,p1,p2,k3,k4,sx1,sy1
 * Any other model_id is rejected with DSM_ERR_INVALID_ARGUMENT (the reference CHECKs ExistsCameraModelWithId,
 * camera.cc:52).  Models 5, 7, 8, 9, 10 evaluate atan/tan/sin/cos with the device's math library. */
typedef struct dsm_camera {
  int32_t model_id;
  int32_t has_prior_focal_length; /* Camera::HasPriorFocalLength, camera.h:191 */
  uint64_t width;
  uint64_t height;
  double params[12];
} dsm_camera;

/* TwoViewGeometry::ConfigurationType, src/estimators/two_view_geometry.h:83-102 */
enum {
  DSM_CONFIG_UNDEFINED = 0,
  DSM_CONFIG_DEGENERATE = 1,
  DSM_CONFIG_CALIBRATED = 2,
  DSM_CONFIG_UNCALIBRATED = 3,
  DSM_CONFIG_PLANAR = 4,
  DSM_CONFIG_PANORAMIC = 5,
  DSM_CONFIG_PLANAR_OR_PANORAMIC = 6,
  DSM_CONFIG_WATERMARK = 7,
  DSM_CONFIG_MULTIPLE = 8
};

/* Fixed-size part of a TwoViewGeometry (two_view_geometry.h:286-303).  Matrices
 * are row-major 3x3.  The variable-length inlier_matches are fetched separately. */
typedef struct dsm_two_view_geometry {
  int32_t config;
  uint32_t num_inliers;  /* == inlier_matches.size() */
  uint32_t num_matches;  /* putative matches that went into Estimate */
  uint32_t reserved;
  double F[9];
  double E[9];
  double H[9];
  double qvec[4];
  double tvec[3];
  double tri_angle;
  /* bookkeeping for the hypotheses/s metric: LO-RANSAC trials and
   * models scored (minimal-sample models + local-optimisation models). */
  uint32_t num_trials[4];  /* E, F, H, watermark-translation */
  uint32_t num_models[4];
} dsm_two_view_geometry;

/* ------------------------------------------------------------------ context */
typedef struct dsm_ctx dsm_ctx;

/* Number of HIP devices visible to this process (0 when there is none).  SiftMatchingOptions::gpu_index "-1" means
 * "all of them", one matcher per device (src/feature/matching.cc:631-645, doc/faq.rst:322-331). */
int dsm_device_count(void);

/* Creates a context bound to HIP device `device`.  Replaces SiftFeatureMatcher's
 * ctor + Setup() (src/feature/matching.cc:610-675, 713-747): returns
 * DSM_ERR_NO_DEVICE where Setup() would return false. */
int dsm_ctx_create(int device, dsm_ctx** out_ctx);
void dsm_ctx_destroy(dsm_ctx* ctx);
/* The HIP device the context is bound to (-1 for NULL): what a companion library needs to place its own buffers and
 * communicators next to the context (include/dagsfm_gather.h). */
int dsm_ctx_device(const dsm_ctx* ctx);
/* Number of pairs of the context's last dsm_match_pairs / dsm_set_matches (0 before any). */
uint32_t dsm_ctx_num_pairs(const dsm_ctx* ctx);
/* Last error text for this context (or for ctx creation when ctx == NULL). */
const char* dsm_last_error(const dsm_ctx* ctx);
/* Blocks until all work queued by this context has finished. */
int dsm_sync(dsm_ctx* ctx);
/* Scheduling / cross-check switches of one context, for tests and profiling: `key` is one of the names DESIGN.md lists
 * under "Tuning / debugging hooks" (e.g. "DSM_VERIFY_LANES"), `value` its setting; value == NULL removes the key.  None
 * of them changes a result (tools/check_schedules.py).  The library never reads the process environment, so a host
 * application's environment cannot change schedules; the reference has no analogue (its options all travel in
 * SiftMatchingOptions, src/feature/sift.h:139-195).  DSM_ERR_INVALID_ARGUMENT for an unknown key. */
int dsm_set_debug_option(dsm_ctx* ctx, const char* key, const char* value);

/* A memory budget at the boundary.  The reference documents its GPU matcher's footprint and leaves the rest of the device to the
 * host application (doc/faq.rst:353-356: "4 n^2 + 4 n 256 bytes"; the mapper's dense stages run on the same GPU next).  This
 * library's stages cut their pair list into chunks sized by the memory they may use for TRANSIENT scratch -- the matcher's
 * per-row outputs of K1 (default: 8 GiB per chunk), the verifier's speculated trials of a chunk of pairs (default: 40 % of what
 * is free at the call, at least 4 GiB, at most 96 GiB) -- and `bytes` > 0 replaces both defaults: the two stages together then
 * hold at most `bytes` of chunk scratch (a quarter of it, at most 8 GiB, for the matcher; the rest for the verifier's lanes; both
 * keep their scratch between calls).  Smaller chunks cost time, never results
 * (tests/test_memory_budget_gpu.py; profiles/r06_memory_budget.txt has the step time of config 2 at 8 / 16 / 38 GiB).  The
 * RESIDENT set -- descriptors, keypoints, matches, per-pair state and results of the current list -- follows from the inputs and
 * is not chunked; dsm_ctx_memory_footprint reports both.  Scratch already held beyond a new, smaller budget is released at once.
 * bytes == 0 restores the defaults.  A budget too small for one pair's scratch still runs (a chunk is never shorter than one pair). */
int dsm_ctx_set_memory_budget(dsm_ctx* ctx, uint64_t bytes);
/* Device memory the context holds right now: *resident_bytes = images + the last calls' inputs / results / per-pair state,
 * *scratch_bytes = the chunk scratch the budget governs.  Either pointer may be NULL. */
int dsm_ctx_memory_footprint(const dsm_ctx* ctx, uint64_t* resident_bytes, uint64_t* scratch_bytes);

/* What the device reports about itself (hipDeviceProp_t): used by bench.py to derive the roofline peaks from
 * the hardware instead of hard-coding them. */
typedef struct dsm_device_info {
  char name[128];
  char arch[64];            /* gcnArchName, e.g. "gfx950:sramecc+:xnack-" */
  int32_t compute_units;    /* multiProcessorCount */
  int32_t clock_khz;        /* clockRate: peak engine clock */
  int32_t memory_clock_khz; /* memoryClockRate */
  int32_t memory_bus_bits;  /* memoryBusWidth */
  uint64_t total_memory;    /* totalGlobalMem, bytes */
  int32_t l2_bytes;         /* l2CacheSize (one XCD's L2) */
  int32_t lds_per_cu;       /* maxSharedMemoryPerMultiProcessor */
} dsm_device_info;
int dsm_get_device_info(dsm_ctx* ctx, dsm_device_info* out);

/* Makes `n_images` images resident in HBM.  Replaces FeatureMatcherCache::Setup /
 * GetDescriptors / GetKeypoints (src/feature/matching.cc:221-316) and
 * SiftMatchGPU::SetDescriptors (lib/SiftGPU/SiftGPU.h:303-336).
 *   n_feats[i]      number of features of image i (may be 0)
 *   desc[i]         n_feats[i] x 128 uint8, row-major (FeatureDescriptors, types.h:102)
 *   kp_xy[i]        n_feats[i] x 2 float (x,y) with stride kp_stride floats between
 *                   keypoints (6 for FeatureKeypoint, types.h:44-81); may be NULL when
 *                   only matching is wanted
 *   cameras[i]      camera of image i; may be NULL when only matching is wanted
 * Pointers are host pointers, borrowed for the duration of the call.  Pageable memory (the reference's Eigen
 * matrices and std::vectors) is read by a few host threads of the library's own into pinned staging slots
 * (32 MB per context, allocated by the first such call); memory that is pinned already is copied where it lies. */
int dsm_set_images(dsm_ctx* ctx, uint32_t n_images, const uint32_t* n_feats,
                   const uint8_t* const* desc, const float* const* kp_xy,
                   uint32_t kp_stride, const dsm_camera* cameras);

/* Adds `n_images` images to the resident set without touching the ones already there: the new images
 * get the indices n_resident .. n_resident + n_images - 1 and only their rows are uploaded.  This is
 * FeatureMatcherCache's incremental behaviour (an LRU that loads what a block of the pair list adds,
 * src/feature/matching.cc:245-316) for the device-side copy: ExhaustiveFeatureMatcher visits the
 * database in blocks (matching.cc:870-905) and consecutive blocks share half of their images.
 * Arguments as dsm_set_images; keypoints / cameras must be given iff the resident images have them.
 * Invalidates the results of earlier dsm_match_pairs / dsm_verify_pairs calls, like dsm_set_images. */
int dsm_append_images(dsm_ctx* ctx, uint32_t n_images, const uint32_t* n_feats,
                      const uint8_t* const* desc, const float* const* kp_xy,
                      uint32_t kp_stride, const dsm_camera* cameras);

/* Brute-force matches every listed image pair on the device.  Replaces the
 * matcher stage of SiftFeatureMatcher::Match (src/feature/matching.cc:749-839)
 * = MatchSiftFeaturesCPU per pair (src/feature/sift.cc:810-822).
 *   pairs   n_pairs x 2 image indices (into the dsm_set_images order)
 * Results stay in HBM until fetched or consumed by dsm_verify_pairs. */
int dsm_match_pairs(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs,
                    const dsm_match_options* options);

/* Installs caller-provided matches (host pointers) as if dsm_match_pairs had produced them, so
 * that dsm_verify_pairs can verify them.  Used for SiftFeatureMatcher::Match's resume path: a
 * pair whose `matches` row exists but whose `two_view_geometries` row does not is only
 * re-verified (src/feature/matching.cc:782-812).  offsets has n_pairs+1 entries. */
int dsm_set_matches(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const uint64_t* offsets,
                    const uint32_t* matches);

/* Per-pair number of matches of the last dsm_match_pairs; `counts` has n_pairs
 * entries (host or device pointer). */
int dsm_get_match_counts(dsm_ctx* ctx, uint32_t* counts);
/* All matches of the last dsm_match_pairs, pair after pair in list order:
 * `offsets` gets n_pairs+1 prefix offsets (in matches), `matches` gets
 * offsets[n_pairs] x 2 uint32 (point2D_idx1, point2D_idx2) in ascending idx1
 * per pair (FeatureMatches, types.h:86-104).  Either pointer may be NULL.
 * `matches_capacity` is in matches (pairs of uint32). */
int dsm_get_matches(dsm_ctx* ctx, uint64_t* offsets, uint32_t* matches,
                    uint64_t matches_capacity);

/* One-shot leaf with the signature shape of MatchSiftFeaturesCPU
 * (src/feature/sift.h:214-217) / MatchSiftFeaturesGPU (sift.h:229-239):
 * host descriptors in, FeatureMatches out.  `matches` must hold
 * min(n1,n2) x 2 uint32 with cross_check, n1 x 2 uint32 without. */
int dsm_match_sift_features(dsm_ctx* ctx, const dsm_match_options* options,
                            const uint8_t* desc1, uint32_t n1,
                            const uint8_t* desc2, uint32_t n2,
                            uint32_t* matches, uint32_t* n_matches);

/* Device timing of the dominant kernel (descriptor distance + fused top-2) of the
 * last dsm_match_pairs, measured with HIP events on the stream the kernel was
 * launched on: total milliseconds and number of launches. */
int dsm_get_match_kernel_time(dsm_ctx* ctx, double* total_ms, uint32_t* n_launches);
/* Same for the interval behind pass 1 in which the follow-up kernel k1_resolve_index ran (best tile of every accepted row
 * -> exact column index).  The dominant kernel resolves those rows in its own tail now: the interval is empty (about 0);
 * only the check build's two-kernel form (DSM_K1_RESOLVE_KERNEL) fills it. */
int dsm_get_match_resolve_time(dsm_ctx* ctx, double* total_ms);
/* Same for the gathered second pass of the cross-check (k1_best_rows over the rows matches12 points at). */
int dsm_get_match_gather_time(dsm_ctx* ctx, double* total_ms);
/* Same for everything else on the stream: the entry list of pass 2 (k2 + scan between pass 1 and pass 2) and the compaction
 * of the mutual matches (k2_entries + scan, the host's waits for the totals included) --
 * without the cross-check: the compaction of the one-way matches -- so that the four match timers sum to the call in both modes. */
int dsm_get_match_tail_time(dsm_ctx* ctx, double* total_ms);

/* ------------------------------------------------------------------ verification */

/* Per-pair PRNG seed used when dsm_verify_pairs gets no explicit seeds: a 32-bit mix of
 * Database::ImagePairToPairId(id1, id2) (src/base/database.h:336-347) xor user_seed.  The
 * reference seeds each verifier thread from the wall clock (src/util/random.cc:40-56) and is
 * not reproducible; one MT19937 stream per pair, consumed E -> F -> H -> watermark in the order of
 * src/estimators/two_view_geometry.cc:325-342, 547-549, is the defined schedule here. */
uint32_t dsm_pair_seed(uint32_t image_id1, uint32_t image_id2, uint32_t user_seed);

/* Geometric verification of every pair of the last dsm_match_pairs on the device.  Replaces
 * the TwoViewGeometryVerifier stage of SiftFeatureMatcher::Match (src/feature/matching.cc:
 * 550-608, 749-839) = TwoViewGeometry::Estimate per pair (two_view_geometry.cc:113-126).
 *   seeds         n_pairs explicit PRNG seeds, or NULL to use dsm_pair_seed(idx1, idx2, user_seed)
 *   stage_filter  non-zero: pairs with fewer than min_num_inliers inliers get a default
 *                 TwoViewGeometry(), as Match() writes them (matching.cc:824-831)
 * options->multiple_models != 0 runs TwoViewGeometry::EstimateMultiple (two_view_geometry.cc:128-167)
 * instead, as the verifier does (matching.cc:596-599): repeated Estimate passes over the matches that are
 * not inliers yet, on ONE generator stream per pair; several geometries -> config MULTIPLE with the inlier
 * matches of all of them (other fields as in a fresh TwoViewGeometry()); num_trials / num_models are summed
 * over the passes. */
int dsm_verify_pairs(dsm_ctx* ctx, const dsm_two_view_options* options, const uint32_t* seeds,
                     uint32_t user_seed, int32_t stage_filter);
/* Results of the last dsm_verify_pairs: n_pairs fixed-size records ... */
/* Guided matching (SiftMatchingOptions::guided_matching, src/feature/sift.h:162) over the pairs of the last
 * dsm_verify_pairs: every pair with at least min_num_inliers inlier matches (matching.cc:449-453) and an F-type
 * (CALIBRATED, UNCALIBRATED) or H-type (PLANAR, PANORAMIC, PLANAR_OR_PANORAMIC) configuration is matched again
 * with the descriptor distance of keypoint pairs that violate F / H (float Sampson / transfer error above
 * max_error^2) set to zero, and the result REPLACES its inlier matches -- MatchGuidedSiftFeaturesCPU
 * (src/feature/sift.cc:824-875), GuidedSiftCPUFeatureMatcher::Run (matching.cc:441-470); config, E, F, H and
 * the pose stay.  Call dsm_verify_pairs with stage_filter = 0 first; stage_filter here is Match()'s
 * post-filter (matching.cc:824-831) on the final inlier counts. */
int dsm_guided_match_pairs(dsm_ctx* ctx, const dsm_match_options* match_options,
                           const dsm_two_view_options* options, int32_t stage_filter);

int dsm_get_two_view_geometries(dsm_ctx* ctx, dsm_two_view_geometry* out);
/* ... and the inlier_matches of all pairs in list order (same conventions as dsm_get_matches). */
int dsm_get_inlier_matches(dsm_ctx* ctx, uint64_t* offsets, uint32_t* inlier_matches,
                           uint64_t capacity);
/* Device time (HIP events on the launch stream) of the verification kernel of the last call. */
int dsm_get_verify_kernel_time(dsm_ctx* ctx, double* total_ms);

/* One-shot leaf with the signature shape of TwoViewGeometry::Estimate
 * (src/estimators/two_view_geometry.h:180-184): host cameras, points (n x 2 doubles, as
 * FeatureKeypointsToPointsVector makes them) and matches in, TwoViewGeometry out.
 * `inlier_matches` must hold n_matches x 2 uint32 (may be NULL). */
int dsm_estimate_two_view_geometry(dsm_ctx* ctx, const dsm_camera* camera1, const double* points1,
                                   uint32_t n1, const dsm_camera* camera2, const double* points2,
                                   uint32_t n2, const uint32_t* matches, uint32_t n_matches,
                                   const dsm_two_view_options* options, uint32_t seed,
                                   dsm_two_view_geometry* out, uint32_t* inlier_matches);

/* Test hook: the first n_draws samples (k indices each) the device sampler draws from
 * `total` items with the given seed (RandomSampler, src/optim/random_sampler.cc:43-62). */
int dsm_debug_sample_sequence(dsm_ctx* ctx, uint32_t seed, uint32_t k, uint32_t total,
                              uint32_t n_draws, uint32_t* out);

/* Test hook: the statistics counters of the last dsm_verify_pairs call that ran with the debug option DSM_VERIFY_DEBUG or
 * DSM_SCORE_PREFILTER=check (16 uint32, summed over the lanes): [1..6] candidates / local optimisations per family, [14]
 * (model, pair) slots whose exact inlier count fell outside the bounds of the scoring's bound step -- must be 0 --, [15] slots
 * the bound step would have skipped. */
int dsm_debug_verify_counters(dsm_ctx* ctx, uint32_t* out16);

/* Test hook: how often the minimal solvers of the last dsm_verify_pairs call that ran with DSM_VERIFY_DEBUG fell back from the
 * certified pivot norms to the exact bookkeeping (6 uint32, summed over the lanes, counted per wave of 64 solves): [0..2] waves
 * of the E / F / H solver that ran the exact form, [3..5] all waves of that solver.  All zero on the product library, whose
 * kernels do not count. */
int dsm_debug_solver_fallbacks(dsm_ctx* ctx, uint32_t* out6);

/* Test hook: Camera::ImageToWorld (src/base/camera.cc:210-214) of n pixel points (x, y) on the device. */
int dsm_debug_image_to_world(dsm_ctx* ctx, const dsm_camera* camera, uint32_t n, const double* xy, double* out_uv);

/* ------------------------------------------------------------------ vocabulary-tree retrieval (candidate pairs)
 * The step BEFORE matching: VocabSimilarityGraph::Run (src/graph/similarity_graph.cpp:101-199)
 * indexes every image in a retrieval::VisualIndex (src/retrieval/visual_index.h) and queries every image against it;
 * an image and each image retrieved for it become a candidate pair.  Works on the images of dsm_set_images
 * (descriptors only).  Deviations from the reference, all in DESIGN.md: the nearest visual words are EXACT (the
 * reference asks FLANN for approximate ones), float sums run left to right, ties keep first-seen order. */
typedef struct dsm_vocabulary {
  uint32_t num_words;      /* visual words (leaves of the vocabulary tree), VisualIndex::NumVisualWords */
  uint32_t reserved;
  const uint8_t* words;    /* [num_words][128] uint8 centroids, visual_words_ (visual_index.h:176-178) */
  const float* projection; /* [64][128] row-major Hamming-embedding projection, InvertedIndex::proj_matrix_ */
  const float* thresholds; /* [num_words][64] per-word embedding thresholds, InvertedFile::thresholds_ */
} dsm_vocabulary;
int dsm_retrieval_set_vocabulary(dsm_ctx* ctx, const dsm_vocabulary* vocabulary);
/* The reference's OWN word ids instead of the device's exact nearest words: VisualIndex::FindWordIds (visual_index.h:
 * 695-738) asks the flann::AutotunedIndex loaded from the vocabulary file for APPROXIMATE neighbours, once with 1
 * neighbour when a feature is indexed (VisualIndex::Add, :201-243) and once with QueryOptions::num_neighbors when it is
 * queried (:664-693).  The host shim restates that search (dagsfm_amd/host/flann_index.cc, bit for bit against the
 * reference's FLANN) and hands the ids over here: index_ids [features] and query_ids [features][k_query] for the
 * features of all resident images back to back, kInvalidWordId (INT_MAX) where FLANN returned fewer.  Later
 * dsm_retrieval_index / _query / _matches use them (num_neighbors must equal k_query); both NULL: exact search again. */
int dsm_retrieval_set_word_ids(dsm_ctx* ctx, const int32_t* index_ids, uint32_t k_query, const int32_t* query_ids);
/* The reference's word search ON THE DEVICE (round 5): the FLANN index the vocabulary file carries -- what
 * flann::AutotunedIndex::loadIndex reads (visual_index.h:564-574) -- as flat arrays, searched by a lane per feature with
 * FLANN's own visit order, branch heap and result set (csrc/flann_search.hip <- lib/FLANN/algorithms/kdtree_index.h:
 * 543-617, kmeans_index.h:717-833, linear_index.h:130-146; ids and float distances equal the reference's knnSearch bit
 * for bit).  The host shim parses the file (dagsfm_amd/host/flann_index.cc) and hands the trees over here; afterwards
 * dsm_retrieval_index searches with 1 neighbour and dsm_retrieval_query / _matches with num_neighbors, both with
 * `num_checks` (IndexOptions / QueryOptions::num_checks).  Every node, child and point index is validated on upload
 * (DSM_ERR_OUT_OF_RANGE).  NULL: the device's exact search again.  Word ids set with dsm_retrieval_set_word_ids win. */
typedef struct dsm_flann_kd_node {
  int32_t divfeat;        /* inner node: split dimension (0..127); leaf: the word's index */
  float divval;
  int32_t child1, child2; /* node indices, greater than the node's own; -1 / -1 marks a leaf */
} dsm_flann_kd_node;
typedef struct dsm_flann_km_node {
  uint64_t pivot;         /* offset of the node's centre in `pivots`, in floats (a multiple of 128) */
  float radius, variance;
  int32_t size;           /* leaf: number of points */
  uint32_t first_child;   /* inner node: `branching` entries of km_childs from here */
  uint32_t num_childs;    /* 0 for a leaf, else == branching */
  uint32_t reserved;
  uint64_t first_point;   /* leaf: `size` entries of km_points from here */
} dsm_flann_km_node;
typedef struct dsm_flann_index {
  int32_t algorithm;      /* flann_algorithm_t: 0 linear, 1 randomised kd-trees, 2 hierarchical k-means */
  int32_t num_checks;     /* SearchParams::checks, >= 0 on a tree index */
  uint32_t num_words;     /* must equal the vocabulary's */
  int32_t branching;      /* k-means */
  float cb_index;         /* k-means */
  int32_t km_root;        /* k-means: index of the root node */
  uint32_t n_kd_nodes, n_kd_roots;
  const dsm_flann_kd_node* kd_nodes;
  const int32_t* kd_roots;
  uint32_t n_km_nodes, reserved;
  const dsm_flann_km_node* km_nodes;
  uint64_t n_km_childs;
  const int32_t* km_childs;
  uint64_t n_km_points;
  const uint64_t* km_points;
  uint64_t n_pivot_floats;
  const float* pivots;
} dsm_flann_index;
int dsm_retrieval_set_flann_index(dsm_ctx* ctx, const dsm_flann_index* index);
/* The same search for caller-supplied descriptors (n x 128 uint8, host memory): ids [n][k] (INT_MAX where FLANN returned
 * fewer) and, if not NULL, FLANN's squared L2 distances [n][k]; 1 <= k <= 8.  What the parity tests and
 * tools/bench_retrieval.py call; *ms (may be NULL) receives the kernel's device time. */
int dsm_retrieval_flann_search(dsm_ctx* ctx, const uint8_t* descriptors, uint32_t n, uint32_t k, int32_t* ids, float* dists,
                               double* ms);
/* VisualIndex::Add (IndexOptions::num_neighbors = 1) for every resident image in list order, then Prepare()
 * (visual_index.h:201-243, 501-505): inverted files sorted by image, IDF weights, normalisation constants. */
int dsm_retrieval_index(dsm_ctx* ctx);
/* VisualIndex::Query (num_images_after_verification = 0, visual_index.h:664-693) for every resident image:
 * counts[q] image scores (<= max_num_images) for query image q, image_idx / scores at [q * max_num_images + k] in
 * retrieval order (descending score).  The query image itself is among its results, as in the reference.
 * num_neighbors: QueryOptions::num_neighbors (VocabSimilaritySearchOptions::num_nearest_neighbors, default 5, max 8). */
int dsm_retrieval_query(dsm_ctx* ctx, uint32_t num_neighbors, uint32_t max_num_images, uint32_t* counts,
                        uint32_t* image_idx, float* scores);
/* The input of the spatial re-ranking (VisualIndex::Query with geometries, visual_index.h:295-346; QueryOptions::
 * num_images_after_verification > 0): for every resident image as the query and its retrieved images (counts / image_idx as
 * dsm_retrieval_query returned them, same max_num_images), the database features that fall into one of the query feature's
 * words, belong to a retrieved image and lie within HammingDistWeightFunctor::kMaxHammingDistance (InvertedIndex::
 * FindMatches + the Hamming test).  offsets[q] .. offsets[q + 1] (n_images + 1 entries) index the tuples of query q;
 * dsm_get_retrieval_matches copies them: 5 uint32 each = query feature, image, database feature, (word << 8) | Hamming
 * distance, position of the entry in the inverted files (the order the reference's pointer comparison has inside one
 * file), in (query feature, neighbour, entry) order.  The 1-to-1 assignment and VoteAndVerify (vote_and_verify.cc) run on
 * the host (dagsfm_amd/host/spatial_verification.cc): they are sequential per image and use the host's float libm. */
int dsm_retrieval_matches(dsm_ctx* ctx, uint32_t num_neighbors, uint32_t max_num_images, const uint32_t* counts,
                          const uint32_t* image_idx, uint64_t* offsets);
int dsm_get_retrieval_matches(dsm_ctx* ctx, uint32_t* tuples, uint64_t capacity);
/* InvertedFile::IDFWeight of every visual word (inverted_file.h:260-271) after dsm_retrieval_index. */
int dsm_get_retrieval_idf(dsm_ctx* ctx, float* idf, uint32_t capacity);
/* Test hook: the k nearest visual words (ascending distance, ties to the lower id) of every feature of one image. */
int dsm_retrieval_debug_word_ids(dsm_ctx* ctx, uint32_t image, uint32_t k, int32_t* out);
/* Device time (HIP events) of the last dsm_retrieval_index / dsm_retrieval_query. */
int dsm_get_retrieval_time(dsm_ctx* ctx, double* index_ms, double* query_ms);

/* ------------------------------------------------------------------ view-graph ingest + rotation-cycle filter
 * The step AFTER the stage: DistributedMapperController::LoadTwoviewGeometries
 * (src/controllers/distributed_mapper_controller.cpp:585-631) turns every two_view_geometries row into a view-graph
 * edge (rotation = the row's qvec), ViewGraph::FilterViewGraphCyclesByRotation(5.0) (src/graph/view_graph.cpp:115-165)
 * keeps an edge iff it lies on a cycle of length 3 whose loop rotation R23 * R12 * R13^T is below the threshold.
 *   pairs  n_pairs x 2 image ids (any ids; a repeat of an earlier pair is ignored: keep = 0)
 *   qvecs  n_pairs x 4 (w, x, y, z): the relative rotation of the pair as stored, i.e. for image_id1 < image_id2
 *   keep   n_pairs flags out;  n_triplets (optional): cycles of length 3 found
 * Host pointers. */
int dsm_view_graph_filter_cycles(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs,
                                 double max_loop_error_degrees, uint8_t* keep, uint64_t* n_triplets);

/* ------------------------------------------------------------------ global rotation averaging
 * The step after the rotation-cycle filter: DistributedMapperController::GlobalRotationAveraging
 * (src/controllers/distributed_mapper_controller.cpp:945-1008) with its defaults (reconstruct_largest_cc, ROBUST_L1L2):
 *   1. the largest connected component of the used edges (ImageGraph::ExtractLargestCC, src/graph/image_graph.cpp:8-50;
 *      edges outside it are dropped, :953-967).  Ties between equal-size components: the one holding the smallest image
 *      id wins (the reference takes unordered_map order -- a free choice here);
 *   2. RobustRotationEstimator (src/rotation_estimation/robust_rotation_estimator.cpp:84-318): every orientation starts
 *      at zero, the smallest image id is held constant, L1 regression by ADMM (src/solver/l1_solver.h) then IRLS;
 *   3. FilterViewPairsFromOrientation (src/sfm/filter_view_pairs_from_orientation.cpp:22-90): an edge whose loop
 *      rotation -R12 * (R2 * -R1) is above the threshold is removed, a kept edge gets RelativeRotationFromTwoRotations
 *      (src/math/util.h:97-106);
 *   4. the largest connected component of the surviving edges.
 * The reference factorises every system with CHOLMOD; here every system is the grounded weighted graph Laplacian
 * (A^T W A = L_w (x) I3) solved by a Jacobi-preconditioned conjugate gradient on the device: the results agree with the
 * reference's mathematics by tolerance, not bit for bit.  A solve that ends above a relative residual of
 * 1e-9 fails the call with DSM_ERR_NOT_CONVERGED. */
#define DSM_RA_MAX_L1_ITERATIONS 8
typedef struct dsm_rotation_averaging_options {
  int32_t max_num_l1_iterations;         /* 5 (robust_rotation_estimator.h:101); at most DSM_RA_MAX_L1_ITERATIONS */
  int32_t max_num_irls_iterations;       /* 100 (:107) */
  double l1_step_convergence_threshold;  /* 0.001 (:104); the L1 loop stops on avg_step <= threshold */
  double irls_step_convergence_threshold;/* 0.001 (:110); the IRLS loop stops on avg_step < threshold */
  double irls_loss_parameter_sigma;      /* DegToRad(5.0) (:114) */
  int32_t admm_initial_max_iterations;   /* 5: L1Solver options.max_num_iterations, doubled per L1 iteration (:201-222) */
  int32_t max_num_cg_iterations;         /* 0: max(1000, 20 * images of the component) per solve */
  int32_t cg_batch_iterations;           /* 0: 16.  CG iterations the host enqueues between two reads of the device's
                                            convergence flags; changes the number of no-op launches, never a result */
  int32_t reserved;
  double admm_rho;                       /* 1.0 (l1_solver.h Options) */
  double admm_alpha;                     /* 1.0 */
  double admm_absolute_tolerance;        /* 1e-4 */
  double admm_relative_tolerance;        /* 1e-2 */
  double max_relative_rotation_difference_degrees; /* 5.0 (DistributedMapperController options) */
  double cg_tolerance;                   /* 1e-12: relative residual at which a solve stops */
  double cg_max_residual;                /* 1e-9: a solve that ends above it is DSM_ERR_NOT_CONVERGED */
} dsm_rotation_averaging_options;

typedef struct dsm_rotation_averaging_report {
  uint32_t num_components;          /* connected components of the used edges */
  uint32_t num_images;              /* images of the largest one (the estimated orientations) */
  uint32_t num_edges;               /* edges of the largest one */
  uint32_t num_l1_iterations;       /* outer L1 iterations run */
  uint32_t admm_iterations[DSM_RA_MAX_L1_ITERATIONS]; /* ADMM iterations of each outer L1 iteration */
  uint32_t num_irls_iterations;
  uint32_t num_filtered_edges;      /* edges removed by the orientation filter */
  uint32_t num_final_images;        /* images of the largest component after the filter */
  uint32_t reserved;
  uint64_t total_cg_iterations;
  double max_cg_relative_residual;  /* largest final relative residual over all solves */
  double last_l1_step;              /* average step of the last L1 iteration */
  double last_irls_step;            /* average step of the last IRLS iteration */
  double device_ms;                 /* HIP events: first upload to the last kernel */
} dsm_rotation_averaging_report;

void dsm_default_rotation_averaging_options(dsm_rotation_averaging_options* o);

/* GlobalRotationAveraging() over an edge list (the arrays of dsm_view_graph_filter_cycles).
 *   pairs    n_pairs x 2 image ids (image_id1, image_id2); qvecs n_pairs x 4 (w, x, y, z): the rotation from image 1 to
 *            image 2, QuaternionToAngleAxis(qvec) as LoadTwoviewGeometries reads it (distributed_mapper_controller.cpp:617-619)
 *   use      n_pairs flags (the `keep` output of dsm_view_graph_filter_cycles) or NULL = every edge.  A repeat of an earlier
 *            used pair, in either order, is ignored (ViewGraph::AddTwoViewGeometry).  id1 == id2, a non-finite or a zero
 *            qvec on a used edge: DSM_ERR_INVALID_ARGUMENT
 *   options  NULL = dsm_default_rotation_averaging_options
 * Per image of the first component, sorted by id (capacity 2 * n_pairs each):
 *   image_ids_out, orientations_out (x 3, angle-axis), image_in_final_cc (0 / 1); *n_images_out = their number.
 * Per input edge: edge_state 0 unused / masked / repeat, 1 outside the first component, 2 removed by the orientation filter,
 *   3 kept -- relative_rotations_out (n_pairs x 3, angle-axis) then holds RelativeRotationFromTwoRotations(R1, R2) (else 0).
 * report (may be NULL).  Host pointers.  No used edge: DSM_OK with *n_images_out = 0. */
int dsm_view_graph_rotation_averaging(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs,
                                      const uint8_t* use, const dsm_rotation_averaging_options* options,
                                      uint32_t* image_ids_out, double* orientations_out, uint8_t* image_in_final_cc,
                                      uint32_t* n_images_out, uint8_t* edge_state, double* relative_rotations_out,
                                      dsm_rotation_averaging_report* report);

/* ------------------------------------------------------------------ global rotation averaging, NONLINEAR
 * GlobalRotationAveraging() with global_rotation_estimator_type = NONLINEAR
 * (src/controllers/distributed_mapper_controller.cpp:969-986): steps 1, 3 and 4 above, and as step 2
 * NonlinearRotationEstimator::EstimateRotations (src/rotation_estimation/nonlinear_rotation_estimator.cpp:82-131): one
 * PairwiseRotationError (src/rotation_estimation/pairwise_rotation_error.h:98-128; weight 1) per edge under one
 * ceres::SoftLOneLoss(robust_loss_width), no constant block, ceres' Levenberg-Marquardt with max_num_iterations = 200 and
 * otherwise ceres' defaults.  The trust-region rules are dsm_bundle_adjust's without the Schur part; the
 * reference's sparse Cholesky of J^T J + D / radius is a conjugate gradient preconditioned by the exact 3 x 3 diagonal
 * blocks here.  The cost is invariant under one rotation applied to every image and nothing holds that
 * gauge: compare orientations relative to one image, or as edge rotations, never absolutely. */
typedef struct dsm_nonlinear_rotation_options {
  double robust_loss_width;              /* 0.1 (nonlinear_rotation_estimator.h:86); > 0 */
  int32_t max_num_iterations;            /* 200 (nonlinear_rotation_estimator.cpp:125) */
  int32_t max_num_consecutive_invalid_steps; /* 5 (ceres) */
  double function_tolerance;             /* 1e-6 (ceres) */
  double gradient_tolerance;             /* 1e-10 (ceres) */
  double parameter_tolerance;            /* 1e-8 (ceres) */
  double initial_trust_region_radius;    /* 1e4 (ceres) */
  double max_trust_region_radius;        /* 1e16 (ceres) */
  double min_relative_decrease;          /* 1e-3 (ceres) */
  double min_lm_diagonal;                /* 1e-6 (ceres) */
  double max_lm_diagonal;                /* 1e32 (ceres) */
  int32_t max_num_cg_iterations;         /* 0: max(1000, 20 * images of the component) per solve */
  int32_t reserved;
  double cg_tolerance;                   /* 1e-14: relative residual at which a solve stops.  Tighter than the robust stage's
                                            1e-12: the reference factorises exactly, and a step solved to 1e-12 moves the cost
                                            of the iterations in mid-descent by up to 1e-7 relative */
  double cg_max_residual;                /* 1e-9: a solve that ends above it is DSM_ERR_NOT_CONVERGED */
  double max_relative_rotation_difference_degrees; /* 5.0 (DistributedMapperController options) */
} dsm_nonlinear_rotation_options;

typedef struct dsm_nonlinear_rotation_report {
  uint32_t num_components;          /* connected components of the used edges */
  uint32_t num_images;              /* images of the largest one */
  uint32_t num_edges;               /* edges of the largest one (the residual blocks) */
  int32_t termination;              /* DSM_BA_CONVERGENCE / DSM_BA_NO_CONVERGENCE / DSM_BA_FAILURE: reported, never an
                                       error -- the reference does not look at ceres' summary either */
  uint32_t num_iterations;          /* LM iterations (every step counts) */
  uint32_t num_successful_steps;
  uint32_t num_rejected_steps;      /* valid steps that did not reduce the cost enough */
  uint32_t num_invalid_steps;
  uint32_t num_filtered_edges;      /* edges removed by the orientation filter */
  uint32_t num_final_images;        /* images of the largest component after the filter */
  uint64_t total_cg_iterations;
  uint64_t num_kernel_launches;     /* launches of the estimator, the no-ops past a stop flag included */
  double initial_cost, final_cost;  /* 1/2 sum rho(|r|^2) */
  double final_trust_region_radius;
  double max_cg_relative_residual;  /* largest final relative residual over all solves */
  double min_rho_margin;            /* |(cost - candidate) - min_relative_decrease * model_cost_change| / cost */
  double min_gradient_margin;       /* relative distance of the gradient max-norm from gradient_tolerance */
  double min_function_margin;       /* relative distance of |cost - candidate| from function_tolerance * cost */
  double device_ms;                 /* HIP events: first upload to the last kernel */
} dsm_nonlinear_rotation_report;

void dsm_default_nonlinear_rotation_options(dsm_nonlinear_rotation_options* o);

#define DSM_NLR_TRACE_COLUMNS 6  /* DSM_BA_TRACE_COLUMNS: cost, radius, rho, CG iterations, accepted, gradient max-norm */

/* The arrays of dsm_view_graph_rotation_averaging, in and out, and additionally:
 *   n_initial = 0: every orientation starts at zero, as Run() does (distributed_mapper_controller.cpp:949-952).  Otherwise
 *     initial_image_ids (n_initial ids, ascending) and initial_orientations (n_initial x 3, angle-axis) -- the image_ids_out /
 *     orientations_out of dsm_view_graph_rotation_averaging fit -- must hold every image of the first component; ids outside
 *     it are ignored.  A missing image, a non-finite value, unsorted or repeated ids: DSM_ERR_INVALID_ARGUMENT.
 *   options NULL = dsm_default_nonlinear_rotation_options; report may be NULL; trace NULL or (max_num_iterations + 1) x
 *     DSM_NLR_TRACE_COLUMNS doubles (rows past the last iteration untouched).
 * DSM_OK whatever the termination type, with the last accepted state; only a conjugate-gradient solve that ends above
 * cg_max_residual fails the call (DSM_ERR_NOT_CONVERGED). */
int dsm_view_graph_rotation_averaging_nonlinear(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const double* qvecs,
                                                const uint8_t* use, uint32_t n_initial, const uint32_t* initial_image_ids,
                                                const double* initial_orientations,
                                                const dsm_nonlinear_rotation_options* options, uint32_t* image_ids_out,
                                                double* orientations_out, uint8_t* image_in_final_cc, uint32_t* n_images_out,
                                                uint8_t* edge_state, double* relative_rotations_out,
                                                dsm_nonlinear_rotation_report* report, double* trace);

/* The per-edge device function of the call above on n arbitrary triples (a test hook, like dsm_debug_image_to_world):
 * rotation1, rotation2, relative_rotation n x 3 angle-axis; residuals n x 3 and jacobians n x 18 (3 x 3 row-major with
 * respect to rotation1, then rotation2) after the loss corrector; rho n x 3 = rho(s), rho'(s), rho''(s) at s = |r|^2 of the
 * uncorrected residual.  Host pointers. */
int dsm_debug_pairwise_rotation_error(dsm_ctx* ctx, uint32_t n, const double* rotation1, const double* rotation2,
                                      const double* relative_rotation, double loss_width, double* residuals, double* jacobians,
                                      double* rho);

/* ------------------------------------------------------------------ view-graph clustering
 * The step after global rotation averaging: DistributedMapperController::ClusteringScenes
 * (src/controllers/distributed_mapper_controller.cpp:633-657) = ImageClustering::Cut() + Expand()
 * (src/clustering/image_clustering.cpp:68-128, 159-199, 451-624), and Cut() alone as the distributed matching path uses it
 * (:395-407; ExpandAllEdges is not restated).
 *   Nodes: the images of the used edges sorted by id (Cluster::InitIGraph, src/clustering/cluster.cpp:53-83); the weight of an
 *   edge is its visibility_score, the inlier count (distributed_mapper_controller.cpp:620).  k = images / num_images_ub
 *   clusters; k <= 1 (also images < num_images_ub, where the reference aborts on CHECK_GE(num_clusters, 1)): every label 0.
 *   SPECTRAL (src/clustering/spectral_cluster.cpp:52-176) on the device: the k algebraically smallest eigenvectors of
 *   L = D - S, D the number of edges of an image (not the sum of weights: the reference's operator, kept as it is), then
 *   KMeans with k-means++ (src/clustering/kmeans.h:158-235; its random draws run on the host with std::mt19937_64).  The
 *   reference solves with Spectra (SymEigsSolver<SMALLEST_ALGE>, ncv = min(2k, N)); here a Chebyshev-filtered subspace
 *   iteration in FP64 with the same block size and stopping rule: parity is by tolerance on the subspace, and the labels are
 *   identical wherever the k-means decisions are not within rounding of a tie.
 *   NCUT (the reference's default, Graclus) stays on the host application: it passes its labels in labels_in.
 *   Expand: the cluster pairs run one after another in ascending (c1, c2) order (the reference races them on a thread pool),
 *   equal weights keep input order (the reference's order is unordered_map order): free choices, DESIGN.md 10. */
typedef struct dsm_clustering_options {
  uint32_t num_images_ub;         /* 100 (image_clustering.h:126); 0 -> DSM_ERR_INVALID_ARGUMENT */
  uint32_t image_overlap;         /* 50 (:129); <= 2 -> invalid (Options::Check, image_clustering.cpp:49-58) */
  float completeness_ratio;       /* 0.5 (:132); > 1 -> invalid */
  int32_t expand;                 /* 1: Cut() + Expand() as ClusteringScenes; 0: Cut() only (inter == intra) */
  uint32_t max_kmeans_iterations; /* 0: unbounded, as KMeans' default */
  int32_t max_eigen_iterations;   /* 0: solver default (1000, Spectra's maxit); < 0 invalid */
  double eigen_tolerance;         /* 1e-10, Spectra's stopping rule (lib/Spectra/SymEigsSolver.h:583):
                                     ||L v - l v|| <= tol * max(eps^(2/3), |l|) for each of the k vectors */
} dsm_clustering_options;

typedef struct dsm_clustering_report {
  uint32_t num_images;              /* images of the used edges */
  uint32_t num_edges;               /* used edges after repeats */
  uint32_t num_clusters;            /* intra (= inter) clusters */
  uint32_t num_lost_edges;          /* edges between two intra clusters */
  uint32_t num_readded_edges;       /* lost edges Expand added back to one cluster */
  uint32_t eigen_iterations;        /* filter + Rayleigh-Ritz iterations (0: no device work) */
  uint32_t kmeans_iterations;       /* Lloyd iterations, the last one without a change included */
  uint32_t ncv;                     /* block size: min(2k, N) */
  uint64_t clustered_images_num;    /* AnalyzeStatistic (image_clustering.cpp:626-632): sum of inter cluster sizes */
  uint64_t clustered_edges_num;     /* sum of inter cluster edges */
  uint64_t operator_applications;   /* products L x (one per column of the block) */
  double max_eigen_residual;        /* max over the k vectors of ||L v - l v|| */
  double max_eigen_residual_ratio;  /* max of ||L v - l v|| / max(eps^(2/3), |l|): <= eigen_tolerance on success */
  double eigen_gap;                 /* l_(k+1) - l_k of the final Ritz values (0 when ncv == k) */
  double device_ms;                 /* HIP events: first upload to the last k-means kernel */
} dsm_clustering_report;

void dsm_default_clustering_options(dsm_clustering_options* o);

/* ClusteringScenes() over an edge list (the arrays of dsm_view_graph_rotation_averaging).
 *   pairs    n_pairs x 2 image ids; weights n_pairs inlier counts (a negative weight on a used edge: invalid)
 *   use      n_pairs flags or NULL = every edge; for the chained call: edge_state == 3 with both images in_final_cc.  A repeat
 *            of an earlier used pair, in either order, is ignored; id1 == id2 on a used edge: DSM_ERR_INVALID_ARGUMENT
 *   labels_in  NULL: SPECTRAL on the device.  Otherwise one label per image of the used edges in ascending id order (each
 *            < the number of those images; e.g. Graclus' NCUT labels): Cut()'s bookkeeping and Expand() run on them, no
 *            device work; the cluster count is max(k, largest label + 1)
 *   options  NULL = dsm_default_clustering_options.  SPECTRAL with k >= images (Spectra needs nev < ncv <= n): invalid
 * Per image of the used edges, sorted by id (capacity 2 * n_pairs each): image_ids_out, labels_out (intra cluster);
 *   *n_images_out = their number.
 * Per input edge: edge_cluster -1 unused / masked / repeat, -2 lost (between two intra clusters) and not added back,
 *   otherwise the inter cluster that holds the edge.
 * Inter clusters: cluster_images[cluster_offsets[c] .. cluster_offsets[c + 1]) their images sorted by id; capacities
 *   2 * n_pairs + 1 (offsets) and 3 * n_pairs (images); *n_clusters_out = their number.
 * report (may be NULL).  Host pointers.  No used edge: DSM_OK with no image and no cluster.  The eigen-solver ending above
 * the tolerance after max_eigen_iterations: DSM_ERR_NOT_CONVERGED (the reference goes on with empty vectors). */
int dsm_view_graph_cluster(dsm_ctx* ctx, uint32_t n_pairs, const uint32_t* pairs, const int32_t* weights, const uint8_t* use,
                           const uint32_t* labels_in, const dsm_clustering_options* options, uint32_t* image_ids_out,
                           uint32_t* labels_out, uint32_t* n_images_out, int32_t* edge_cluster, uint32_t* cluster_offsets,
                           uint32_t* cluster_images, uint32_t* n_clusters_out, dsm_clustering_report* report);
/* The spectrum behind the labels of the last dsm_view_graph_cluster on this context that ran the eigen-solver: the ncv final
 * Ritz values ascending (*n_values; the first k are the eigenvalues the labels come from) and the k Ritz vectors the
 * k-means ran on, [n_rows = images][n_cols = k] row-major.  The first min(count, capacity) of each are copied; either
 * array may be NULL with capacity 0. */
int dsm_get_clustering_spectrum(dsm_ctx* ctx, double* values, uint32_t values_capacity, double* vectors, uint64_t vectors_capacity,
                                uint32_t* n_values, uint32_t* n_rows, uint32_t* n_cols);

/* ------------------------------------------------------------------ cluster alignment
 * The merge step after every cluster is reconstructed: SfMAligner::Align() (src/controllers/sfm_aligner.cpp:149-228) as
 * MergeClusters() calls it (distributed_mapper_controller.cpp:742-795), up to the transforms; Reconstruction::Merge stays
 * with the host application.
 *   For clusters i < j: the common registered images (all of them go to the separators); the correspondences
 *   (X(P1) in i, X(P2) in j) of every track element of a point P2 of j on a common image whose point2D carries a point P1 of
 *   i, ordered by ascending point id of j, then (image_id, point2D_idx).  Pairs with >= 2 common images estimate i -> j and
 *   j -> i: N > 5 PROSAC (sample 4, MLE cost, Umeyama with scaling) and the refit, 3 <= N <= 5 Umeyama on all N; msd is the
 *   mean residual over all N; the edge weight max(msd_ij, msd_ji) is kept when <= max_reprojection_error (as float).
 *   Then the largest component, Kruskal's MST, the anchor (leaves removed layer by layer) and the composed Sim3s.
 *   Free choices: no edge for N <= 2 (the reference: NaN / a rotation-only LM); the closed form instead of
 *   Refine_RTS; seeds per (i, j, direction); ties by cluster index. */
typedef struct dsm_align_options {
  double threshold;              /* 0.1: PROSAC error_thresh (AlignOptions); <= 0 or non-finite -> DSM_ERR_INVALID_ARGUMENT */
  double max_reprojection_error; /* 1.8: larger edge weights are dropped */
  double failure_probability;    /* 0.01 (RansacParameters); outside (0, 1) -> invalid */
  int32_t min_iterations;        /* 100 */
  int32_t max_iterations;        /* 5000; > 5000 or < min_iterations or < 1 -> invalid (PROSAC's index range) */
  uint32_t random_seed;          /* user part of the per-direction seeds, dsm_align_seed */
  uint32_t reserved;
} dsm_align_options;

/* one cluster pair with >= 2 common registered images; direction 0 is i -> j (x_j ~ s R x_i + t), 1 is j -> i */
typedef struct dsm_align_pair {
  uint32_t i, j;
  uint32_t num_common_images;
  uint32_t num_correspondences;  /* N */
  uint32_t num_inliers[2];       /* PROSAC's final inliers (N > 5), else 0 */
  uint32_t iterations[2];        /* PROSAC iterations (N > 5), else 0 */
  int32_t edge;                  /* 1: an edge of the cluster graph */
  uint32_t reserved;
  double msd[2];                 /* mean residual over all N; NaN when N <= 2, DBL_MAX when PROSAC kept < 4 inliers */
  double weight;                 /* max(msd[0], msd[1]) */
  double s[2];
  double R[2][9];                /* row-major */
  double t[2][3];
  /* PROSAC's own result before the refit (N > 5; else cost NaN and the identity): the MLE cost of the best model over all
     N and that model */
  double prosac_cost[2];
  double prosac_s[2];
  double prosac_R[2][9];
  double prosac_t[2][3];
} dsm_align_pair;

typedef struct dsm_align_report {
  uint32_t num_clusters;
  uint32_t num_pairs;              /* pairs with >= 2 common images (the entries of pairs_out) */
  uint32_t num_edges;              /* kept edges */
  uint32_t num_in_component;       /* clusters of the largest component */
  uint32_t num_prosac_problems;    /* directions with N > 5 */
  uint32_t num_separators;
  uint64_t num_observations;
  uint64_t num_correspondences;    /* summed over every cluster pair that shares an observation */
  uint64_t prosac_iterations;      /* summed over the PROSAC problems */
  double min_residual_margin;      /* min |residual - threshold| / threshold over every residual PROSAC scored */
  double min_cost_margin;          /* min |cost - best| / best over the strict-best tests whose outcome can matter:
                                      not between two costs without an inlier (both N * threshold); a near-tie between two
                                      trials of one inlier count counts only when no better model by >= 1e-9 follows it.
                                      0 means PROSAC's choice may depend on rounding there, not that any output is wrong */
  double min_weight_margin;        /* min |weight - max_reprojection_error| / max_reprojection_error over the pairs */
  double device_ms;                /* HIP events: first upload to the last refit kernel */
  double join_ms, prosac_ms, refit_ms;
} dsm_align_report;

void dsm_default_align_options(dsm_align_options* o);
/* the default seed of direction d (0: i -> j, 1: j -> i) of clusters i < j */
uint32_t dsm_align_seed(uint32_t i, uint32_t j, uint32_t direction, uint32_t user_seed);

/* SfMAligner over K cluster reconstructions, each given as CSR over the clusters (host pointers):
 *   image_offsets[K + 1], image_ids: the registered images of each cluster (a repeat inside a cluster is ignored)
 *   point_offsets[K + 1], point_ids, point_xyz (3 doubles per point): the 3D points (ids unique inside a cluster)
 *   obs_offsets[K + 1], obs (3 x uint32 per track element: image_id, point2D_idx, point index inside the cluster)
 *   options  NULL = dsm_default_align_options; seeds NULL = dsm_align_seed, else K * K entries, seeds[a * K + b] for a -> b.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): K == 0 or K > 65536, an observation on an image the cluster has not registered, a point
 * index out of range, a repeated (image_id, point2D_idx) or point id inside one cluster, options out of range, a non-finite
 * point_xyz coordinate or threshold (checked on the host before the first launch; the message says "non-finite").
 * Outputs: pairs_out (capacity pairs_capacity; *n_pairs_out = their number, only the first min(number, capacity) written) in
 *   ascending (i, j); *anchor_out; per cluster in_component, mst_parent (-1: the anchor or outside the component) and
 *   sim3_to_anchor (13 doubles: s, R row-major, t; the identity outside the component); separators (capacity: the summed
 *   registered images) sorted ascending, *n_separators_out.  report may be NULL. */
int dsm_align_clusters(dsm_ctx* ctx, uint32_t num_clusters, const uint32_t* image_offsets, const uint32_t* image_ids,
                       const uint32_t* point_offsets, const uint64_t* point_ids, const double* point_xyz,
                       const uint32_t* obs_offsets, const uint32_t* obs, const dsm_align_options* options,
                       const uint32_t* seeds, dsm_align_pair* pairs_out, uint32_t pairs_capacity, uint32_t* n_pairs_out,
                       int32_t* anchor_out, uint8_t* in_component, int32_t* mst_parent, double* sim3_to_anchor,
                       uint32_t* separators, uint32_t* n_separators_out, dsm_align_report* report);

/* ------------------------------------------------------------------ global bundle adjustment
 * Step 8 of DistributedMapperController::Run(), AdjustGlobalBundle() (src/controllers/distributed_mapper_controller.cpp:
 * 836-931): BundleAdjuster::Solve() over the merged reconstruction with the ITERATIVE_SCHUR + SCHUR_JACOBI branch
 * (src/optim/bundle_adjustment.cc:273-284) at every size.
 *   Residual: BundleAdjustmentCostFunction (src/base/cost_functions.h:45-85): UnitQuaternionRotatePoint(qvec, X) + tvec,
 *   divided by z, CameraModel::WorldToImage (src/base/camera_models.h), minus the observation; the trivial loss.
 *   Blocks (bundle_adjustment.cc:330-456): qvec with QuaternionParameterization (normalised first, :345), tvec with a
 *   subset parameterisation of the constant-tvec mask, constant pose -> both constant; camera params with a subset
 *   parameterisation of the indices the refine flags keep (ParameterizeCameras), all three flags off -> constant; a constant
 *   point keeps its residuals with a fixed block.  Images and cameras without residuals are not in the problem and come back
 *   bit-identical.
 *   Minimiser: Levenberg-Marquardt trust region with Jacobi scaling, the Schur complement over the variable points solved
 *   by Jacobi-block-preconditioned CG (rules in DESIGN.md 12). */
enum { DSM_BA_CONVERGENCE = 0, DSM_BA_NO_CONVERGENCE = 1, DSM_BA_FAILURE = 2 };  /* ceres::TerminationType names */

typedef struct dsm_bundle_adjustment_options {
  int32_t max_num_iterations;                /* 50 (GlobalBundleAdjustment(), bundle_adjustment.h:522-542); >= 0 */
  int32_t max_linear_solver_iterations;      /* 100 (BundleAdjustmentOptions ctor, bundle_adjustment.h:70-90); >= 1 */
  double gradient_tolerance;                 /* 1.0 */
  double function_tolerance;                 /* 0 */
  double parameter_tolerance;                /* 0 */
  int32_t max_num_consecutive_invalid_steps; /* 10 (Solver::Options); >= 0 */
  int32_t refine_focal_length;               /* 1 */
  int32_t refine_principal_point;            /* 0 */
  int32_t refine_extra_params;               /* 1 */
} dsm_bundle_adjustment_options;

typedef struct dsm_bundle_adjustment_report {
  int32_t termination;                /* DSM_BA_CONVERGENCE / DSM_BA_NO_CONVERGENCE / DSM_BA_FAILURE */
  int32_t num_iterations;             /* LM iterations after iteration 0, accepted or not */
  int32_t num_successful_steps;
  int32_t num_invalid_steps;
  uint64_t num_residuals;             /* 2 x observations */
  uint64_t num_effective_parameters;  /* tangent dimensions of the variable blocks */
  uint64_t total_cg_iterations;
  double initial_cost, final_cost;    /* 1/2 sum |r|^2 over every observation */
  double initial_mean_reprojection_error, final_mean_reprojection_error;  /* mean |r| */
  /* the smallest margin of every decision a rounding difference could flip (DBL_MAX when never taken): the acceptance test
     rho > 1e-3 as |(cost - candidate_cost) - 1e-3 model_cost_change| / cost; the CG stop test and the gradient test as
     |a - t| / max(|a|, |t|) against eta = 0.1 and gradient_tolerance */
  double min_rho_margin, min_cg_margin, min_gradient_margin;
  double setup_ms;                    /* host validation, canonical sort and upload (host clock) */
  double jacobian_ms, cg_ms, candidate_ms, total_ms;  /* HIP events */
} dsm_bundle_adjustment_report;

#define DSM_BA_TRACE_COLUMNS 6  /* per iteration: cost, radius, rho, CG iterations, accepted, gradient max-norm */

void dsm_default_bundle_adjustment_options(dsm_bundle_adjustment_options* o);

/* Bundle adjustment in place (host pointers):
 *   cameras: camera_model_ids[num_cameras] (the eleven models), camera_params: each camera's parameters back to back in
 *     camera order (CameraModel::kNumParams of its model each)
 *   images: image_camera[num_images], image_qvec (4 per image, w x y z), image_tvec (3), image_constant_pose (NULL = none),
 *     image_constant_tvec (NULL = none; bit k: tvec[k] constant)
 *   points: point_ids (unique), point_xyz (3), point_constant (NULL = none), track_offsets[num_points + 1], obs_image[n],
 *     obs_xy[2 n] (n = track_offsets[num_points])
 *   options NULL = dsm_default_bundle_adjustment_options; report may be NULL; trace NULL or (max_num_iterations + 1) x
 *     DSM_BA_TRACE_COLUMNS doubles (rows past the last iteration untouched).
 * Invalid (DSM_ERR_INVALID_ARGUMENT): an unknown model, an out-of-range index, a track shorter than 2, one image observing one
 *   point twice, a repeated point id, non-finite input, a zero qvec, a mask above 7, no residuals, options out of range.
 * The result is the same bytes for every order of the points and of the elements inside a track. */
int dsm_bundle_adjust(dsm_ctx* ctx, uint32_t num_cameras, const int32_t* camera_model_ids, double* camera_params,
                      uint32_t num_images, const uint32_t* image_camera, double* image_qvec, double* image_tvec,
                      const uint8_t* image_constant_pose, const uint8_t* image_constant_tvec, uint32_t num_points,
                      const uint64_t* point_ids, double* point_xyz, const uint8_t* point_constant, const uint32_t* track_offsets,
                      const uint32_t* obs_image, const double* obs_xy, const dsm_bundle_adjustment_options* options,
                      dsm_bundle_adjustment_report* report, double* trace);

/* ------------------------------------------------------------------ re-triangulation of the separators
 * Step 7 of DistributedMapperController::Run(), Triangulate() (src/controllers/distributed_mapper_controller.cpp:823-834):
 * IncrementalTriangulator::TriangulateImage (src/sfm/incremental_triangulator.cc:61-117) for every separator image of the
 * merged reconstruction, with Find (max_transitivity 1), Continue and Create (LORANSAC, CombinationSampler, ANGULAR_ERROR
 * residuals; recursion on the unused correspondences) as the reference runs them.  The correspondence graph is built from
 * the verified pairs as CorrespondenceGraph::AddCorrespondences does (one call per pair in input order; a match whose feature
 * already holds a correspondence to the other image is dropped).
 *   Rulings: separators run in ascending image id (the reference: an unordered_set); new point ids are the ids
 *   the sequential run hands out from next_point3D_id, in (separator, point2D, recursion depth) order, however the device
 *   schedules the problems; Continue's angular error uses the projection matrix like Create's residual (the reference
 *   rotates by the quaternion; the same value up to rounding); self-pairs, repeated pairs (either order), repeated ids and
 *   out-of-range indices are refused instead of dropped. */
typedef struct dsm_triangulation_options {
  double create_max_angle_error;   /* 2.0 degrees */
  double continue_max_angle_error; /* 2.0 degrees */
  double min_angle;                /* 1.5 degrees */
  double min_focal_length_ratio;   /* 0.1  (HasBogusParams) */
  double max_focal_length_ratio;   /* 10.0 */
  double max_extra_param;          /* 1.0 */
  double ransac_confidence;        /* 0.9999 */
  double ransac_min_inlier_ratio;  /* 0.02 (LORANSAC does not read it; kept for the record) */
  int32_t ransac_max_num_trials;   /* 10000 */
  int32_t ignore_two_view_tracks;  /* 1 */
  int32_t max_transitivity;        /* 1; any other value is DSM_ERR_INVALID_ARGUMENT */
  int32_t reserved;
} dsm_triangulation_options;

typedef struct dsm_triangulation_report {
  uint32_t num_separators;        /* separators processed: registered, camera without bogus parameters */
  uint32_t num_rounds;            /* commit rounds of the schedule */
  uint64_t num_problems;          /* (separator, point2D) with a non-empty filtered correspondence list */
  uint64_t num_deferred;          /* problems deferred, summed over the rounds */
  uint64_t num_correspondences;   /* directed entries of the correspondence graph */
  uint64_t ransac_trials;         /* LORANSAC trials, summed over every Create level */
  uint64_t num_tris;              /* observations added: Continue's plus the new tracks' */
  uint64_t num_new_points;
  uint64_t num_new_observations;
  uint64_t num_continued;
  /* the smallest relative margin of every decision a rounding difference could flip (INFINITY when never taken):
     |residual - max_error^2| / max_error^2, equal-count support sums |s1 - s2| / max, |angle - min_angle| / min_angle,
     cheirality |depth - eps| / max(|depth|, eps), Continue's best against the second best and against the threshold,
     the bogus-parameter ratios against their bounds; 0 for a residual whose cosine is at or above 1 - 8 eps (acos NaN, or
     NaN by rounding: the reference counts NaN as an outlier) */
  double min_residual_margin, min_support_margin, min_angle_margin, min_depth_margin, min_continue_margin, min_bogus_margin;
  double setup_ms;                /* host validation and canonical order (host clock) */
  double graph_ms;                /* HIP events: uploads, duplicate rule, sort, offsets */
  double continue_ms, ransac_ms;  /* HIP events, summed over the rounds */
  double schedule_ms;             /* the round schedule: one pass over the problems' feature sets (host clock) */
  double apply_ms;                /* HIP events: the state updates of every round */
  double round_gap_ms;            /* device time of the rounds outside their kernels (launch gaps) */
  double download_ms;             /* HIP events: the results back to the host */
  double assemble_ms;             /* ids, tracks and lists from the results (host clock) */
  double replay_ms;               /* schedule_ms + apply_ms + round_gap_ms + assemble_ms */
  double device_ms;               /* HIP events: first upload to the last download */
} dsm_triangulation_report;

void dsm_default_triangulation_options(dsm_triangulation_options* o);

/* TriangulateImage over the separators (host pointers).  T = points2D_offsets[num_images] below.
 *   cameras: camera_ids[num_cameras] (unique), cameras (the eleven models; width and height feed the bogus test)
 *   images: image_ids[num_images] (unique), image_camera_ids, image_registered (0 / 1), image_qvec (4 each, w x y z),
 *     image_tvec (3 each), points2D_offsets[num_images + 1] (CSR over the images in input order, <= 262144 per image),
 *     points2D_xy (2 per point2D), points2D_point3D (an index into the points3D or -1)
 *   points3D: point3D_ids (unique), point3D_xyz (3 each)
 *   pairs: pair_image_ids (2 per pair), match_offsets[num_pairs + 1] (uint64), matches (idx1, idx2 per match), in load order
 *   separators: separator_ids (unique image ids, any order; as dsm_align_clusters returns them)
 *   next_point3D_id: the first new id; 0 = the largest existing id + 1; at or below an existing id: invalid
 * Outputs, each with room for T entries (pairs of uint32 for an observation, 3 doubles for an xyz):
 *   new points in id order: new_point_ids, new_point_xyz, new_track_offsets[n + 1], new_track_obs (image_id, point2D_idx; the
 *     track in the order of Create's correspondence list, the reference observation last); *n_new_points
 *   continued_obs (image_id, point2D_idx) with continued_point_ids, in the sequential order; *n_continued
 *   touched_obs (image_id, point2D_idx) ascending with touched_point_ids: every point2D that received a point; *n_touched
 *   num_tris_per_separator[num_separators] (input order; 0 for an unregistered or bogus separator), *num_tris_out
 * Output arrays other than the counts may be NULL.  report may be NULL.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): a self-pair, a repeated pair, a repeated id, an unknown image / camera id, an index out
 *   of range, non-finite input, a zero qvec, an unknown camera model, options out of range.
 * The result is the same bytes for any order of the points3D and of the matches inside a pair (when no match of the pair is
 * dropped as a duplicate). */
int dsm_retriangulate(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                      uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                      const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                      const uint32_t* points2D_offsets, const double* points2D_xy, const int32_t* points2D_point3D,
                      uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, uint32_t num_pairs,
                      const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                      uint32_t num_separators, const uint32_t* separator_ids, uint64_t next_point3D_id,
                      const dsm_triangulation_options* options, uint64_t* new_point_ids, double* new_point_xyz,
                      uint64_t* new_track_offsets, uint32_t* new_track_obs, uint64_t* n_new_points, uint32_t* continued_obs,
                      uint64_t* continued_point_ids, uint64_t* n_continued, uint32_t* touched_obs, uint64_t* touched_point_ids,
                      uint64_t* n_touched, uint32_t* num_tris_per_separator, uint64_t* num_tris_out,
                      dsm_triangulation_report* report);

/* ------------------------------------------------------------------ re-triangulation of under-reconstructed image pairs
 * IncrementalTriangulator::Retriangulate (src/sfm/incremental_triangulator.cc:289-390), what IterativeGlobalRefinement runs
 * before every global bundle adjustment of a cluster (src/controllers/incremental_mapper_controller.cc:114-116): for every
 * image pair whose share of triangulated correspondences is below re_min_ratio at its turn, Continue (threshold
 * re_max_angle_error) or a two-view Create (threshold create_max_angle_error, :380-382) per correspondence.  The
 * correspondence graph, ImageToWorld, the two-view triangulation and the tests are those of dsm_retriangulate.
 *   Rulings: pairs run in ascending (min image id, max image id), i.e. ascending ImagePairToPairId (the
 *   reference: an unordered_map); image1 is the image with the smaller id however the input pair is written; a pair's
 *   correspondences run in FindCorrespondencesBetweenImages order, ascending point2D index of image1, not in load order;
 *   num_total_corrs is the number of matches a pair keeps after the duplicate rule, and a pair that keeps none is skipped
 *   without a trial (status DSM_PAIR_NOT_UNDER_RECONSTRUCTED); num_tri_corrs is the number of kept matches whose two features
 *   carry the same point3D (what SetObservationAsTriangulated maintains, reconstruction.cc:2018-2050), recomputed from the
 *   feature -> point state; per pair, in the reference's order: (double)tri / (double)total >= re_min_ratio skips, an
 *   unregistered image skips, re_num_trials >= re_max_trials skips, re_num_trials is incremented, a camera with bogus
 *   parameters skips (the trial stays counted); per correspondence: both features with a point: nothing; exactly one: Continue
 *   of the other feature onto that point, the angular error through the projection matrix as in dsm_retriangulate; neither:
 *   Create over {feature of image1, feature of image2}, skipped with ignore_two_view_tracks when IsTwoViewObservation holds
 *   for the feature of image1 (correspondence_graph.cc:250-261); Create on two views is one LORANSAC trial without local
 *   optimisation: triangulate, both cheirality depths, the triangulation angle against min_angle, both residuals within the
 *   threshold, and the new track is (image1, image2); new point ids are handed out from next_point3D_id in sequential
 *   (pair, correspondence) order however the device schedules the pairs. */
typedef struct dsm_pair_retriangulation_options {
  dsm_triangulation_options tri;   /* as dsm_retriangulate reads it; continue_max_angle_error is replaced by re_max_angle_error */
  double re_max_angle_error;       /* 5.0 degrees */
  double re_min_ratio;             /* 0.2 */
  int32_t re_max_trials;           /* 1 */
  int32_t reserved;
} dsm_pair_retriangulation_options;

enum {
  DSM_PAIR_NOT_UNDER_RECONSTRUCTED = 0, /* tri / total >= re_min_ratio when the call started (or no kept match) */
  DSM_PAIR_CLOSED_BY_ITS_TURN = 1,      /* open when the call started, closed by what earlier pairs of the call added */
  DSM_PAIR_UNREGISTERED = 2,
  DSM_PAIR_TRIALS_EXHAUSTED = 3,
  DSM_PAIR_BOGUS_CAMERA = 4,            /* the trial is counted */
  DSM_PAIR_PROCESSED = 5
};

typedef struct dsm_pair_retriangulation_report {
  uint32_t num_candidates;        /* pairs open on the input state, registered, with trials left, on cameras that pass */
  uint32_t num_rounds;            /* rounds of the schedule: 1 + the longest chain of candidate pairs sharing features */
  uint64_t num_pairs_by_status[6];
  uint64_t num_correspondences;   /* matches kept after the duplicate rule, over all pairs */
  /* the correspondences of the processed pairs by case; tried = taken + rejected (a two-view skip is not a try) */
  uint64_t num_both, num_continue_tried, num_continue_taken, num_two_view_skipped, num_create_tried, num_create_taken;
  uint64_t num_tris;              /* observations added: one per Continue taken, two per point created */
  uint64_t num_new_points;
  uint64_t num_continued;
  /* the margins of dsm_triangulation_report that occur here (INFINITY when never taken): both residuals of a Create,
     its triangulation angle, its cheirality depths, Continue's error against re_max_angle_error, the bogus ratios */
  double min_residual_margin, min_angle_margin, min_depth_margin, min_continue_margin, min_bogus_margin;
  double setup_ms;                /* host validation and canonical order (host clock) */
  double graph_ms;                /* HIP events: uploads, duplicate rule, ranks, the correspondence lists, the first counts */
  double schedule_ms;             /* candidates and their rounds: one pass over the candidates' feature sets (host clock) */
  double rounds_ms;               /* HIP events: the first round's gate to the last round's solve */
  double gate_ms, solve_ms;       /* HIP events, summed over the rounds; 0 in a call of more than 1024 rounds, which records
                                     no events per round */
  double round_gap_ms;            /* rounds_ms outside the kernels (launch gaps); 0 where gate_ms and solve_ms are */
  double download_ms;             /* HIP events: the final counts and the results back to the host */
  double assemble_ms;             /* ids, tracks and lists from the results (host clock) */
  double device_ms;               /* HIP events: first upload to the last download */
} dsm_pair_retriangulation_report;

void dsm_default_pair_retriangulation_options(dsm_pair_retriangulation_options* o);

/* Retriangulate over the image pairs (host pointers).  The scene arguments are those of dsm_retriangulate, without the
 * separators.  T = points2D_offsets[num_images].
 *   re_num_trials[num_pairs]: the trials every pair has had (the reference's re_num_trials_, which persists across calls; here
 *     the host owns it), in input pair order; read, and written with the trials of this call added.  NULL: zeros, nothing out.
 * Outputs, each with room for T entries unless its size is given:
 *   new points in id order: new_point_ids, new_point_xyz (3 each), new_track_obs (4 each: image_id1, point2D_idx1, image_id2,
 *     point2D_idx2); *n_new_points
 *   continued_obs (image_id, point2D_idx) with continued_point_ids, in the sequential order; *n_continued
 *   touched_obs (image_id, point2D_idx) ascending with touched_point_ids: every point2D that received a point; *n_touched
 *   pair_num_total_corrs[num_pairs], pair_num_tri_corrs[num_pairs] (after the call), pair_status[num_pairs] (DSM_PAIR_*), in
 *     input pair order; *num_tris_out
 * Output arrays other than the counts may be NULL.  report may be NULL.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): everything dsm_retriangulate refuses; a non-finite or non-positive re_max_angle_error; a
 *   non-finite or negative re_min_ratio; a negative re_max_trials.
 * The result is the same bytes for any order of the points3D, for any order of the matches inside a pair (when no match of
 * the pair is dropped as a duplicate), and for a pair written as (image2, image1) with its matches swapped. */
int dsm_retriangulate_pairs(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                            uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                            const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                            const uint32_t* points2D_offsets, const double* points2D_xy, const int32_t* points2D_point3D,
                            uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz, uint32_t num_pairs,
                            const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                            uint64_t next_point3D_id, const dsm_pair_retriangulation_options* options, uint32_t* re_num_trials,
                            uint64_t* new_point_ids, double* new_point_xyz, uint32_t* new_track_obs, uint64_t* n_new_points,
                            uint32_t* continued_obs, uint64_t* continued_point_ids, uint64_t* n_continued, uint32_t* touched_obs,
                            uint64_t* touched_point_ids, uint64_t* n_touched, uint32_t* pair_num_total_corrs,
                            uint32_t* pair_num_tri_corrs, uint8_t* pair_status, uint64_t* num_tris_out,
                            dsm_pair_retriangulation_report* report);

/* ------------------------------------------------------------------ absolute pose estimation (image registration)
 * EstimateAbsolutePose (src/estimators/pose.cc:48-158) as IncrementalMapper::RegisterNextImage calls it
 * (src/sfm/incremental_mapper.cc:438-496), for a batch of independent problems: per problem a camera, N
 * 2D-3D correspondences and the flag estimate_focal_length.  One LO-RANSAC (P3P minimal solver, EPnP local optimisation,
 * src/optim/loransac.h:91-233) per focal-length factor; the unit of work is the RUN = (problem, factor).
 * Every run draws from its own MT19937 stream: the results depend on the problem, the options and the seeds alone, not on
 * the batch, the order of the problems or the schedule. */
#define DSM_ABSOLUTE_POSE_MAX_POINTS 1048576u  /* correspondences of one problem; more is DSM_ERR_INVALID_ARGUMENT */
#define DSM_ABSOLUTE_POSE_MAX_FACTORS 1024u    /* focal-length factors (num_focal_length_samples + 1 at most) */
#define DSM_ABSOLUTE_POSE_MAX_TRIALS 1000000u  /* trials of one run after RANSAC's constructor cap; more is DSM_ERR_INVALID_ARGUMENT */
typedef struct dsm_absolute_pose_options {
  int32_t num_focal_length_samples; /* 30    AbsolutePoseEstimationOptions, src/estimators/pose.h:55; incremental_mapper.cc:440 */
  int32_t reserved;
  double min_focal_length_ratio;    /* 0.1   incremental_mapper.h:106 (pose.h:59 has 0.2) */
  double max_focal_length_ratio;    /* 10    incremental_mapper.h:107 (pose.h:63 has 5) */
  double max_error;                 /* 12.0  pixels, abs_pose_max_error, incremental_mapper.h:84 */
  double min_inlier_ratio;          /* 0.25  abs_pose_min_inlier_ratio, incremental_mapper.h:90 */
  double confidence;                /* 0.9999 incremental_mapper.cc:449 */
  uint64_t min_num_trials;          /* 30    incremental_mapper.cc:448 */
  uint64_t max_num_trials;          /* UINT64_MAX: RANSACOptions' default (ransac.h:62), which the mapper leaves; RANSAC's constructor caps it
                                       (ransac.h:141-147): 585 with the values above */
  uint32_t random_seed;             /* user part of the per-run seeds, dsm_absolute_pose_seed */
  uint32_t reserved2;
} dsm_absolute_pose_options;

typedef struct dsm_absolute_pose_result {
  int32_t success;            /* EstimateAbsolutePose's return value */
  int32_t factor_index;       /* index of the winning focal-length factor (-1: none) */
  uint32_t num_inliers;
  uint32_t num_trials;        /* report.num_trials of the winning run */
  int32_t model_is_local;     /* the winning model came from the local optimisation (EPnP) */
  int32_t reserved;
  double focal_length_factor; /* the winning factor (0 when none) */
  double proj_matrix[12];     /* 3 x 4, row-major */
  double qvec[4];             /* w x y z */
  double tvec[3];
  double focal_params[2];     /* the camera's focal parameters after the call (scaled only with estimate_focal_length);
                                 a model with one focal length repeats it */
} dsm_absolute_pose_result;

#define DSM_ABSOLUTE_POSE_MARGINS 9
typedef struct dsm_absolute_pose_report {
  uint32_t num_problems, num_factors; /* num_factors: runs of a problem with the flag set */
  uint64_t num_runs, num_trials, num_models, num_local_optimizations; /* summed over the runs */
  /* per problem is the call's margins_out; here the minima over the batch (INFINITY where never taken).  In order:
     0 residual against the threshold (relative)   1 depth against epsilon   2 equal-count residual sums (relative)
     3 P3P root |imag| against 1e-10 (relative)    4 P3P real root against 0 (absolute; the roots are O(1))
     5 EPnP rank pivot against its threshold       6 EPnP sign tests on b3 / b4 / b5 (relative to the largest)
     7 EPnP three-way error comparison (relative)  8 EPnP Procrustes determinant against 0 */
  double min_margin[DSM_ABSOLUTE_POSE_MARGINS];
  double setup_ms;            /* host: validation, factors, tables */
  double prepare_ms, ransac_ms, choice_ms; /* HIP events: uploads + normalisation, the runs, results back + the choice */
  double device_ms;           /* HIP events: first upload to the last download */
} dsm_absolute_pose_report;

void dsm_default_absolute_pose_options(dsm_absolute_pose_options* o);
/* seed of run (problem b, factor index s) */
uint32_t dsm_absolute_pose_seed(uint32_t problem, uint32_t factor_index, uint32_t user_seed);
/* The focal-length factors of pose.cc:87-102, the loop restated as written (its length is decided by the accumulated
 * rounding of f += 1 / n).  Writes at most `capacity` factors, returns their number (0 for options out of range). */
uint32_t dsm_absolute_pose_factors(const dsm_absolute_pose_options* options, double* factors_out, uint32_t capacity);
/* RANSAC's constructor cap on max_num_trials (ransac.h:141-147) for these options. */
uint64_t dsm_absolute_pose_max_trials(const dsm_absolute_pose_options* options);

/* Host pointers, CSR over the problems: problem b owns points offsets[b] .. offsets[b + 1].
 *   cameras[B], estimate_focal_length[B] (0 / 1), offsets[B + 1] (ascending from 0), points2D (2 per point, pixels),
 *   points3D (3 per point), options (NULL = defaults), seeds (NULL = dsm_absolute_pose_seed(b, s, options->random_seed),
 *   else B * S entries, seeds[b * S + s], S = dsm_absolute_pose_factors; a problem without the flag reads seeds[b * S])
 *   results_out[B], inlier_mask_out[offsets[B]] (0 / 1; all 0 for a failed problem), margins_out (NULL or
 *   B * DSM_ABSOLUTE_POSE_MARGINS doubles), report (NULL or the sums).
 * N < 3 is not an error: success = 0, zero trials.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, non-finite points or camera parameters, an unknown camera
 *   model, offsets that do not ascend from 0, a problem above DSM_ABSOLUTE_POSE_MAX_POINTS, more factors than
 *   DSM_ABSOLUTE_POSE_MAX_FACTORS, options outside what AbsolutePoseEstimationOptions::Check / RANSACOptions::Check accept,
 *   and options that Check accepts but that leave a run's trial count unbounded: dsm_absolute_pose_max_trials above
 *   DSM_ABSOLUTE_POSE_MAX_TRIALS (confidence = 1 or min_inlier_ratio = 0 with the default max_num_trials).  The reference
 *   loops that long on a host thread; one kernel launch must not.  Set max_num_trials to bound such a call. */
int dsm_estimate_absolute_poses(dsm_ctx* ctx, uint32_t num_problems, const dsm_camera* cameras,
                                const uint8_t* estimate_focal_length, const uint64_t* offsets, const double* points2D,
                                const double* points3D, const dsm_absolute_pose_options* options, const uint32_t* seeds,
                                dsm_absolute_pose_result* results_out, uint8_t* inlier_mask_out, double* margins_out,
                                dsm_absolute_pose_report* report);

/* ------------------------------------------------------------------ absolute pose refinement (image registration, second half)
 * RefineAbsolutePose (src/estimators/pose.cc:198-311) as IncrementalMapper::RegisterNextImage calls it
 * (src/sfm/incremental_mapper.cc:498-535) on the pose and the inlier mask of EstimateAbsolutePose, for a batch of independent
 * problems: BundleAdjustmentCostFunction with the 3D point constant under ceres::CauchyLoss(loss_function_scale),
 * qvec normalised and moved through QuaternionParameterization, tvec free, the principal point constant, the focal and the
 * extra parameters free by the problem's flags.  The trust-region rules are DESIGN.md 12's with Ceres' default function (1e-6)
 * and parameter (1e-8) tolerances and 5 consecutive invalid steps; the damped normal equations are solved by an unpivoted
 * Cholesky (the reference asks for DENSE_QR).  A result depends on the problem and the options alone. */
#define DSM_POSE_REFINEMENT_MAX_ITERATIONS 1000u /* max_num_iterations above it is DSM_ERR_INVALID_ARGUMENT: one launch holds the loop */
#define DSM_POSE_REFINE_FOCAL_LENGTH 1u          /* refine_flags bit 0: AbsolutePoseRefinementOptions::refine_focal_length */
#define DSM_POSE_REFINE_EXTRA_PARAMS 2u          /* refine_flags bit 1: refine_extra_params */
typedef struct dsm_pose_refinement_options {
  double gradient_tolerance;  /* 1.0  AbsolutePoseRefinementOptions, src/estimators/pose.h:82 */
  double loss_function_scale; /* 1.0  pose.h:88; 0 passes Check() (pose.h:102) but divides by zero: DSM_ERR_INVALID_ARGUMENT */
  int32_t max_num_iterations; /* 100  pose.h:85 */
  int32_t reserved;
} dsm_pose_refinement_options;

typedef struct dsm_pose_refinement_result {
  int32_t success;               /* RefineAbsolutePose's return value, Solver::Summary::IsSolutionUsable() */
  int32_t termination;           /* DSM_BA_CONVERGENCE / DSM_BA_NO_CONVERGENCE / DSM_BA_FAILURE */
  uint32_t num_iterations;       /* every trust-region iteration counts, as in dsm_bundle_adjustment_report */
  uint32_t num_successful_steps; /* accepted steps */
  uint32_t num_invalid_steps;
  uint32_t num_residual_blocks;  /* points with inlier_mask != 0 */
  double initial_cost, final_cost; /* 1/2 sum rho(|r|^2) */
  double qvec[4];                /* w x y z, normalised (an empty problem returns the input bits) */
  double tvec[3];
  double camera_params[12];      /* the camera's parameters after the call (dsm_camera::params) */
} dsm_pose_refinement_result;

#define DSM_POSE_REFINEMENT_MARGINS 5
/* per step in steps_out: 0 not run, then */
enum { DSM_POSE_STEP_ACCEPTED = 1, DSM_POSE_STEP_REJECTED = 2, DSM_POSE_STEP_INVALID = 3, DSM_POSE_STEP_TOLERANCE = 4 };
typedef struct dsm_pose_refinement_report {
  uint32_t num_problems, reserved;
  uint64_t num_points;     /* offsets[B] */
  uint64_t num_iterations; /* summed over the problems */
  /* per problem is the call's margins_out; here the minima over the batch (INFINITY where never taken).  In order:
     0 acceptance test, in cost: |(cost - candidate) - 1e-3 model_cost_change| / cost   1 gradient test (relative)
     2 function tolerance (relative)   3 parameter tolerance (relative)   4 Cholesky pivot against 0, relative to the diagonal */
  double min_margin[DSM_POSE_REFINEMENT_MARGINS];
  double setup_ms;                          /* host: validation */
  double upload_ms, solve_ms, download_ms;  /* HIP events: uploads, the kernel, results back */
  double device_ms;                         /* HIP events: first upload to the last download */
} dsm_pose_refinement_report;

void dsm_default_pose_refinement_options(dsm_pose_refinement_options* o);

/* Host pointers, the CSR layout of dsm_estimate_absolute_poses (its outputs feed this call without repacking):
 *   cameras[B], offsets[B + 1], points2D (2 per point, pixels), points3D (3 per point), inlier_mask[offsets[B]] (0 skips the
 *   point, pose.cc:219-223), qvecs_in[B * 4], tvecs_in[B * 3], refine_flags[B] (DSM_POSE_REFINE_* bits, as
 *   incremental_mapper.cc:451-483 sets them per image), options (NULL = defaults),
 *   results_out[B], margins_out (NULL or B * DSM_POSE_REFINEMENT_MARGINS doubles), steps_out (NULL or
 *   B * max_num_iterations bytes, DSM_POSE_STEP_* per iteration), report (NULL or the sums).
 * A problem without inliers is not an error: success = 1, zero iterations, qvec / tvec / camera parameters the input bits
 * (qvec not normalised): Ceres solves the empty problem and calls it usable.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, non-finite points, poses or camera parameters, an unknown
 *   camera model, offsets that do not ascend from 0, a problem above DSM_ABSOLUTE_POSE_MAX_POINTS, refine_flags above 3,
 *   options outside AbsolutePoseRefinementOptions::Check, loss_function_scale = 0, max_num_iterations above
 *   DSM_POSE_REFINEMENT_MAX_ITERATIONS. */
int dsm_refine_absolute_poses(dsm_ctx* ctx, uint32_t num_problems, const dsm_camera* cameras, const uint64_t* offsets,
                              const double* points2D, const double* points3D, const uint8_t* inlier_mask,
                              const double* qvecs_in, const double* tvecs_in, const uint8_t* refine_flags,
                              const dsm_pose_refinement_options* options, dsm_pose_refinement_result* results_out,
                              double* margins_out, uint8_t* steps_out, dsm_pose_refinement_report* report);

/* ------------------------------------------------------------------ point and observation filters
 * Reconstruction::FilterObservationsWithNegativeDepth, FilterPoints3DWithLargeReprojectionError,
 * FilterPoints3DWithSmallTriangulationAngle, ComputeMeanReprojectionError(track_ids) and the verdict of FilterImages
 * (src/base/reconstruction.cc:728-770, 814-858, 1352-1465) in one call, on the arrays of dsm_bundle_adjust.
 * The passes named by `passes` run in the order of their bits; each works on the survivors of the one before it:
 *   DSM_FILTER_NEGATIVE_DEPTH      an observation with row 2 of the projection matrix . (X, 1) < DBL_EPSILON goes; a point that
 *                                  would be left with fewer than two observations goes as a whole (DeleteObservation)
 *   DSM_FILTER_REPROJECTION_ERROR  observations above max_reproj_error^2 go; a point shorter than 2, or left with one
 *                                  observation or none, goes; a surviving point's error = mean |r| over the kept observations
 *   DSM_FILTER_TRIANGULATION_ANGLE a point none of whose pairs of views reaches min_tri_angle goes
 *   DSM_FILTER_MEAN_ERROR          deletes nothing: every selected surviving point's error = sum |r| over the observations in
 *                                  front of the camera / track length, and the mean over all of them
 * FilterAllPoints3D / FilterPoints3D / FilterPoints3DInImages = passes 2 | 4 with a selection; the prelude of
 * AdjustGlobalBundle = pass 1; the RMSE lines = pass 8. */
enum {
  DSM_FILTER_NEGATIVE_DEPTH = 1,
  DSM_FILTER_REPROJECTION_ERROR = 2,
  DSM_FILTER_TRIANGULATION_ANGLE = 4,
  DSM_FILTER_MEAN_ERROR = 8
};

typedef struct dsm_point_filter_options {
  double max_reproj_error;       /* 4.0 pixels (IncrementalMapper::Options::filter_max_reproj_error); >= 0 */
  double min_tri_angle;          /* 1.5 degrees (filter_min_tri_angle); >= 0 */
  double min_focal_length_ratio; /* 0.1  (HasBogusParams, incremental_mapper.h:106-108); >= 0 */
  double max_focal_length_ratio; /* 10.0 */
  double max_extra_param;        /* 1.0 */
  uint32_t passes;               /* DSM_FILTER_* bits, 1 .. 15; the default is 2 | 4 */
  uint32_t reserved;
} dsm_point_filter_options;

typedef struct dsm_point_filter_report {
  uint64_t num_points, num_observations;  /* the input's */
  uint64_t num_selected;                  /* points the selection names */
  /* per pass, in bit order (the fourth deletes nothing): the reference function's return value, points deleted,
     observations deleted (those of the deleted points included) */
  uint64_t num_filtered[4], points_deleted[4], observations_deleted[4];
  uint64_t num_points_kept, num_observations_kept;
  uint64_t num_images_filtered;
  uint64_t lane_path_tracks, wave_path_tracks; /* points served by a lane / by a one-wave workgroup (by input track length) */
  uint64_t pairs_evaluated;                    /* triangulation angles computed */
  uint64_t mean_error_observations;            /* the divisor of mean_reprojection_error */
  double mean_reprojection_error; /* pass 8: ComputeMeanReprojectionError(track_ids); NaN when nothing is selected or pass 8 did not run */
  double mean_point_error;        /* ComputeMeanReprojectionError(): the mean of the surviving points' errors that are set; 0 for none */
  /* the smallest relative margin |a - t| / max(|a|, |t|) of every decision rounding can flip (INFINITY when never taken):
     depth against DBL_EPSILON, e^2 against max_reproj_error^2, the deciding triangulation angles against min_tri_angle (a kept
     point: its first passing pair in the reference's order; a deleted point: every pair), the bogus ratios against their bounds */
  double min_depth_margin, min_error_margin, min_angle_margin, min_bogus_margin;
  double setup_ms;  /* host validation and the path bins (host clock) */
  double upload_ms, residuals_ms, tracks_ms, angles_ms, compaction_ms, download_ms; /* HIP events */
  double device_ms; /* HIP events: first upload to the last download */
} dsm_point_filter_report;

void dsm_default_point_filter_options(dsm_point_filter_options* o);

/* The filters over a reconstruction (host pointers; indices as in dsm_bundle_adjust).  n = track_offsets[num_points] below.
 *   cameras[num_cameras] (the eleven models; width and height feed the bogus test)
 *   images: image_camera[num_images], image_qvec (4 each, w x y z), image_tvec (3 each), image_registered (NULL = all)
 *   points: point_xyz (3 each), track_offsets[num_points + 1], obs_image[n], obs_xy[2 n]
 *   selection, fixed from the input before the first pass: point_selected[num_points] (NULL = all), image_selected[num_images]
 *     (NULL = none); a point is selected when its flag is set or one of its observations lies in a selected image.
 *     DSM_FILTER_REPROJECTION_ERROR, DSM_FILTER_TRIANGULATION_ANGLE and DSM_FILTER_MEAN_ERROR leave an unselected point
 *     untouched; DSM_FILTER_NEGATIVE_DEPTH ignores the selection (the reference's pass has none)
 *   options NULL = dsm_default_point_filter_options
 * Outputs, each may be NULL: point_keep[num_points], obs_keep[n] (0 / 1; 0 for every observation of a deleted point),
 *   point_error[num_points] (-1.0 = no error, Point3D::HasError; a deleted point carries -1.0), kept_track_offsets[num_points + 1]
 *   and kept_obs[n]: the surviving tracks compacted (a deleted point has an empty segment; kept_obs holds indices into the input
 *   observations, in track order, kept_track_offsets[num_points] of them), image_filtered[num_images] (1 for a registered image
 *   that observes no surviving point or whose camera has bogus parameters), report.
 * Tracks of length 0 and 1 are not refused (the passes delete them as the reference does).
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, offsets that do not ascend from 0, an index out of range, an
 *   unknown camera model, non-finite input, a zero qvec, an observation in an image flagged unregistered, passes 0 or above 15,
 *   a negative or non-finite threshold.
 * A point's results depend on that point, its images and the options alone, not on the batch or the order of the points. */
int dsm_filter_points3D(dsm_ctx* ctx, uint32_t num_cameras, const dsm_camera* cameras, uint32_t num_images,
                        const uint32_t* image_camera, const double* image_qvec, const double* image_tvec,
                        const uint8_t* image_registered, uint32_t num_points, const double* point_xyz,
                        const uint32_t* track_offsets, const uint32_t* obs_image, const double* obs_xy,
                        const uint8_t* point_selected, const uint8_t* image_selected, const dsm_point_filter_options* options,
                        uint8_t* point_keep, uint8_t* obs_keep, double* point_error, uint32_t* kept_track_offsets,
                        uint32_t* kept_obs, uint8_t* image_filtered, dsm_point_filter_report* report);

/* ------------------------------------------------------------------ local bundle adjustment (inside every cluster's mapper)
 * IncrementalMapper::AdjustLocalBundle (src/sfm/incremental_mapper.cc:562-656): BundleAdjuster::Solve() over the new image and
 * its best-connected neighbours with IncrementalMapperOptions::LocalBundleAdjustment()
 * (src/controllers/incremental_mapper_controller.cc:234-255), for a batch of independent problems.  Residual,
 * parameterisations, trust region and termination order are dsm_bundle_adjust's; additionally a robust loss
 * (Ceres' Corrector, first branch: rho'' < 0 for both losses), cameras held constant per camera, and the DENSE_SCHUR branch the
 * reference takes up to 50 images (bundle_adjustment.cc:274-278): the points are eliminated, the reduced camera system is formed
 * explicitly and factored by an unpivoted Cholesky.  One workgroup per problem runs the whole loop in one launch. */
#define DSM_LOCAL_BUNDLE_MAX_REDUCED_DIM 128u   /* columns of the reduced camera system of one problem; more is DSM_ERR_INVALID_ARGUMENT */
#define DSM_LOCAL_BUNDLE_MAX_ITERATIONS 1000u   /* max_num_iterations above it is DSM_ERR_INVALID_ARGUMENT: one launch holds the loop */
enum { DSM_LOSS_TRIVIAL = 0, DSM_LOSS_SOFT_L1 = 1, DSM_LOSS_CAUCHY = 2 };  /* BundleAdjustmentOptions::LossFunctionType */

typedef struct dsm_local_bundle_options {
  int32_t max_num_iterations;                /* 25   ba_local_max_num_iterations, incremental_mapper_controller.h; :240 */
  int32_t max_num_consecutive_invalid_steps; /* 10   (dsm_bundle_adjustment_options' value) */
  double gradient_tolerance;                 /* 10.0 incremental_mapper_controller.cc:238 */
  double function_tolerance;                 /* 0    :237 */
  double parameter_tolerance;                /* 0    :239 */
  int32_t refine_focal_length;               /* 1    :248 (ba_refine_focal_length) */
  int32_t refine_principal_point;            /* 0    :249 */
  int32_t refine_extra_params;               /* 1    :250 */
  int32_t loss_function_type;                /* DSM_LOSS_SOFT_L1  :252-253 */
  double loss_function_scale;                /* 1.0  :251; > 0 for a non-trivial loss */
} dsm_local_bundle_options;

typedef struct dsm_local_bundle_result {
  int32_t solved;                 /* BundleAdjuster::Solve's return value: 0 when the problem has no residuals */
  int32_t termination;            /* DSM_BA_CONVERGENCE / DSM_BA_NO_CONVERGENCE / DSM_BA_FAILURE */
  uint32_t num_iterations;        /* every trust-region iteration counts */
  uint32_t num_successful_steps;
  uint32_t num_invalid_steps;
  uint32_t reduced_dim;           /* columns of the reduced camera system */
  uint64_t num_residuals;         /* 2 x observations; the mapper's num_adjusted_observations is half of it */
  uint64_t num_effective_parameters; /* tangent dimensions of the variable blocks */
  double initial_cost, final_cost;   /* 1/2 sum rho(|r|^2) */
  double initial_mean_reprojection_error, final_mean_reprojection_error; /* mean |r| (before the loss) */
} dsm_local_bundle_result;

#define DSM_LOCAL_BUNDLE_MARGINS 4
#define DSM_LOCAL_BUNDLE_TRACE_COLUMNS 5 /* DSM_BA_TRACE_COLUMNS without the CG count: cost, radius, rho, accepted, gradient max-norm */
typedef struct dsm_local_bundle_report {
  uint32_t num_problems, reserved;
  uint64_t num_points, num_observations; /* summed over the problems */
  uint64_t num_iterations;
  /* per problem is the call's margins_out; here the minima over the batch (INFINITY where never taken).  In order:
     0 acceptance test, in cost: |(cost - candidate) - 1e-3 model_cost_change| / cost   1 gradient test (relative)
     2 Cholesky pivot of the reduced system, relative to its diagonal   3 pivot of a point's 3 x 3 block, relative to its diagonal */
  double min_margin[DSM_LOCAL_BUNDLE_MARGINS];
  double setup_ms;                          /* host: validation and the canonical order */
  double upload_ms, solve_ms, download_ms;  /* HIP events */
  double device_ms;                         /* HIP events: first upload to the last download */
} dsm_local_bundle_report;

void dsm_default_local_bundle_options(dsm_local_bundle_options* o);

/* B independent problems, CSR over the problems, host pointers, adjusted in place; indices inside a problem are local to it.
 *   cameras: camera_offsets[B + 1]; camera_model_ids; camera_params (every camera's parameters back to back, in camera order
 *     over the whole batch); camera_constant (NULL = none; 1 holds the camera constant whatever the refine flags say)
 *   images: image_offsets[B + 1]; image_camera (index into the problem's cameras); image_qvec (4 each); image_tvec (3 each);
 *     image_constant_pose, image_constant_tvec (NULL = none; bit k: tvec[k] constant) as in dsm_bundle_adjust
 *   points: point_offsets[B + 1]; point_ids (unique inside a problem: the canonical order); point_xyz; point_constant (NULL = none)
 *   tracks: track_offsets holds, for problem b, num_points_b + 1 entries starting at point_offsets[b] + b, counted from 0
 *     inside the problem; obs_offsets[B + 1] says where a problem's observations start in obs_image / obs_xy.  A track of
 *     length 1 (or 0) is accepted.
 *   options NULL = defaults; results_out[B]; margins_out NULL or B x DSM_LOCAL_BUNDLE_MARGINS; trace_out NULL or
 *     B x (max_num_iterations + 1) x DSM_LOCAL_BUNDLE_TRACE_COLUMNS (rows past a problem's last iteration are NaN); report NULL or
 *     the sums.
 * A problem without residuals: solved = 0, nothing touched.  A problem with residuals and no variable block: CONVERGENCE after
 * zero iterations, nothing touched.  Blocks without residuals come back bit-identical.
 * A problem's result depends on that problem and the options alone: not on the batch, its place in it, or the order of its
 * points, track elements, images or cameras.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, offsets that do not ascend from 0, an unknown model, an
 *   out-of-range index, non-finite input, a zero qvec, a mask above 7, one image observing one point twice, a repeated point
 *   id, an unknown loss type, loss_function_scale <= 0 for a non-trivial loss, options out of range, max_num_iterations above
 *   DSM_LOCAL_BUNDLE_MAX_ITERATIONS, a reduced camera system above DSM_LOCAL_BUNDLE_MAX_REDUCED_DIM columns (such a problem
 *   belongs to dsm_bundle_adjust). */
int dsm_adjust_local_bundles(dsm_ctx* ctx, uint32_t num_problems, const uint32_t* camera_offsets, const int32_t* camera_model_ids,
                             double* camera_params, const uint8_t* camera_constant, const uint32_t* image_offsets,
                             const uint32_t* image_camera, double* image_qvec, double* image_tvec,
                             const uint8_t* image_constant_pose, const uint8_t* image_constant_tvec,
                             const uint32_t* point_offsets, const uint64_t* point_ids, double* point_xyz,
                             const uint8_t* point_constant, const uint32_t* track_offsets, const uint64_t* obs_offsets,
                             const uint32_t* obs_image, const double* obs_xy, const dsm_local_bundle_options* options,
                             dsm_local_bundle_result* results_out, double* margins_out, double* trace_out,
                             dsm_local_bundle_report* report);

/* ---- SIFT feature extraction ----
 * ExtractSiftFeaturesCPU (src/feature/sift.cc:252-426): VLFeat's vl_sift_process_first_octave / _next_octave, vl_sift_detect,
 * vl_sift_calc_keypoint_orientations and vl_sift_calc_keypoint_descriptor (lib/VLFeat/sift.c:975-1431, 1559-1692, 1923-2093)
 * restated in the reference's evaluation order, and COLMAP's loop around them: the groups per DoG level, the first
 * max_num_orientations orientations of a keypoint, L1_ROOT / L2 (src/feature/utils.cc:47-77), the bytes, the VLFeat -> UBC bin
 * order (sift.cc:58-74) and the max_num_features cut (sift.cc:387-398; the level that crosses the limit is kept whole).
 * DESIGN.md 18.  ExtractCovariantSiftFeaturesCPU is below: dsm_extract_covariant_sift (domain_size_pooling) and
 * dsm_extract_covariant_sift_affine (estimate_affine_shape as well).  SiftGPU is not covered. */
enum { DSM_SIFT_L1_ROOT = 0, DSM_SIFT_L2 = 1 };  /* SiftExtractionOptions::Normalization, src/feature/sift.h */

typedef struct dsm_sift_options {  /* SiftExtractionOptions, src/feature/sift.h:36-112 */
  int32_t num_octaves;          /* 4; negative: as many as the image allows (vl_sift_new, sift.c:885-887) */
  int32_t octave_resolution;    /* 3 */
  int32_t first_octave;         /* -1 */
  int32_t max_num_orientations; /* 2 */
  int32_t max_num_features;     /* 8192 */
  int32_t upright;              /* 0 */
  int32_t normalization;        /* DSM_SIFT_L1_ROOT */
  int32_t reserved;
  double peak_threshold;        /* 0.02 / octave_resolution */
  double edge_threshold;        /* 10.0 */
} dsm_sift_options;

void dsm_sift_default_options(dsm_sift_options* o);

/* One grey image, host pointers: gray_u8 holds height rows of row_stride >= width bytes.  keypoints_out [capacity x 4] receives
 * (x + 0.5, y + 0.5, sigma, angle) as sift.cc:355-357 hands them to FeatureKeypoint(x, y, scale, orientation); descriptors_out
 * [capacity x 128] the bytes in UBC order, NULL where only keypoints are wanted (sift.cc:358).  options NULL = the defaults.
 * *num_features_out: the number of features found; above capacity the call fails with DSM_ERR_OUT_OF_RANGE, nothing is written
 * to the outputs and the count is still valid.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, an empty image, row_stride < width, options that
 *   SiftExtractionOptions::Check (sift.cc:218-234) rejects, an unknown normalization.
 * DSM_ERR_OUT_OF_RANGE: first_octave outside -4 .. 16, octave_resolution or num_octaves above 64, a first octave of 2^31
 *   samples or more over its levels, or one whose scratch exceeds dsm_ctx_set_memory_budget (the stage does not tile). */
int dsm_extract_sift(dsm_ctx* ctx, const dsm_sift_options* options, const uint8_t* gray_u8, uint32_t width, uint32_t height,
                     uint32_t row_stride, uint32_t capacity, float* keypoints_out, uint8_t* descriptors_out,
                     uint32_t* num_features_out);

/* HIP-event times of the last dsm_extract_sift on this context, in ms, summed over the octaves: 0 the octave's base (load, up- /
 * downsampling, its smoothing), 1 the smoothing of the levels, 2 DoG + extremum test + candidate count, 3 candidate emission +
 * refinement, 4 gradient, 5 orientations, 6 descriptors.  DSM_ERR_NOT_READY before the first call. */
#define DSM_SIFT_STAGES 7
int dsm_get_sift_time(dsm_ctx* ctx, double* stage_ms);

/* ---- covariant SIFT feature extraction with domain-size pooling ----
 * ExtractCovariantSiftFeaturesCPU (src/feature/sift.cc:428-598) with estimate_affine_shape = false: the extractor
 * SiftExtraction.domain_size_pooling selects (src/feature/extraction.cc:374-380).  VLFeat's scale space (lib/VLFeat/
 * scalespace.c:669-812, imopv.c:620-679), the DoG detector of covdet (covdet.c:1921-2144 with :1057-1126 and :1206-1318), its
 * orientations (:2698-2892), its patch extraction (:2166-2446) and vl_sift_calc_raw_descriptor (sift.c:1754-1903) restated in
 * the reference's evaluation order, and COLMAP's loop around them: the std::sort by (o, s) descending (sift.cc:479-487), the
 * cut that keeps the crossing (o, s) group whole (:489-513), the pooling scales (:530-553), the mean over them (:577),
 * L1_ROOT / L2, the bytes and the VLFeat -> UBC bin order.  DESIGN.md 21. */
typedef struct dsm_covariant_sift_options {  /* SiftExtractionOptions, src/feature/sift.h:36-112 */
  int32_t octave_resolution;      /* 3 */
  int32_t first_octave;           /* -1 */
  int32_t max_num_features;       /* 8192 */
  int32_t upright;                /* 0 */
  int32_t normalization;          /* DSM_SIFT_L1_ROOT */
  int32_t estimate_affine_shape;  /* 0; 1: dsm_extract_covariant_sift_affine runs vl_covdet_extract_affine_shape, and
                                   * dsm_extract_covariant_sift answers DSM_ERR_INVALID_ARGUMENT */
  int32_t domain_size_pooling;    /* 1; 0: one scale of 1, as the reference's function does without it */
  int32_t dsp_num_scales;         /* 10 */
  double peak_threshold;          /* 0.02 / octave_resolution */
  double edge_threshold;          /* 10.0 */
  double dsp_min_scale;           /* 1.0 / 6.0 */
  double dsp_max_scale;           /* 3.0 */
} dsm_covariant_sift_options;
/* num_octaves and max_num_orientations have no field: covdet reads neither.  The last octave comes from the image
 * (covdet.c:1699: floor(log2(min(width - 1, height - 1) / 15))), and at most four orientations are kept (covdet.c:1432). */

void dsm_covariant_sift_default_options(dsm_covariant_sift_options* o);

/* One grey image, host pointers: gray_u8 holds height rows of row_stride >= width bytes.  keypoints_out [capacity x 6] receives
 * (x + 0.5, y + 0.5, a11, a12, a21, a22) as sift.cc:494-501 fills FeatureKeypoint; descriptors_out [capacity x 128] the bytes in
 * UBC order, NULL where only keypoints are wanted (sift.cc:516).  options NULL = the defaults.
 * *num_features_out: the number of features found; above capacity the call fails with DSM_ERR_OUT_OF_RANGE, nothing is written
 * to the outputs and the count is still valid.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): NULL where data is needed, an empty image, row_stride < width, options that
 *   SiftExtractionOptions::Check (sift.cc:218-234) rejects (max_num_features, octave_resolution, peak_threshold, edge_threshold,
 *   dsp_min_scale or dsp_num_scales not positive, dsp_max_scale < dsp_min_scale), an unknown normalization,
 *   estimate_affine_shape != 0.
 * DSM_ERR_OUT_OF_RANGE:
 *   - an image the reference aborts on.  With last = floor(log2(min(width - 1, height - 1) / 15)) the scale space holds the
 *     octaves first_octave .. last.  The reference needs last >= first_octave (vl_scalespace_new_with_geometry asserts a valid
 *     geometry) and, for a negative first_octave, last >= 0 (the upsampling chain of _vl_scalespace_start_octave_from_image
 *     starts at octave 0: the assertion at scalespace.c:396).  So: min(width, height) - 1 < 15 * 2^max(first_octave, 0) is
 *     refused -- a 12 x 40 image at first_octave = -1, any image under 16 pixels on a side;
 *   - first_octave outside -4 .. 16, octave_resolution above 64, dsp_num_scales above 64, a first octave of 2^31 samples or
 *     more over its levels, a scale space whose scratch exceeds dsm_ctx_set_memory_budget (the stage does not tile). */
int dsm_extract_covariant_sift(dsm_ctx* ctx, const dsm_covariant_sift_options* options, const uint8_t* gray_u8, uint32_t width,
                               uint32_t height, uint32_t row_stride, uint32_t capacity, float* keypoints_out,
                               uint8_t* descriptors_out, uint32_t* num_features_out);

/* ExtractCovariantSiftFeaturesCPU with every option: dsm_extract_covariant_sift's arguments, outputs and errors, except that
 * estimate_affine_shape is honoured (src/feature/sift.cc:467-473).  With the option and without upright,
 * vl_covdet_extract_affine_shape (lib/VLFeat/covdet.c:2462-2668) runs in the place of vl_covdet_extract_orientations: every
 * feature's frame is adapted to the second-moment matrix of its 41 x 41 patch in at most 14 passes and then rotated so that
 * the y axis keeps its direction; no feature is dropped or copied, and the orientation scores keep their detection value, 0.
 * With the option at 0, or with upright, the call returns exactly what dsm_extract_covariant_sift returns.  DESIGN.md 27. */
int dsm_extract_covariant_sift_affine(dsm_ctx* ctx, const dsm_covariant_sift_options* options, const uint8_t* gray_u8,
                                      uint32_t width, uint32_t height, uint32_t row_stride, uint32_t capacity, float* keypoints_out,
                                      uint8_t* descriptors_out, uint32_t* num_features_out);

/* The shape adaptation of the last successful dsm_extract_covariant_sift_affine on this context: *rounds = the launches of the
 * moment kernel (at most DSM_AFFINE_SHAPE_MAX_ROUNDS); exits = the features that left vl_covdet_extract_affine_shape_for_frame
 * as diverged (anisotropy above 5), at the iteration limit, with a zero moment, and converged, in that order -- they sum to the
 * features after the suppression; active[r] = the features whose moments round r computed, 0 from *rounds on.  All zero where
 * the call ran no adaptation (the option at 0, upright, no feature).  Any pointer may be NULL.
 * DSM_ERR_NOT_READY before such a call. */
#define DSM_AFFINE_SHAPE_MAX_ROUNDS 14
int dsm_get_affine_shape_stats(dsm_ctx* ctx, uint32_t* rounds, uint32_t exits[4], uint32_t active[DSM_AFFINE_SHAPE_MAX_ROUNDS]);

/* The features of the last successful dsm_extract_covariant_sift or dsm_extract_covariant_sift_affine on this context, in
 * output order, as a test compares them (the final bytes hide differences below 1 / 512): octave_scale [n x 2] = VlCovDetFeature's (o, s), scores [n x 3] = peakScore, edgeScore,
 * orientationScore, raw_descriptors [n x num_scales x 128] = vl_sift_calc_raw_descriptor's floats of every pooling scale, in
 * VLFeat's bin order, before the pooling (num_scales = dsp_num_scales, or 1 without domain_size_pooling).  Any of the three
 * may be NULL.  *n_out: the count; above capacity DSM_ERR_OUT_OF_RANGE and nothing is written.
 * DSM_ERR_NOT_READY before the first successful call, and for raw_descriptors after a call without descriptors_out. */
int dsm_get_covariant_sift_raw(dsm_ctx* ctx, uint32_t capacity, int32_t* octave_scale, float* scores, float* raw_descriptors,
                               uint32_t* n_out);

/* HIP-event times of the last dsm_extract_covariant_sift or dsm_extract_covariant_sift_affine on this context, in ms: 0 the
 * scale space (load, up- / downsampling, every smoothing of every octave), 1 detection (DoG, extremum test, compaction,
 * refinement, summed over the octaves), 2 what stands at sift.cc:467-473: the orientations, or the shape adaptation's moment
 * kernel summed over its rounds, 3 descriptors (patch, gradient and raw descriptor of every (feature, pooling scale)), 4 pooling,
 * normalisation and bytes.  DSM_ERR_NOT_READY before the first call. */
#define DSM_COVARIANT_SIFT_STAGES 5
int dsm_get_covariant_sift_time(dsm_ctx* ctx, double* stage_ms);

/* ---- image and reconstruction undistortion ----
 * image_undistorter / COLMAPUndistorter's numerical work: UndistortCamera (src/base/undistortion.cc:659-842), the point loop of
 * UndistortReconstruction (:869-879), UndistortImage -> WarpImageBetweenCameras and the two homography warps
 * (src/base/warp.cc:51-172) with Bitmap::InterpolateBilinear (src/util/bitmap.cc:225-281) and BitmapColor<float>::Cast<uint8_t>
 * (src/util/bitmap.h:217-243).  DESIGN.md 22.  All eleven camera models, both directions, bit for bit the CPU path's.
 *
 * NOT covered: the Bitmap::Rescale that ends WarpImageBetweenCameras and WarpImageWithHomographyBetweenCameras when the target
 * camera's size differs from the source's (warp.cc:92-95, 168-171).  It is FreeImage_Rescale; the device delivers the warp at
 * the source resolution (warp.cc:58-90, 133-166) and reports that the caller's Bitmap::Rescale(target.width, target.height)
 * is still owed.  Image decoding and writing, RectifyStereoCameras (the caller passes H), the exporters' text files: the host's. */
typedef struct dsm_undistort_options { /* UndistortCameraOptions, src/base/undistortion.h:41-62 */
  double blank_pixels;    /* 0.0 */
  double min_scale;       /* 0.2 */
  double max_scale;       /* 2.0 */
  int32_t max_image_size; /* -1 */
  int32_t reserved;
  double roi_min_x;       /* 0.0 */
  double roi_min_y;       /* 0.0 */
  double roi_max_x;       /* 1.0 */
  double roi_max_y;       /* 1.0 */
} dsm_undistort_options;

void dsm_default_undistort_options(dsm_undistort_options* o);

/* UndistortCamera (undistortion.cc:659-842) for n cameras, host pointers; options NULL = the defaults.  out_cameras[i] is the
 * PINHOLE camera (model 1, no prior focal length) of cameras[i]: the focal lengths copied by the number of focal indices
 * (:679-688), the ROI arithmetic (:695-726), the border scan (:729-777) on the device for all cameras in one launch, the scalar
 * tail (:779-839) with Camera::Rescale(scale) (camera.cc:228-247) on the host in the reference's order, std::min / std::max /
 * Clip with the reference's argument order (a NaN scale clips to min_scale).
 * Invalid (DSM_ERR_INVALID_ARGUMENT, out_cameras untouched): every CHECK of :661-671 (blank_pixels outside [0, 1], min_scale
 * <= 0 or > max_scale, max_image_size == 0, a ROI outside [0, 1] or empty; a NaN fails them as it fails the CHECKs), an unknown
 * model, a camera without pixels or with a side above 2^30, 2^31 border pixels or more in one batch. */
int dsm_undistort_cameras(dsm_ctx* ctx, const dsm_undistort_options* options, uint32_t n, const dsm_camera* cameras,
                          dsm_camera* out_cameras);

/* The loop of UndistortReconstruction (undistortion.cc:869-879) over all 2D points of all images, host pointers:
 * xy[i] <- undistorted_cameras[c].WorldToImage(cameras[c].ImageToWorld(xy[i])) with c = camera_index[i], in place, xy
 * [n_points x 2].  n_points = 0 is a valid call.
 * Invalid (xy untouched): NULL where data is needed, an unknown model, a camera index >= n_cameras. */
int dsm_undistort_points2D(dsm_ctx* ctx, uint32_t n_cameras, const dsm_camera* cameras, const dsm_camera* undistorted_cameras,
                           uint64_t n_points, const uint32_t* camera_index, double* xy);

/* The warps of src/base/warp.cc for a batch of n_images images of one source camera and size, host pointers.  Images are rows
 * top-down of interleaved bytes, channels = 1 (grey) or 3 (the channels are independent: their byte order is the caller's);
 * image k starts at src + k * src_image_stride, its row y at + y * src_row_stride (dst likewise).  The image size is the
 * source camera's (the reference CHECKs that they agree, warp.cc:54-55).
 *   H == NULL                     WarpImageBetweenCameras (:51-90), up to but not including the Rescale of :92-95: the target
 *                                 camera is rescaled to the source size (Camera::Rescale(width, height), camera.cc:249-267)
 *                                 when the sizes differ; per target pixel ImageToWorld of the scaled target at (x + 0.5, y + 0.5),
 *                                 WorldToImage of the source, the bilinear sample at (sx - 0.5, sy - 0.5).
 *   H, both cameras               WarpImageWithHomographyBetweenCameras (:124-166) as written: H * (x + 0.5, y + 0.5, 1),
 *                                 hnormalized, ImageToWorld of the UNSCALED target_camera (:154), WorldToImage of the source.
 *   H, a size-only source camera  WarpImageWithHomography (:98-122).  The reference takes no camera there; the sizes come in
 *                                 cameras whose model_id is DSM_CAMERA_SIZE_ONLY and of which only width and height are read:
 *                                 source_camera the source image's, target_camera the target image's (NULL: the source's).
 * H is row-major; each row of H * p is summed left to right (Eigen fixes no order for it).
 * dst receives the warp at the SOURCE resolution in the two camera modes (dst images are source-sized), at the target size in
 * the third.  *out_scaled_target_camera (may be NULL): the target camera rescaled to the source size (a copy where the sizes
 * agree).  *out_needs_rescale (may be NULL): 1 when the reference would now call Bitmap::Rescale(target_camera.width,
 * target_camera.height) -- the caller's to do with FreeImage -- else 0.  out_source_xy (may be NULL): [height x width x 2]
 * doubles, the source point (sx, sy) of every target pixel before the - 0.5, so that a wrong map can be told from a wrong sample.
 * A source coordinate that is NaN or whose floor lies outside int writes 0 (the reference's cast is undefined there).
 * A batch that does not fit dsm_ctx_set_memory_budget is cut into chunks of images (one image always runs).
 * Invalid (dst and the outputs untouched): channels other than 1 or 3, a row stride below width * channels, an image stride
 * below row stride * height (n_images > 1), an unknown model, a camera without pixels or with a side above 2^30, H without
 * target_camera for a real source camera, a size-only source camera without H or with a real target camera. */
#define DSM_CAMERA_SIZE_ONLY (-1)
int dsm_warp_images(dsm_ctx* ctx, const dsm_camera* source_camera, const dsm_camera* target_camera, const double* H,
                    uint32_t n_images, uint32_t channels, const uint8_t* src, uint64_t src_row_stride, uint64_t src_image_stride,
                    uint8_t* dst, uint64_t dst_row_stride, uint64_t dst_image_stride, dsm_camera* out_scaled_target_camera,
                    int32_t* out_needs_rescale, double* out_source_xy);

/* HIP-event times in ms of the last call of each kind on this context: 0 the border scan of dsm_undistort_cameras, 1 the kernel of
 * dsm_undistort_points2D, and of dsm_warp_images, summed over its chunks, 2 the upload, 3 the warp kernel, 4 the download.
 * DSM_ERR_NOT_READY before the first of these calls. */
#define DSM_UNDISTORTION_STAGES 5
int dsm_get_undistortion_time(dsm_ctx* ctx, double* stage_ms);

/* ---- training the vocabulary tree (vocab_tree_builder, VisualIndex::Build, src/retrieval/visual_index.h:510-536) ----
 * The two numerical steps of Build, DESIGN.md 23: Quantize (:623-665) = flann::hierarchicalClustering<L2<uint8_t>> with
 * KMEANSPP seeding -- the WHOLE k-means tree (lib/FLANN/algorithms/kmeans_index.h:329-345, 496-530, 544-713), then
 * getMinVarianceClusters (:928-969) and std::round -- and InvertedIndex::ComputeHammingEmbedding (inverted_index.h:184-217).
 * Not covered: flann::AutotunedIndex::buildIndex over the words (it decides by wall-clock timings), the Gaussian + QR
 * projection (GenerateHammingEmbeddingProjection, Eigen), writing the vocabulary file: the host's. */
typedef struct dsm_vocabulary_build_options { /* VisualIndex::BuildOptions, visual_index.h:99-118 */
  int32_t num_visual_words;   /* 65536 */
  int32_t branching;          /* 256; 2 .. 4096 */
  int32_t num_iterations;     /* 11; negative: until convergence, as FLANN reads it */
  int32_t workgroup_node_max; /* scheduling only, never the result: a node of at most this many points is clustered by one
                                 workgroup (nodes whose draws are known beforehand in batches), a larger one by the whole
                                 chip, a launch per phase.  0: the default, max(2 * branching - 2, 256) */
} dsm_vocabulary_build_options;
void dsm_default_vocabulary_build_options(dsm_vocabulary_build_options* o);

/* VisualIndex::Quantize of n x 128 uint8 descriptors (host memory); options NULL = the defaults.  *num_words_out receives the
 * number of centres the reference returns (<= num_visual_words: getMinVarianceClusters stops when the next split would pass
 * it), words [num_visual_words][128] its rounded centres in its order, centers (may be NULL) the float centres.
 * FLANN draws from the process's rand() (lib/FLANN/util/random.h:62-76); rand_fn(user) stands for it and is called on the host
 * in the reference's order -- `branching` times per clustered node, depth first -- NULL: rand() itself.  With the same stream
 * of draws the count, the order and every byte are the reference's.  rand() is the PROCESS's stream, as it is for the
 * reference: whatever else calls it between the caller's srand() and this call's draws shifts the result (seen on the first
 * vocabulary call of a process); a caller who needs srand(seed) to fix the words passes rand_fn, or calls once before seeding.
 * Invalid (DSM_ERR_INVALID_ARGUMENT): the reference's CHECKs -- num_visual_words < branching, n < num_visual_words, branching
 * < 2 -- and branching > 4096, n > 2^31 - 1, a negative workgroup_node_max, NULL where data is needed; num_iterations == 0
 * on a node of identical points, which then keeps all of them in one child for ever (the reference recurses until its stack
 * is gone; with an iteration the empty-cluster repair splits such a node).
 * DSM_ERR_OUT_OF_RANGE: the descriptors and the tree's state (about 144 bytes per descriptor) do not fit
 * dsm_ctx_set_memory_budget or the device's free memory.  The device memory of the call is released when it returns. */
int dsm_retrieval_quantize(dsm_ctx* ctx, const dsm_vocabulary_build_options* options, const uint8_t* descriptors, uint64_t n,
                           int (*rand_fn)(void*), void* user, uint32_t* num_words_out, uint8_t* words, float* centers);

/* Test hook: the k-means tree of the last dsm_retrieval_quantize, nodes in depth-first order (a node, then the subtrees of
 * its children in order).  first_child is -1 for a leaf; the other children are the later nodes with this parent, in order.
 * variance and radius are float bits.  pivots [nodes][128] floats (may be NULL), indices [n] the final permutation
 * (may be NULL).  *num_nodes (may be NULL) is set before the capacities are checked (DSM_ERR_OUT_OF_RANGE). */
typedef struct dsm_vocabulary_tree_node {
  int32_t parent, first_child, size;
  uint32_t variance_bits, radius_bits;
} dsm_vocabulary_tree_node;
int dsm_get_vocabulary_tree(dsm_ctx* ctx, uint32_t* num_nodes, dsm_vocabulary_tree_node* nodes, float* pivots, uint32_t node_capacity,
                            int32_t* indices, uint64_t indices_capacity);

/* InvertedIndex::ComputeHammingEmbedding (inverted_index.h:184-217, inverted_file.h:275-291) of n training descriptors, host
 * pointers: thresholds [num_words][64] = Median (util/math.h:211-229) of the word's projected descriptors per dimension,
 * has_embedding [num_words] = 1 where it was computed.  A word with fewer than 5 descriptors (kMinEntries) keeps zero
 * thresholds and flag 0.  projection [64][128] row-major is the caller's; each projected value is summed left to right in
 * float, as dsm_retrieval_index / _query sum it.  word_ids [n] (may be NULL): the caller's word of every descriptor, e.g. the
 * reference's FLANN answer; NULL: the exact nearest word, ties to the lower id, as dsm_retrieval_index assigns it.
 * Invalid: NULL where data is needed, num_words == 0, a word id outside the words. */
int dsm_retrieval_train_embedding(dsm_ctx* ctx, const uint8_t* descriptors, uint64_t n, const uint8_t* words, uint32_t num_words,
                                  const float* projection, const int32_t* word_ids, float* thresholds, uint8_t* has_embedding);

/* Times in ms of the last dsm_retrieval_quantize (0 seeding, 1 assignment -- and the whole kernel of the workgroup form --, 2
 * centre update, 3 statistics: the distances to the float centres and the root's chains, 4 partition: the host's swap
 * partition with its copies) and of the last dsm_retrieval_train_embedding (5).  HIP events, host clock for the host's
 * pieces.  DSM_ERR_NOT_READY before the first of these calls. */
#define DSM_VOCABULARY_BUILD_STAGES 6
int dsm_get_vocabulary_build_time(dsm_ctx* ctx, double* stage_ms);

/* ---- PatchMatch multi-view stereo (patch_match_stereo, PatchMatchCuda, src/mvs/patch_match_cuda.cu) ----
 * DESIGN.md 24.  The reference has this stage as CUDA only, built with fast math, hardware texture filtering and cuRAND; the
 * contract here is its algorithm operation for operation in IEEE float, with the points it leaves to the hardware fixed as
 * DESIGN.md 24 lists them (Philox4x32-10 draws, software bilinear sampling, fminf / fmaxf, the bilateral weight as a product of
 * two host tables, correctly rounded exp / sin / cos).  tests/patch_match_ref.py is the normative restatement; the device equals
 * it bit for bit.
 * NOT covered: source-image selection and depth ranges from the sparse model (the caller names both, as patch-match.cfg does),
 * max_image_size rescaling, image decoding, the Workspace cache and meshing: the host's. */
typedef struct dsm_patch_match_options { /* PatchMatchOptions, src/mvs/patch_match.h:59-139, ranges of Check() :141-168 */
  int32_t window_radius;                   /* 5; 1 .. 32 */
  int32_t window_step;                     /* 1; 1 .. 2 */
  int32_t num_samples;                     /* 15; > 0 */
  int32_t num_iterations;                  /* 5; > 0 */
  int32_t geom_consistency;                /* 1 */
  int32_t filter;                          /* 1 */
  int32_t filter_min_num_consistent;       /* 2; >= 0 */
  uint32_t seed;                           /* 0: the first word of the Philox key */
  double sigma_spatial;                    /* -1; <= 0: window_radius (patch_match.cc:454) */
  double sigma_color;                      /* 0.2f; > 0 */
  double ncc_sigma;                        /* 0.6f; > 0 */
  double min_triangulation_angle;          /* 1.0 degrees; [0, 180) */
  double incident_angle_sigma;             /* 0.9f; > 0 */
  double geom_consistency_regularizer;     /* 0.3f; >= 0 */
  double geom_consistency_max_cost;        /* 3.0; >= 0 */
  double filter_min_ncc;                   /* 0.1f; [-1, 1] */
  double filter_min_triangulation_angle;   /* 3.0 degrees; [0, 180] */
  double filter_geom_consistency_max_cost; /* 1.0; >= 0 */
} dsm_patch_match_options;
void dsm_default_patch_match_options(dsm_patch_match_options* o);

/* One image of the undistorted workspace (mvs::Image, src/mvs/image.h): grey bytes, rows top-down, row y at data + y *
 * row_stride; K, R row-major and T in float as mvs::Image holds them.  depth_map [height][width] and normal_map
 * [3][height][width] (the slice layout of Mat<float>) are read with geom_consistency only. */
typedef struct dsm_mvs_image {
  const uint8_t* data;
  uint64_t row_stride;
  uint32_t width, height;
  float K[9], R[9], T[3];
  uint32_t reserved;
  const float* depth_map;
  const float* normal_map;
} dsm_mvs_image;

/* PatchMatchCuda::Run for a batch of problems, host pointers; options NULL = the defaults.  Problem p has the reference image
 * ref_image[p], the source images src_images[src_offsets[p] .. src_offsets[p + 1]) (their order is the order of the slices S
 * of the outputs) and the depth range [depth_min[p], depth_max[p]].  The Philox key of a problem is (seed, ref_image[p]), so a
 * problem's bytes depend neither on its place in the batch nor on how the batch is cut.
 * With geom_consistency the depth and normal map of the reference image initialise the problem and the depth maps of the
 * source images enter the cost (InitWorkspaceMemory :1614-1656, InitSourceImages :1466-1497): both must be given for every
 * image a problem names.
 * Outputs, one pointer per problem: out_depth[p] [H][W], out_normal[p] [3][H][W], out_sel_prob[p] [S][H][W] (out_sel_prob or
 * an entry of it may be NULL), out_mask[p] [S][H][W] bytes (the consistency mask, written with filter only; out_mask may be
 * NULL).  H, W: the reference image's.
 * n_problems = 0 is a valid call that writes nothing.  A problem without source images is valid: no hypothesis has a cost, so
 * FindMinCost's `<=` keeps the last one (the perturbed depth with the current normal) in every sweep, and with filter and
 * filter_min_num_consistent > 0 every pixel is filtered to 0; its S-sliced outputs are empty.
 * The batch is cut into chunks of problems whose maps fit dsm_ctx_set_memory_budget (4 GiB without one; one problem always
 * runs); the image table is resident for the whole call.  The results do not depend on the cut.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): an option outside the range above (a NaN fails it), depth_min <= 0
 * or depth_min > depth_max, an image index out of range, an image without pixels or with a side above 32768, a row stride
 * below the width, NULL where data is needed. */
int dsm_patch_match(dsm_ctx* ctx, const dsm_patch_match_options* options, uint32_t n_images, const dsm_mvs_image* images,
                    uint32_t n_problems, const uint32_t* ref_image, const uint64_t* src_offsets, const uint32_t* src_images,
                    const float* depth_min, const float* depth_max, float* const* out_depth, float* const* out_normal,
                    float* const* out_sel_prob, uint8_t* const* out_mask);

/* HIP-event times in ms of the last dsm_patch_match, summed over its chunks: 0 upload (image table, tables, initial maps), 1
 * reference filter and initialisation, 2 initial cost, 3 sweeps, 4 rotation, 5 download.  DSM_ERR_NOT_READY before the first call. */
#define DSM_PATCH_MATCH_STAGES 6
int dsm_get_patch_match_time(dsm_ctx* ctx, double* stage_ms);

/* ---- Stereo fusion of depth and normal maps (stereo_fusion, StereoFusion, src/mvs/fusion.cc) ----
 * DESIGN.md 26.  StereoFusion::Run from "Reading configuration" onward (fusion.cc:169-293) with Fuse() (:295-473): the
 * fused points in the reference's order, each with the images that see it.  The contract is the reference's loop operation
 * for operation in IEEE float (matrix rows, the dot product and the squared norm summed left to right, no contraction);
 * tests/stereo_fusion_ref.py is the normative restatement and the device equals it bit for bit.  The device does not run
 * seed after seed: it traverses every pending seed of an image against the committed masks at once and commits, in rank
 * order, the seeds whose pixels nobody of a lower rank claims (DESIGN.md 26 shows why that is the sequential result).
 * Deviations: a point's visibility list is in ascending image index (the reference copies an unordered_set); P, inv_P and
 * inv_R are inputs; min_num_pixels < 1 is refused (the reference would CHECK-fail in Median); depths and normals must be
 * finite, and a NaN that arithmetic produces fails the test it enters and is never an index.
 * NOT covered: the Workspace (decoding, max_image_size, the cache), fusion.cfg, the PMVS vis.dat reader, check_num_images
 * and the overlap lists (an input, as patch-match.cfg's lists are), meshing: the host's. */
typedef struct dsm_stereo_fusion_options { /* StereoFusionOptions, src/mvs/fusion.h:55-85, ranges of Check() fusion.cc:98-108 */
  int32_t min_num_pixels;      /* 5; >= 1 (the reference: >= 0) and <= max_num_pixels */
  int32_t max_num_pixels;      /* 10000 */
  int32_t max_traversal_depth; /* 100; > 0 */
  int32_t lane_capacity;       /* 0 = the default: pixels and queue entries a seed's lane holds; scheduling only, >= 0 */
  double max_reproj_error;     /* 2.0f; >= 0 */
  double max_depth_error;      /* 0.01f; >= 0 */
  double max_normal_error;     /* 10.0f degrees; >= 0 */
} dsm_stereo_fusion_options;
void dsm_default_stereo_fusion_options(dsm_stereo_fusion_options* o);

/* One image of fusion.  used = 0: the image is in no fusion.cfg (its maps are not read; the reference holds a 0 x 0 map).
 * depth_map [height][width], normal_map [3][height][width] (the slice layout of Mat<float>), rgb: bitmap_height rows of
 * bitmap_width RGB byte triples, row y at rgb + y * row_stride.  P, inv_P (3 x 4) and inv_R (3 x 3) row-major as
 * fusion.cc:220-235 composes them (capi.fusion_matrices does so by the ruling of DESIGN.md 24), bitmap_scale = (width /
 * bitmap_width, height / bitmap_height) in float (:216-218). */
typedef struct dsm_fusion_image {
  int32_t used;
  uint32_t width, height;
  uint32_t bitmap_width, bitmap_height;
  uint32_t reserved;
  uint64_t row_stride;
  const float* depth_map;
  const float* normal_map;
  const uint8_t* rgb;
  float P[12], inv_P[12], inv_R[9], bitmap_scale[2];
  uint32_t reserved2;
} dsm_fusion_image;

typedef struct dsm_fused_point { /* PlyPoint, src/util/ply.h:45-55 */
  float x, y, z, nx, ny, nz;
  uint8_t r, g, b, reserved;
} dsm_fused_point;

/* StereoFusion::Run (fusion.cc:169-293), host pointers; options NULL = the defaults.  overlapping_images_[i] is
 * overlap_images[overlap_offsets[i] .. overlap_offsets[i + 1]).  *n_points gets the number of fused points; the points stay
 * in the context for dsm_get_fused_points.
 * The maps, masks and claims of all used images are resident on the device for the call (depth 4, normal 12, mask 1, claim 4 bytes
 * per pixel and the bitmaps) next to the lanes' storage; a call that does not fit dsm_ctx_set_memory_budget (when one is set) or the free
 * memory, or has 2^31 pixels or more, is refused with DSM_ERR_OUT_OF_RANGE.  There is no cache emulation.
 * n_images = 0 and "no image used" are valid and give 0 points.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): an option outside its range (a NaN fails it), an overlap index out
 * of range or equal to its own image, a used image without pixels or with a side above 32768 (maps or bitmap), a row stride
 * below 3 x bitmap_width, a depth or normal that is not finite, NULL where data is needed. */
int dsm_fuse_stereo(dsm_ctx* ctx, const dsm_stereo_fusion_options* options, uint32_t n_images, const dsm_fusion_image* images,
                    const uint64_t* overlap_offsets, const uint32_t* overlap_images, uint64_t* n_points);
/* The points of the last dsm_fuse_stereo in the reference's order (fused_points_) and their visibility
 * (fused_points_visibility_): vis_offsets gets n_points + 1 prefix offsets, vis_images the image indices, ascending per
 * point.  Same conventions as dsm_get_matches: any pointer may be NULL, the capacities are in points and in indices. */
int dsm_get_fused_points(dsm_ctx* ctx, dsm_fused_point* points, uint64_t capacity, uint64_t* vis_offsets, uint32_t* vis_images,
                         uint64_t vis_capacity);
/* Times in ms of the last dsm_fuse_stereo (HIP events, host clock around the host's pieces): 0 upload, 1 traversal, 2 claims
 * and commit decisions, 3 medians (the commit kernel), 4 download (scan, gather and copy); 5 the number of rounds, 6 the
 * number of seed traversals.  DSM_ERR_NOT_READY before the first call. */
#define DSM_STEREO_FUSION_STAGES 7
int dsm_get_stereo_fusion_time(dsm_ctx* ctx, double* stage_ms);
/* Per image of the last dsm_fuse_stereo: its place in the order of FindNextImage (fusion.cc:58-79; 0 for an image the loop
 * never reached) and the rounds it took (0 for an image without pixels).  Either pointer may be NULL; capacity in images. */
int dsm_get_stereo_fusion_rounds(dsm_ctx* ctx, uint32_t* order_pos, uint32_t* rounds, uint32_t capacity);

/* ---- Source images and depth ranges of PatchMatch's problems (mvs::Model, src/mvs/model.cc) ----
 * DESIGN.md 28.  The queries of mvs::Model that turn a sparse model into patch_match's problems, in one call:
 * GetMaxOverlappingImages (model.cc:119-169) with ReadProblems' condition on the candidates (src/mvs/patch_match.cc:349),
 * ComputeDepthRanges (:176-216), ComputeSharedPoints (:218-233) and ComputeTriangulationAngles (:235-274) with
 * ComputeProjectionCenter (src/mvs/image.cc:125-130), CalculateTriangulationAngle (src/base/triangulation.cc:122-145), DegToRad
 * and Percentile (src/util/math.h:194-200, 231-246).  The contract is the reference's operations in its evaluation order
 * (entries Eigen leaves open summed left to right, no contraction) with the correctly rounded acos (csrc/exact_acos.h);
 * tests/source_selection_ref.py is the normative restatement and the device equals it bit for bit.
 * Rulings: equal counts go to the lower image index (the reference's sorts leave them open); an item whose acos argument left
 * [-1, 1] has the angle NaN, which orders above every number and fails `>=` (the reference's behaviour there is unspecified).
 * At most 65536 images (DSM_ERR_OUT_OF_RANGE beyond). */
typedef struct dsm_source_selection_options {
  int32_t max_num_src_images;           /* 20: patch-match.cfg's `__auto__, 20` (src/base/undistortion.cc:243); >= 0 */
  float triangulation_angle_percentile; /* 75 (model.cc:127, patch_match.cc:333); in [0, 100] */
  double min_triangulation_angle;       /* 1.0 degrees (PatchMatchOptions, src/mvs/patch_match.h); fusion passes 0 */
} dsm_source_selection_options;
void dsm_default_source_selection_options(dsm_source_selection_options* o);

typedef struct dsm_image_overlap { /* one entry of ComputeSharedPoints and ComputeTriangulationAngles: a < b */
  uint32_t a, b, count;
  float angle; /* the percentile element of the pair's angles, radians */
} dsm_image_overlap;

/* Host pointers; options NULL = the defaults.  R [n_images][9] row-major and T [n_images][3] as in dsm_mvs_image, xyz
 * [n_points][3], the track of point p = track_images[track_offsets[p] .. track_offsets[p + 1]) (an image may repeat: every
 * repeat counts, as in the reference).  candidate_mask NULL: Model::GetMaxOverlappingImages; else [n_images] bytes, and only
 * images with a non-zero byte may be chosen as sources (ReadProblems' ref_image_idxs.count, patch_match.cc:349).
 * depth_ranges gets [n_images][2] = ComputeDepthRanges' (first, second), (-1, -1) for an image without a positive depth;
 * *n_list_entries and *n_pairs (either may be NULL) the sizes for dsm_get_source_images and dsm_get_image_overlap.
 * Every pair of elements of every track is one item of 8 bytes, sorted on the device; a call whose items and tables do not fit
 * dsm_ctx_set_memory_budget (when one is set) or the free device memory is refused with DSM_ERR_OUT_OF_RANGE and a message
 * that names the need and the budget -- never a partial result.  n_images = 0 and n_points = 0 are valid.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): max_num_src_images < 0, a percentile outside [0, 100], a NaN angle,
 * offsets that do not start at 0 or decrease, an image index out of range, NULL where data is needed. */
int dsm_select_source_images(dsm_ctx* ctx, const dsm_source_selection_options* options, uint32_t n_images, const float* R, const float* T,
                             uint64_t n_points, const float* xyz, const uint64_t* track_offsets, const uint32_t* track_images,
                             const uint8_t* candidate_mask, float* depth_ranges, uint64_t* n_list_entries, uint64_t* n_pairs);
/* The lists of the last dsm_select_source_images: list_offsets gets n_images + 1 prefix offsets, list_images the source
 * images of every image, most shared points first.  Either pointer may be NULL; capacity in indices. */
int dsm_get_source_images(dsm_ctx* ctx, uint64_t* list_offsets, uint32_t* list_images, uint64_t capacity);
/* The pair table of the last dsm_select_source_images in ascending (a, b): what ComputeSharedPoints and
 * ComputeTriangulationAngles return for both directions of a pair (patch_match.cc:330-335 calls them directly). */
int dsm_get_image_overlap(dsm_ctx* ctx, dsm_image_overlap* pairs, uint64_t capacity);
/* HIP-event times in ms of the last dsm_select_source_images: 0 upload, 1 depths (kernel, sort, ranges), 2 items (count, scan,
 * angles), 3 the sort of the items, 4 pair statistics and selection, 5 download; then the counts 6 items (pairs of track
 * elements with different images), 7 pairs, 8 nan_items.  DSM_ERR_NOT_READY before the first call. */
#define DSM_SOURCE_SELECTION_STAGES 9
int dsm_get_source_selection_time(dsm_ctx* ctx, double* stage_ms);

/* ---- The initial image pair of a batch of reconstructions (IncrementalMapper, src/sfm/incremental_mapper.cc) ----
 * DESIGN.md 29.  What brings up a cluster's reconstruction, for many clusters (problems) over one scene in one call:
 * FindInitialImagePair (incremental_mapper.cc:146-200) with FindFirstInitialImage / FindSecondInitialImage (:791-930),
 * EstimateInitialTwoViewGeometry (:1121-1176) = TwoViewGeometry::EstimateCalibrated + EstimateRelativePose
 * (src/estimators/two_view_geometry.cc:292-380, 169-230), and the two-view triangulation of RegisterInitialImagePair
 * (:289-339).  A problem sees the pairs whose two images are both in its subset: the per-cluster DatabaseCache of
 * src/controllers/distributed_mapper_controller.cpp:688-702.
 *   Rulings: the first images run in (prior focal length first, NumCorrespondences descending, image id
 *   ascending), the second images of a first image in (prior focal length first, correspondences with the first descending,
 *   image id ascending) -- the reference iterates unordered maps and sorts unstably, so its ties are open; a first image needs
 *   more than 0 correspondences in the problem, init_num_reg_trials < init_max_reg_trials and num_registrations == 0, a second
 *   image num_registrations == 0 and at least init_min_num_inliers correspondences with the first; the counts are the matches
 *   a pair keeps after the duplicate rule of CorrespondenceGraph::AddCorrespondences (dsm_retriangulate's), an image's
 *   NumCorrespondences their sum over its pairs in the problem; the candidates are the directed pairs in that nested order,
 *   every undirected pair once (its first occurrence), without the input tried set; with one seed image the first list is
 *   that image alone (:152-164, no test of the first image), with both the single pair (seed_image1, seed_image2) whatever
 *   the tried set says (the controller's direct RegisterInitialImagePair); a candidate's matches are
 *   FindCorrespondencesBetweenImages(id1, id2): ascending point2D index of image 1, oriented as found; EstimateCalibrated is
 *   forced (both cameras count as having a prior) with TwoViewGeometry::Options' defaults, min_num_trials 30 and max_error
 *   init_max_error, on a fresh MT19937 stream per candidate seeded with dsm_pair_seed(id1, id2, user_seed) -- the reference
 *   continues a thread-local stream; EstimateRelativePose: UNDEFINED, DEGENERATE and WATERMARK fail, the pose comes from E for
 *   CALIBRATED / UNCALIBRATED and from H otherwise, tri_angle = Median(CalculateTriangulationAngles(0, -R^T t, points3D))
 *   (src/base/triangulation.cc:147-181, Median of src/util/math.h:211-229), 0 without a point in front of both cameras, R the
 *   rotation matrix of the returned qvec; accepted (:1166-1169) with inliers >= init_min_num_inliers, |tvec.z| <
 *   init_max_forward_motion and tri_angle > DegToRad(init_min_tri_angle); the triangulation has image 1 at the identity and
 *   image 2's projection matrix and centre through its quaternion (ComposeProjectionMatrix(qvec, tvec),
 *   ProjectionCenterFromPose), per correspondence ImageToWorld twice, TriangulatePoint, CalculateTriangulationAngle >= the
 *   minimum and HasPointPositiveDepth for both, the survivors in correspondence order.
 * The candidates of all unfinished problems are verified speculation_window at a time; the first accepted candidate in list
 * order wins, and candidates behind it were speculated: they are counted and do not enter the tried list.  No result depends
 * on speculation_window, the batch, the memory budget or the order of the problems. */
typedef struct dsm_initial_pair_options {
  int32_t init_min_num_inliers;   /* 100  (IncrementalMapper::Options, src/sfm/incremental_mapper.h:68-81); >= 0 */
  int32_t init_max_reg_trials;    /* 2; >= 1 */
  double init_max_error;          /* 4.0 pixels; > 0 */
  double init_max_forward_motion; /* 0.95; in [0, 1] */
  double init_min_tri_angle;      /* 16.0 degrees; >= 0 */
  uint32_t user_seed;             /* 0 */
  uint32_t speculation_window;    /* 64; candidates per problem and round; scheduling only, never the result; >= 1 */
} dsm_initial_pair_options;
void dsm_default_initial_pair_options(dsm_initial_pair_options* o);

#define DSM_NO_IMAGE 0xFFFFFFFFu /* kInvalidImageId: no seed image, no pair found */
enum { DSM_INITIAL_PAIR_NONE = 0, DSM_INITIAL_PAIR_FOUND = 1 };

typedef struct dsm_initial_pair_result { /* one per problem */
  int32_t status;                /* DSM_INITIAL_PAIR_* */
  uint32_t image_id1, image_id2; /* in the order the search found them; DSM_NO_IMAGE without a pair (:196-197) */
  uint32_t num_tried;            /* pairs tried in this call, the successful one included */
  uint64_t num_points;           /* points the triangulation kept */
  dsm_two_view_geometry two_view_geometry; /* prev_init_two_view_geometry_ of the pair found, tri_angle as EstimateRelativePose
                                              computes it; zero without a pair.  Its inlier matches: inlier_matches. */
} dsm_initial_pair_result;

typedef struct dsm_initial_pair_report {
  uint32_t num_rounds;        /* speculation rounds */
  uint32_t num_batches;       /* verifier calls: more than num_rounds where the memory budget cut a round by problems */
  uint64_t num_candidates;    /* candidates of all problems' lists */
  uint64_t num_verified;      /* candidates that went through the verifier */
  uint64_t num_speculated;    /* of those, behind their problem's success */
  /* the smallest relative margin of every decision rounding could flip (INFINITY when never taken), over the candidates up to
     and including each problem's success: tri_angle against its threshold, |tvec.z| against init_max_forward_motion; over
     the correspondences of the pairs found: the angle gate and the two depths */
  double min_tri_angle_margin, min_forward_motion_margin, min_point_angle_margin, min_point_depth_margin;
  double setup_ms;            /* host validation, the problems' pair lists (host clock) */
  double graph_ms;            /* HIP events: uploads, the duplicate rule, the counts, the candidate order */
  double gather_ms, verify_ms, pose_ms; /* HIP events summed over the batches: match lists, the verifier, k_ip_relative_pose */
  double triangulate_ms;      /* HIP events: k_ip_triangulate and the download of the points */
  double device_ms;           /* HIP events: first upload to the last download */
} dsm_initial_pair_report;

/* Host pointers, the conventions of dsm_retriangulate.
 *   cameras: camera_ids[num_cameras] (unique), cameras (the eleven models)
 *   images: image_ids[num_images] (unique, none DSM_NO_IMAGE), image_camera_ids, points2D_offsets[num_images + 1] (<= 262144 per
 *     image), points2D_xy (2 per point2D)
 *   pairs, in load order: pair_image_ids (2 per pair), match_offsets[num_pairs + 1] (uint64), matches (idx1, idx2 per match):
 *     what DatabaseCache::Load kept (src/base/database_cache.cc); min_num_matches and the watermark filter stay with the host
 *   problems: problem_image_offsets[num_problems + 1] (CSR, as dsm_align_clusters takes clusters), problem_image_ids;
 *     num_registrations and init_num_reg_trials aligned with problem_image_ids (NULL: zeros); tried_offsets[num_problems + 1]
 *     (uint64) and tried_pairs (2 image ids per pair, either order; init_image_pairs_), both NULL: none; seed_image1 and
 *     seed_image2 [num_problems] (DSM_NO_IMAGE = none), NULL: none
 * Outputs: results[num_problems]; tried_out_offsets[num_problems + 1] and tried_out_pairs (2 ids per pair, as tried, in trial
 *   order, the successful pair last) with room for tried_capacity pairs -- the pairs of the problems' subsets bound it;
 *   point_offsets[num_problems + 1], point_xyz (3 each) and point_obs (point2D_idx1, point2D_idx2) in correspondence order with
 *   room for point_capacity points -- the sum over the problems of the largest match count of a pair bounds it;
 *   inlier_offsets[num_problems + 1] and inlier_matches (point2D_idx1, point2D_idx2): the inlier matches of the geometry of
 *   the pair found, with room for inlier_capacity matches (the same bound).  A capacity that is too small is
 *   DSM_ERR_OUT_OF_RANGE.  tried_out_pairs, point_xyz, point_obs, inlier_offsets and inlier_matches may be NULL (nothing is
 *   written and no capacity is needed), report may be NULL, options NULL = the defaults.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): what dsm_retriangulate refuses of these arguments; a problem image
 *   that is not an image of the scene; a repeated image inside a problem; a seed image outside its problem, or twice the same;
 *   options out of range.  More than 2^20 problem images or 2^19 kept matches of one pair is DSM_ERR_OUT_OF_RANGE. */
int dsm_find_initial_pairs(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                           uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                           const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                           const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                           uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                           const uint32_t* num_registrations, const uint32_t* init_num_reg_trials, const uint64_t* tried_offsets,
                           const uint32_t* tried_pairs, const uint32_t* seed_image1, const uint32_t* seed_image2,
                           const dsm_initial_pair_options* options, dsm_initial_pair_result* results,
                           uint64_t* tried_out_offsets, uint32_t* tried_out_pairs, uint64_t tried_capacity,
                           uint64_t* point_offsets, double* point_xyz, uint32_t* point_obs, uint64_t point_capacity,
                           uint64_t* inlier_offsets, uint32_t* inlier_matches, uint64_t inlier_capacity,
                           dsm_initial_pair_report* report);

/* ---- the next images of a batch of reconstructions: IncrementalMapper::FindNextImages ----
 * src/sfm/incremental_mapper.cc:202-256 with the ranks of :46-73, over the state the reference keeps incrementally in
 * Image::Increment / DecrementCorrespondenceHasPoint3D (src/base/image.cc:113-137) and VisibilityPyramid
 * (src/base/visibility_pyramid.cc:53-106), recomputed here from the scene arrays: the call is stateless.
 *   A slot is one (problem, image) incidence in the order of problem_image_ids.  A problem sees the pairs whose two images are
 *   both in it; correspondences are the matches a pair keeps after the duplicate rule of
 *   CorrespondenceGraph::AddCorrespondences.  A point2D of a slot is visible when at least one of its correspondences in the
 *   problem ends on an observation that has a point in that problem; NumVisiblePoints3D counts the visible points2D,
 *   NumObservations the points2D with at least one correspondence in the problem.  The visibility score is the six-level
 *   pyramid's over the visible points2D: cell cx = Clip(size_t(64 * x / width), 0, 63) in double in that order (cy alike, with
 *   the camera's width and height), level l = 0 .. 5 has the cells (cx >> (5 - l), cy >> (5 - l)), score = the sum over the
 *   levels of occupied cells * 4^(l + 1).  An image is eligible when it is not registered, NumVisiblePoints3D >=
 *   abs_pose_min_num_inliers and num_reg_trials < max_reg_trials; the first bucket holds the eligible images that are not
 *   filtered and have num_reg_trials == 0, the second the rest; each bucket is sorted by the reference's float rank
 *   descending, then by image id ascending (the reference's unstable sort of an unordered map's content leaves ties open).
 * No result depends on the order of the problems, of the pairs, of the matches of a pair none of which is a duplicate, on the
 * batch or on the memory budget. */
enum { DSM_NEXT_IMAGE_MAX_VISIBLE_POINTS_NUM = 0, DSM_NEXT_IMAGE_MAX_VISIBLE_POINTS_RATIO = 1, DSM_NEXT_IMAGE_MIN_UNCERTAINTY = 2 };

typedef struct dsm_next_images_options {
  int32_t image_selection_method;   /* 2 = MIN_UNCERTAINTY (IncrementalMapper::Options, src/sfm/incremental_mapper.h:87-131); 0 .. 2 */
  int32_t abs_pose_min_num_inliers; /* 30; > 0 */
  int32_t max_reg_trials;           /* 3; >= 1 */
} dsm_next_images_options;
void dsm_default_next_images_options(dsm_next_images_options* o);

typedef struct dsm_next_images_report {
  uint64_t num_eligible;      /* images in the lists of all problems */
  uint64_t num_first_bucket;  /* of those: not filtered and never tried */
  uint64_t num_second_bucket; /* the rest */
  uint32_t num_batches;       /* more than 1 where the memory budget cut the call by problems */
  double setup_ms;            /* host validation, the problems' pair lists (host clock) */
  double graph_ms;            /* HIP events: the scene's uploads and the duplicate rule */
  double visibility_ms;       /* HIP events summed over the batches: the state's upload and the bitmaps */
  double score_ms;            /* the counts, the pyramid scores and the keys */
  double rank_ms;             /* the placement and the downloads */
  double device_ms;           /* HIP events: first upload to the last download */
} dsm_next_images_report;

/* Host pointers; cameras, images, pairs and problems as dsm_find_initial_pairs takes them (width and height of a camera feed
 * the pyramid).  Per slot: slot_registered (0 / 1), slot_obs_offsets[num_slots + 1] (uint64; must equal the running sum of the
 * images' point2D counts: the caller's layout is checked, not guessed), slot_num_reg_trials and slot_filtered (NULL: zeros).
 * Per observation: slot_obs_point3D, an index into the problem's points or -1.
 * Outputs: next_offsets[num_problems + 1] and next_image_ids with room for next_capacity ids (the unregistered slots bound it;
 *   too small: DSM_ERR_OUT_OF_RANGE, nothing written); slot_num_visible, slot_num_observations and slot_score [num_slots] may
 *   each be NULL (slot_score is 0 for a registered slot: only a candidate's pyramid is evaluated); report may be NULL,
 *   options NULL = the defaults.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): what dsm_find_initial_pairs refuses of these arguments; a
 *   slot_registered other than 0 / 1; slot_obs_offsets that are not that running sum; a point index below -1; an observation
 *   with a point on a slot that is not registered (the reference CHECKs it); negative points2D coordinates, or a camera
 *   without width or height, on an image of a slot that is not registered; options out of range.  More than 2^31
 *   observations over all slots is DSM_ERR_OUT_OF_RANGE. */
int dsm_find_next_images(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                         uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                         const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                         const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                         uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                         const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                         const uint32_t* slot_num_reg_trials, const uint8_t* slot_filtered,
                         const dsm_next_images_options* options, uint64_t* next_offsets, uint32_t* next_image_ids,
                         uint64_t next_capacity, uint32_t* slot_num_visible, uint32_t* slot_num_observations,
                         uint64_t* slot_score, dsm_next_images_report* report);

/* ---- the local bundles of a batch of registered images: IncrementalMapper::FindLocalBundle ----
 * src/sfm/incremental_mapper.cc:932-1099 with CalculateTriangulationAngles (src/base/triangulation.cc:147-181) and Percentile
 * (src/util/math.h:231-246), stateless over the observations' points.
 *   A point's track is the set of observations of its problem that reference it.  The shared count of another image is the
 *   number of (query point2D with a point, track element on that image) incidences as the reference's loop counts them: a
 *   point referenced by two points2D of the query counts twice, and so do two track elements on the same other image.  The
 *   overlapping images are sorted by shared count descending, then image id ascending (the reference's unstable sort of an
 *   unordered map's content leaves ties open).  No more of them than local_ba_num_images - 1: they are the answer in that
 *   order, no angle is computed.  Otherwise the eight thresholds of :1001-1010 apply as written there -- the doubles
 *   0.6 * NumPoints3D etc. against the count converted to double, NumPoints3D the query's points2D with a point, the inner
 *   loop breaking at the first image below the overlap threshold -- then the fill-up in overlap order.  tri_angle is
 *   Percentile(CalculateTriangulationAngles(centre(query), centre(other), the xyz of every query point2D with a point, in
 *   point2D order, repeats included), 75): the reference's text, not its comment -- it depends on the other image through its
 *   projection centre only.  Centres are ProjectionCenterFromPose as dsm_find_initial_pairs evaluates it, the angle uses
 *   the correctly rounded acos, Percentile's index is round(75.0 / 100 * (n - 1)) clamped to 0 .. n - 1; a NaN angle orders
 *   behind every number.  Which angles get computed is scheduling: the device computes them for every overlapping image at
 *   or above the loosest overlap threshold (0.1 * NumPoints3D) of a query that enters the chain. */
typedef struct dsm_local_bundle_selection_options {
  int32_t local_ba_num_images;   /* 6 (IncrementalMapper::Options, src/sfm/incremental_mapper.h:98-102); >= 2 */
  double local_ba_min_tri_angle; /* 6.0 degrees; >= 0 and finite */
} dsm_local_bundle_selection_options;
void dsm_default_local_bundle_selection_options(dsm_local_bundle_selection_options* o);

typedef struct dsm_local_bundle_selection_report {
  uint64_t num_copied;         /* queries answered by the copy path (:983-988) */
  uint64_t num_chained;        /* queries that went through the thresholds */
  uint64_t num_angles;         /* tri_angles computed on the device */
  uint64_t num_filled;         /* images taken by the fill-up (:1080-1096) */
  double min_tri_angle_margin; /* the smallest |tri_angle - threshold| / max(threshold, DBL_EPSILON) over the comparisons the
                                  chains made; INFINITY when none was made */
  uint32_t num_batches;        /* more than 1 where the memory budget cut the call by queries */
  double setup_ms;             /* host validation (host clock) */
  double tracks_ms;            /* HIP events: uploads, the centres, the inversion of the observations into tracks */
  double overlap_ms;           /* summed over the batches: the shared counts and the sorted overlap lists */
  double angles_ms;            /* the angles and their percentiles */
  double device_ms;            /* HIP events: first upload to the last download */
} dsm_local_bundle_selection_report;

/* Host pointers.  Images (image_ids, points2D_offsets), problems and the per-slot / per-observation state as
 * dsm_find_next_images takes them; FindLocalBundle reads no camera, no pair and no point2D coordinate, so none is passed.
 *   slot_qvec (4 per slot), slot_tvec (3 per slot): read for registered slots only
 *   points: point_offsets[num_problems + 1] (uint64, CSR over the problems), point_xyz (3 per point); slot_obs_point3D indexes
 *     its problem's points
 *   queries: query_problem[num_queries], query_image_id[num_queries]; a query image must be registered in its problem
 * Outputs: bundle_offsets[num_queries + 1] and bundle_image_ids with room for bundle_capacity ids (num_queries *
 *   (local_ba_num_images - 1) bounds it); optionally (all four or none) the overlap lists: overlap_offsets[num_queries + 1],
 *   overlap_image_ids, overlap_shared (the counts) and overlap_tri_angle (-1 for a candidate no threshold could reach, and for
 *   every candidate of a query on the copy path) with room for overlap_capacity entries (the sum over the queries of their
 *   problem's images less one bounds it).  A capacity that is too small is DSM_ERR_OUT_OF_RANGE and nothing is written.
 *   report may be NULL, options NULL = the defaults.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): what dsm_find_next_images refuses of these arguments; a point index
 *   outside its problem's points; a non-finite pose of a registered slot or point; a query on an unknown problem, or on an
 *   image that is not in the problem or not registered there; options out of range.  More than 2^31 observations or points is
 *   DSM_ERR_OUT_OF_RANGE. */
int dsm_find_local_bundles(dsm_ctx* ctx, uint32_t num_images, const uint32_t* image_ids, const uint32_t* points2D_offsets,
                           uint32_t num_problems, const uint32_t* problem_image_offsets, const uint32_t* problem_image_ids,
                           const uint8_t* slot_registered, const uint64_t* slot_obs_offsets, const int32_t* slot_obs_point3D,
                           const double* slot_qvec, const double* slot_tvec, const uint64_t* point_offsets, const double* point_xyz,
                           uint32_t num_queries, const uint32_t* query_problem, const uint32_t* query_image_id,
                           const dsm_local_bundle_selection_options* options, uint64_t* bundle_offsets, uint32_t* bundle_image_ids,
                           uint64_t bundle_capacity, uint64_t* overlap_offsets, uint32_t* overlap_image_ids, uint32_t* overlap_shared,
                           double* overlap_tri_angle, uint64_t overlap_capacity, dsm_local_bundle_selection_report* report);

/* ------------------------------------------------------------------ completing and merging tracks
 * IncrementalTriangulator::CompleteTracks / CompleteAllTracks and MergeTracks / MergeAllTracks
 * (src/sfm/incremental_triangulator.cc:231-287, Merge :588-677, Complete :679-746, Reconstruction::MergePoints3D
 * reconstruction.cc:215-241): what IncrementalMapper::AdjustLocalBundle runs after every local bundle adjustment (MERGE then
 * COMPLETE over one id set) and IterativeGlobalRefinement before every global one (CompleteAndMergeTracks: COMPLETE then MERGE
 * over all points).  The correspondence graph is dsm_retriangulate's; the reprojection error is dsm_filter_points3D's
 * (CalculateSquaredReprojectionError by qvec / tvec, DBL_MAX below a depth of epsilon).  CompleteImage is dsm_complete_images
 * (below), which takes the same scene and runs these steps first.
 *   Rulings: points run in ascending point3D id (the reference: unordered sets); a step without a selection
 *   takes a snapshot of the ids at its start; a merged point gets the id AddPoint3D would hand out from next_point3D_id, in
 *   the order of the merge events of the sequential run (an intermediate merged point that is merged again consumes one),
 *   however the device schedules the components; the camera verdict of HasBogusParams is computed per camera, not cached across
 *   calls; a selected id merged away earlier in the call is skipped (ExistsPoint3D), merged ids are never selected. */
typedef struct dsm_track_update_options {
  dsm_triangulation_options tri;       /* dsm_update_tracks reads the three bogus-parameter limits only; dsm_complete_images also
                                          min_angle, ignore_two_view_tracks, ransac_confidence, ransac_max_num_trials, max_transitivity */
  double  complete_max_reproj_error;   /* 4.0 px */
  double  merge_max_reproj_error;      /* 4.0 px */
  int32_t complete_max_transitivity;   /* 5; < 1 is DSM_ERR_INVALID_ARGUMENT */
  int32_t reserved;
} dsm_track_update_options;

enum { DSM_TRACKS_MERGE = 0, DSM_TRACKS_COMPLETE = 1 };

typedef struct dsm_track_update_report {
  uint32_t num_points;                 /* input points */
  uint32_t num_steps;
  uint32_t complete_rounds;            /* claim rounds, summed over the COMPLETE steps */
  uint32_t complete_serial_steps;      /* COMPLETE steps finished by the serial form (claim pool exhausted, or asked for) */
  uint32_t num_components;             /* of the last MERGE step: components holding a selected point, and the largest one */
  uint32_t largest_component;          /*   (in selected points) */
  uint64_t num_correspondences;        /* directed entries of the correspondence graph */
  uint64_t complete_trials;            /* reprojection tests of Complete, as the sequential run takes them */
  uint64_t merge_trials;               /* pairs Merge enters into merge_trials_ */
  uint64_t num_completed, num_merged;  /* the step counts, summed per kind */
  uint64_t num_merge_events;           /* MergePoints3D calls = ids handed out */
  /* the smallest relative margin |a - t| / max(|a|, |t|) of every decision taken (INFINITY when never taken): err^2 against
     the squared threshold in Complete (speculative walks of the claim rounds included) and in Merge, the depth against
     epsilon, the bogus ratios against their bounds */
  double min_complete_error_margin, min_merge_error_margin, min_depth_margin, min_bogus_margin;
  double setup_ms;                     /* host validation, slot order, the tracks as lists (host clock) */
  double graph_ms;                     /* uploads and the correspondence graph (host clock around the synchronised phase, as all below) */
  double complete_ms;                  /* the COMPLETE steps */
  double components_ms, schedule_ms, merge_ms; /* MERGE steps: labelling, the per-component lists (host), the runs and the ids */
  double download_ms;                  /* the tracks written out and brought back */
  double device_ms;                    /* first upload to the last download */
} dsm_track_update_report;

void dsm_default_track_update_options(dsm_track_update_options* o);

/* The steps in order over one state, which stays on the device between them (host pointers).  Cameras, images, points2D and
 * pairs as dsm_retriangulate_pairs takes them, without points2D_point3D: feature -> point follows from the tracks.
 *   points3D: point3D_ids (unique), point3D_xyz (3 each), track_offsets[num_points3D + 1], track_obs ((image_id, point2D_idx)
 *     per element, in track order)
 *   steps[num_steps]: DSM_TRACKS_MERGE / DSM_TRACKS_COMPLETE; selected_ids[num_selected]: the id set every step runs over
 *     (NULL: all points, a snapshot per step); next_point3D_id: the first merged id; 0 = the largest existing id + 1
 * Outputs in ascending id: *out_num_points, out_point_ids, out_xyz (3 each), out_track_offsets[n + 1], out_track_obs
 *   ((image_id, point2D_idx); room for the input's elements plus every point2D, i.e. at most T = points2D_offsets[num_images]
 *   entries are written), out_modified with *out_num_modified (modified_point3D_ids_ as these steps change it, starting
 *   empty: inserted on a completion; on a merge the two inputs erased and the merged id inserted), step_counts[num_steps]
 *   (num_merged / num_completed as the reference returns them).  The point arrays need room for num_points3D entries.
 *   Output arrays other than the counts may be NULL.  report may be NULL.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): what dsm_retriangulate refuses of these arguments; a track element
 *   on an unknown or unregistered image or out of range; a feature in two tracks; complete_max_transitivity < 1; a negative
 *   or non-finite threshold; an unknown step; a selected id that is no point3D, or repeated.
 * The result is the same bytes for any order of the points3D and of the matches inside a pair (when no match of the pair is
 * dropped as a duplicate). */
int dsm_update_tracks(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
                      uint32_t num_images, const uint32_t* image_ids, const uint32_t* image_camera_ids,
                      const uint8_t* image_registered, const double* image_qvec, const double* image_tvec,
                      const uint32_t* points2D_offsets, const double* points2D_xy, uint32_t num_pairs,
                      const uint32_t* pair_image_ids, const uint64_t* match_offsets, const uint32_t* matches,
                      uint32_t num_points3D, const uint64_t* point3D_ids, const double* point3D_xyz,
                      const uint64_t* track_offsets, const uint32_t* track_obs, uint32_t num_steps, const int32_t* steps,
                      uint64_t num_selected, const uint64_t* selected_ids, uint64_t next_point3D_id,
                      const dsm_track_update_options* options, uint64_t* out_num_points, uint64_t* out_point_ids,
                      double* out_xyz, uint64_t* out_track_offsets, uint32_t* out_track_obs, uint64_t* out_num_modified,
                      uint64_t* out_modified, uint64_t* step_counts, dsm_track_update_report* report);

/* ------------------------------------------------------------------ completing an image's observations
 * IncrementalTriangulator::CompleteImage (src/sfm/incremental_triangulator.cc:119-229), the last call of
 * IncrementalMapper::AdjustLocalBundle's tail (MergeTracks, CompleteTracks, CompleteImage): in point2D order over one state, a
 * point2D with a point runs Complete(point) (dsm_update_tracks's walk), one without runs Find at transitivity 1,
 * EstimateTriangulation with REPROJECTION_ERROR residuals (LORANSAC, CombinationSampler, InlierSupportMeasurer; the
 * projection-matrix overload of CalculateSquaredReprojectionError) and AddPoint3D of the inliers.
 *   Rulings: the listed images run in the given order; RANSACOptions::min_num_trials is carried from one point2D
 *   to the next inside an image as the reference carries it (assigned C(n, 2) only where the list holds n <= 15 entries, 0 at
 *   the start of every image); new ids continue the counter the steps' merge events draw from, in the order of the sequential
 *   run; ransac_confidence and ransac_max_num_trials are read from the options (the reference: 0.9999 and 10000). */
typedef struct dsm_complete_images_report {
  uint32_t num_images;                 /* listed images */
  uint32_t num_rounds;                 /* ordered commit passes over the items (one per call that has items) */
  uint64_t num_items;                  /* (listed image, point2D) items of the registered images on passing cameras */
  uint64_t num_estimated_ahead;        /* creating candidates whose estimate ran ahead of the commit pass, a lane each */
  uint64_t num_serial_items;           /* creating items whose estimate ran on the commit lane: no room in the estimate pool, a carried
                                          min_num_trials other than the predicted one, or the serial form asked for */
  uint64_t complete_trials;            /* reprojection tests of Complete, the steps' included */
  uint64_t ransac_trials;              /* LORANSAC trials of the estimates the sequential run takes */
  uint64_t num_new_points, num_new_observations;   /* AddPoint3D calls and their track elements */
  uint64_t num_completed_observations; /* what the Complete walks of the images added */
  /* the smallest relative margin of every decision taken (INFINITY when never taken; estimates that ran ahead and were not
     used are included): the squared reprojection residual against max_error^2, equal-count support sums against each other,
     the triangulation angle against min_angle, depths against epsilon, Complete's squared error against its threshold, the
     bogus ratios against their bounds */
  double min_residual_margin, min_support_margin, min_angle_margin, min_depth_margin, min_complete_error_margin, min_bogus_margin;
  double estimate_ms;                  /* the candidates, their lists and the estimates that run ahead (host clock, synchronised) */
  double commit_ms;                    /* the ordered pass: the Complete walks, the creations, the remaining estimates */
  double device_ms;                    /* first upload to the last download, the steps included */
  dsm_track_update_report steps;       /* the report of the steps (its download_ms and device_ms cover the whole call) */
} dsm_complete_images_report;

/* dsm_update_tracks's arguments (scene, state, steps -- there may be none --, selection, next_point3D_id, options), then
 * complete_image_ids[num_complete_images] (unique): the steps run first, then CompleteImage for every listed image in the
 * given order, all over one device-resident state.  An unregistered image or one on a camera with bogus parameters
 * contributes 0.  complete_max_reproj_error is Complete's threshold and the RANSAC max_error; complete_max_transitivity is
 * read by the Complete walks only.
 * Outputs as dsm_update_tracks, with new points: the point arrays need room for num_points3D plus the points2D of the listed
 *   images; image_num_tris[num_complete_images] is what CompleteImage returns per image.  report may be NULL.
 * Invalid (DSM_ERR_INVALID_ARGUMENT, outputs untouched): what dsm_update_tracks refuses; an unknown or repeated image id in
 *   complete_image_ids; tri.max_transitivity != 1; ransac_max_num_trials < 1; a confidence outside (0, 1); a negative or
 *   non-finite min_angle.  A correspondence list of more than 8192 entries is DSM_ERR_OUT_OF_RANGE. */
int dsm_complete_images(dsm_ctx* ctx, uint32_t num_cameras, const uint32_t* camera_ids, const dsm_camera* cameras,
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
                        dsm_complete_images_report* report);

void dsm_default_match_options(dsm_match_options* o);
void dsm_default_two_view_options(dsm_two_view_options* o);

#ifdef __cplusplus
}
#endif
#endif /* DAGSFM_MI355X_H_ */
