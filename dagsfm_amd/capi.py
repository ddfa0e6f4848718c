"""ctypes binding of the C-ABI in include/dagsfm_mi355x.h (no torch types cross it)."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSM_LIB_PATH: developer override (e.g. the -DDSM_PROFILE_SECTIONS build under dagsfm_amd/prof/)
LIB_PATH = os.environ.get("DSM_LIB_PATH") or os.path.join(_HERE, "libdagsfm_mi355x.so")
# the same sources with -DDSM_CHECK_BUILD: the product plus the cross-check schedules (csrc/ctx.h, csrc/Makefile).  Only
# tools/ and the schedule-parametrised tests load it -- Context(check=True), or any check-only DSM_* variable in the process
# environment when the context is created; everything else, bench.py and the shim included, runs the product library.
CHECK_LIB_PATH = os.environ.get("DSM_CHECK_LIB_PATH") or os.path.join(_HERE, "libdagsfm_mi355x_check.so")

# the RCCL companion (include/dagsfm_gather.h): multi-GPU assembly of the match graph below the host language
GATHER_LIB_PATH = os.path.join(_HERE, "libdagsfm_gather.so")

u8p = ctypes.POINTER(ctypes.c_uint8)
u32p = ctypes.POINTER(ctypes.c_uint32)
u64p = ctypes.POINTER(ctypes.c_uint64)
f32p = ctypes.POINTER(ctypes.c_float)


class DsmError(RuntimeError):
    pass


class MatchOptions(ctypes.Structure):
    """SiftMatchingOptions (matching half), /root/reference/src/feature/sift.h:116-165."""
    _fields_ = [("max_ratio", ctypes.c_double), ("max_distance", ctypes.c_double),
                ("cross_check", ctypes.c_int32), ("max_num_matches", ctypes.c_int32)]


class TwoViewOptions(ctypes.Structure):
    """TwoViewGeometry::Options + RANSACOptions, two_view_geometry.h:105-157, ransac.h:47-72."""
    _fields_ = [("min_num_inliers", ctypes.c_uint64), ("min_E_F_inlier_ratio", ctypes.c_double),
                ("max_H_inlier_ratio", ctypes.c_double), ("watermark_min_inlier_ratio", ctypes.c_double),
                ("watermark_border_size", ctypes.c_double), ("detect_watermark", ctypes.c_int32),
                ("multiple_models", ctypes.c_int32), ("max_error", ctypes.c_double),
                ("min_inlier_ratio", ctypes.c_double), ("confidence", ctypes.c_double),
                ("min_num_trials", ctypes.c_uint64), ("max_num_trials", ctypes.c_uint64),
                ("multiple_ignore_watermark", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class Camera(ctypes.Structure):
    _fields_ = [("model_id", ctypes.c_int32), ("has_prior_focal_length", ctypes.c_int32),
                ("width", ctypes.c_uint64), ("height", ctypes.c_uint64), ("params", ctypes.c_double * 12)]


class TwoViewGeometry(ctypes.Structure):
    _fields_ = [("config", ctypes.c_int32), ("num_inliers", ctypes.c_uint32), ("num_matches", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("F", ctypes.c_double * 9), ("E", ctypes.c_double * 9),
                ("H", ctypes.c_double * 9), ("qvec", ctypes.c_double * 4), ("tvec", ctypes.c_double * 3),
                ("tri_angle", ctypes.c_double), ("num_trials", ctypes.c_uint32 * 4),
                ("num_models", ctypes.c_uint32 * 4)]


class DeviceInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 128), ("arch", ctypes.c_char * 64), ("compute_units", ctypes.c_int32),
                ("clock_khz", ctypes.c_int32), ("memory_clock_khz", ctypes.c_int32), ("memory_bus_bits", ctypes.c_int32),
                ("total_memory", ctypes.c_uint64), ("l2_bytes", ctypes.c_int32), ("lds_per_cu", ctypes.c_int32)]


class Vocabulary(ctypes.Structure):
    """dsm_vocabulary: visual words, Hamming-embedding projection and per-word thresholds (visual_index.h / inverted_index.h)."""
    _fields_ = [("num_words", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("words", ctypes.c_void_p),
                ("projection", ctypes.c_void_p), ("thresholds", ctypes.c_void_p)]


_libs = {}


RA_MAX_L1_ITERATIONS = 8  # DSM_RA_MAX_L1_ITERATIONS
DSM_ERR_INVALID_ARGUMENT = 1
DSM_ERR_NOT_CONVERGED = 6


class RotationAveragingOptions(ctypes.Structure):
    """dsm_rotation_averaging_options: RobustRotationEstimator::Options + L1Solver::Options defaults
    (/root/reference/src/rotation_estimation/robust_rotation_estimator.h:96-115, src/solver/l1_solver.h)."""
    _fields_ = [("max_num_l1_iterations", ctypes.c_int32), ("max_num_irls_iterations", ctypes.c_int32),
                ("l1_step_convergence_threshold", ctypes.c_double), ("irls_step_convergence_threshold", ctypes.c_double),
                ("irls_loss_parameter_sigma", ctypes.c_double), ("admm_initial_max_iterations", ctypes.c_int32),
                ("max_num_cg_iterations", ctypes.c_int32), ("cg_batch_iterations", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("admm_rho", ctypes.c_double), ("admm_alpha", ctypes.c_double), ("admm_absolute_tolerance", ctypes.c_double),
                ("admm_relative_tolerance", ctypes.c_double), ("max_relative_rotation_difference_degrees", ctypes.c_double),
                ("cg_tolerance", ctypes.c_double), ("cg_max_residual", ctypes.c_double)]


class RotationAveragingReport(ctypes.Structure):
    _fields_ = [("num_components", ctypes.c_uint32), ("num_images", ctypes.c_uint32), ("num_edges", ctypes.c_uint32),
                ("num_l1_iterations", ctypes.c_uint32), ("admm_iterations", ctypes.c_uint32 * RA_MAX_L1_ITERATIONS),
                ("num_irls_iterations", ctypes.c_uint32), ("num_filtered_edges", ctypes.c_uint32), ("num_final_images", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("total_cg_iterations", ctypes.c_uint64), ("max_cg_relative_residual", ctypes.c_double),
                ("last_l1_step", ctypes.c_double), ("last_irls_step", ctypes.c_double), ("device_ms", ctypes.c_double)]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("admm_iterations", "reserved")}
        d["admm_iterations"] = list(self.admm_iterations)[:self.num_l1_iterations]
        return d


NLR_TRACE_COLUMNS = 6  # DSM_NLR_TRACE_COLUMNS: cost, radius, rho, CG iterations, accepted, gradient max-norm


class NonlinearRotationOptions(ctypes.Structure):
    """dsm_nonlinear_rotation_options: NonlinearRotationEstimator (/root/reference/src/rotation_estimation/
    nonlinear_rotation_estimator.h:86, .cpp:123-125) and ceres::Solver::Options defaults."""
    _fields_ = [("robust_loss_width", ctypes.c_double), ("max_num_iterations", ctypes.c_int32),
                ("max_num_consecutive_invalid_steps", ctypes.c_int32), ("function_tolerance", ctypes.c_double),
                ("gradient_tolerance", ctypes.c_double), ("parameter_tolerance", ctypes.c_double),
                ("initial_trust_region_radius", ctypes.c_double), ("max_trust_region_radius", ctypes.c_double),
                ("min_relative_decrease", ctypes.c_double), ("min_lm_diagonal", ctypes.c_double), ("max_lm_diagonal", ctypes.c_double),
                ("max_num_cg_iterations", ctypes.c_int32), ("reserved", ctypes.c_int32), ("cg_tolerance", ctypes.c_double),
                ("cg_max_residual", ctypes.c_double), ("max_relative_rotation_difference_degrees", ctypes.c_double)]


class NonlinearRotationReport(ctypes.Structure):
    _fields_ = [("num_components", ctypes.c_uint32), ("num_images", ctypes.c_uint32), ("num_edges", ctypes.c_uint32),
                ("termination", ctypes.c_int32), ("num_iterations", ctypes.c_uint32), ("num_successful_steps", ctypes.c_uint32),
                ("num_rejected_steps", ctypes.c_uint32), ("num_invalid_steps", ctypes.c_uint32), ("num_filtered_edges", ctypes.c_uint32),
                ("num_final_images", ctypes.c_uint32), ("total_cg_iterations", ctypes.c_uint64),
                ("num_kernel_launches", ctypes.c_uint64), ("initial_cost", ctypes.c_double),
                ("final_cost", ctypes.c_double), ("final_trust_region_radius", ctypes.c_double),
                ("max_cg_relative_residual", ctypes.c_double), ("min_rho_margin", ctypes.c_double),
                ("min_gradient_margin", ctypes.c_double), ("min_function_margin", ctypes.c_double), ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ClusteringOptions(ctypes.Structure):
    """dsm_clustering_options: ImageClustering::Options defaults (src/clustering/image_clustering.h:126-132)
    and Spectra's compute() stopping rule."""
    _fields_ = [("num_images_ub", ctypes.c_uint32), ("image_overlap", ctypes.c_uint32), ("completeness_ratio", ctypes.c_float),
                ("expand", ctypes.c_int32), ("max_kmeans_iterations", ctypes.c_uint32), ("max_eigen_iterations", ctypes.c_int32),
                ("eigen_tolerance", ctypes.c_double)]


class ClusteringReport(ctypes.Structure):
    _fields_ = [("num_images", ctypes.c_uint32), ("num_edges", ctypes.c_uint32), ("num_clusters", ctypes.c_uint32),
                ("num_lost_edges", ctypes.c_uint32), ("num_readded_edges", ctypes.c_uint32), ("eigen_iterations", ctypes.c_uint32),
                ("kmeans_iterations", ctypes.c_uint32), ("ncv", ctypes.c_uint32), ("clustered_images_num", ctypes.c_uint64),
                ("clustered_edges_num", ctypes.c_uint64), ("operator_applications", ctypes.c_uint64),
                ("max_eigen_residual", ctypes.c_double), ("max_eigen_residual_ratio", ctypes.c_double), ("eigen_gap", ctypes.c_double),
                ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AlignOptions(ctypes.Structure):
    """dsm_align_options: AlignOptions / RansacSimilarity defaults (src/controllers/sfm_aligner.h,
    src/estimators/ransac_similarity.h:206-245) and the per-direction seed."""
    _fields_ = [("threshold", ctypes.c_double), ("max_reprojection_error", ctypes.c_double),
                ("failure_probability", ctypes.c_double), ("min_iterations", ctypes.c_int32), ("max_iterations", ctypes.c_int32),
                ("random_seed", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class AlignReport(ctypes.Structure):
    _fields_ = [("num_clusters", ctypes.c_uint32), ("num_pairs", ctypes.c_uint32), ("num_edges", ctypes.c_uint32),
                ("num_in_component", ctypes.c_uint32), ("num_prosac_problems", ctypes.c_uint32), ("num_separators", ctypes.c_uint32),
                ("num_observations", ctypes.c_uint64), ("num_correspondences", ctypes.c_uint64), ("prosac_iterations", ctypes.c_uint64),
                ("min_residual_margin", ctypes.c_double), ("min_cost_margin", ctypes.c_double), ("min_weight_margin", ctypes.c_double),
                ("device_ms", ctypes.c_double), ("join_ms", ctypes.c_double), ("prosac_ms", ctypes.c_double), ("refit_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class BundleAdjustmentOptions(ctypes.Structure):
    """dsm_bundle_adjustment_options: GlobalBundleAdjustment() / BundleAdjustmentOptions defaults
    (src/optim/bundle_adjustment.h:70-90, 522-542)."""
    _fields_ = [("max_num_iterations", ctypes.c_int32), ("max_linear_solver_iterations", ctypes.c_int32),
                ("gradient_tolerance", ctypes.c_double), ("function_tolerance", ctypes.c_double),
                ("parameter_tolerance", ctypes.c_double), ("max_num_consecutive_invalid_steps", ctypes.c_int32),
                ("refine_focal_length", ctypes.c_int32), ("refine_principal_point", ctypes.c_int32),
                ("refine_extra_params", ctypes.c_int32)]


class BundleAdjustmentReport(ctypes.Structure):
    _fields_ = [("termination", ctypes.c_int32), ("num_iterations", ctypes.c_int32), ("num_successful_steps", ctypes.c_int32),
                ("num_invalid_steps", ctypes.c_int32), ("num_residuals", ctypes.c_uint64),
                ("num_effective_parameters", ctypes.c_uint64), ("total_cg_iterations", ctypes.c_uint64),
                ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("initial_mean_reprojection_error", ctypes.c_double), ("final_mean_reprojection_error", ctypes.c_double),
                ("min_rho_margin", ctypes.c_double), ("min_cg_margin", ctypes.c_double), ("min_gradient_margin", ctypes.c_double),
                ("setup_ms", ctypes.c_double), ("jacobian_ms", ctypes.c_double), ("cg_ms", ctypes.c_double),
                ("candidate_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TriangulationOptions(ctypes.Structure):
    """dsm_triangulation_options: IncrementalTriangulator::Options and Create()'s RANSAC settings
    (src/sfm/incremental_triangulator.h, incremental_triangulator.cc:497-514)."""
    _fields_ = [("create_max_angle_error", ctypes.c_double), ("continue_max_angle_error", ctypes.c_double),
                ("min_angle", ctypes.c_double), ("min_focal_length_ratio", ctypes.c_double),
                ("max_focal_length_ratio", ctypes.c_double), ("max_extra_param", ctypes.c_double),
                ("ransac_confidence", ctypes.c_double), ("ransac_min_inlier_ratio", ctypes.c_double),
                ("ransac_max_num_trials", ctypes.c_int32), ("ignore_two_view_tracks", ctypes.c_int32),
                ("max_transitivity", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class TrackUpdateOptions(ctypes.Structure):
    """dsm_track_update_options: of `tri` dsm_update_tracks reads the three bogus-parameter limits only; dsm_complete_images also
    min_angle, ignore_two_view_tracks, ransac_confidence, ransac_max_num_trials and max_transitivity (which must be 1)."""
    _fields_ = [("tri", TriangulationOptions), ("complete_max_reproj_error", ctypes.c_double),
                ("merge_max_reproj_error", ctypes.c_double), ("complete_max_transitivity", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class TrackUpdateReport(ctypes.Structure):
    _fields_ = [("num_points", ctypes.c_uint32), ("num_steps", ctypes.c_uint32), ("complete_rounds", ctypes.c_uint32),
                ("complete_serial_steps", ctypes.c_uint32), ("num_components", ctypes.c_uint32), ("largest_component", ctypes.c_uint32),
                ("num_correspondences", ctypes.c_uint64), ("complete_trials", ctypes.c_uint64), ("merge_trials", ctypes.c_uint64),
                ("num_completed", ctypes.c_uint64), ("num_merged", ctypes.c_uint64), ("num_merge_events", ctypes.c_uint64),
                ("min_complete_error_margin", ctypes.c_double), ("min_merge_error_margin", ctypes.c_double),
                ("min_depth_margin", ctypes.c_double), ("min_bogus_margin", ctypes.c_double), ("setup_ms", ctypes.c_double),
                ("graph_ms", ctypes.c_double), ("complete_ms", ctypes.c_double), ("components_ms", ctypes.c_double),
                ("schedule_ms", ctypes.c_double), ("merge_ms", ctypes.c_double), ("download_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double)]


TRACKS_MERGE, TRACKS_COMPLETE = 0, 1  # DSM_TRACKS_*
_TRACK_UPDATE_ARGTYPES = ([ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 7
                          + [ctypes.c_uint32] + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 4
                          + [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                             ctypes.POINTER(TrackUpdateOptions)] + [ctypes.c_void_p] * 9)


class CompleteImagesReport(ctypes.Structure):
    """dsm_complete_images_report; `steps` is the report of the steps that ran first."""
    _fields_ = [("num_images", ctypes.c_uint32), ("num_rounds", ctypes.c_uint32), ("num_items", ctypes.c_uint64),
                ("num_estimated_ahead", ctypes.c_uint64), ("num_serial_items", ctypes.c_uint64), ("complete_trials", ctypes.c_uint64),
                ("ransac_trials", ctypes.c_uint64), ("num_new_points", ctypes.c_uint64), ("num_new_observations", ctypes.c_uint64),
                ("num_completed_observations", ctypes.c_uint64), ("min_residual_margin", ctypes.c_double),
                ("min_support_margin", ctypes.c_double), ("min_angle_margin", ctypes.c_double), ("min_depth_margin", ctypes.c_double),
                ("min_complete_error_margin", ctypes.c_double), ("min_bogus_margin", ctypes.c_double), ("estimate_ms", ctypes.c_double),
                ("commit_ms", ctypes.c_double), ("device_ms", ctypes.c_double), ("steps", TrackUpdateReport)]


# dsm_complete_images: dsm_update_tracks's arguments with the image list before the options and image_num_tris before the report
_COMPLETE_IMAGES_ARGTYPES = (_TRACK_UPDATE_ARGTYPES[:25] + [ctypes.c_uint32, ctypes.c_void_p] + _TRACK_UPDATE_ARGTYPES[25:-1]
                             + [ctypes.c_void_p, ctypes.c_void_p])


class TriangulationReport(ctypes.Structure):
    _fields_ = [("num_separators", ctypes.c_uint32), ("num_rounds", ctypes.c_uint32), ("num_problems", ctypes.c_uint64),
                ("num_deferred", ctypes.c_uint64), ("num_correspondences", ctypes.c_uint64), ("ransac_trials", ctypes.c_uint64),
                ("num_tris", ctypes.c_uint64), ("num_new_points", ctypes.c_uint64), ("num_new_observations", ctypes.c_uint64),
                ("num_continued", ctypes.c_uint64), ("min_residual_margin", ctypes.c_double), ("min_support_margin", ctypes.c_double),
                ("min_angle_margin", ctypes.c_double), ("min_depth_margin", ctypes.c_double), ("min_continue_margin", ctypes.c_double),
                ("min_bogus_margin", ctypes.c_double), ("setup_ms", ctypes.c_double), ("graph_ms", ctypes.c_double),
                ("continue_ms", ctypes.c_double), ("ransac_ms", ctypes.c_double), ("schedule_ms", ctypes.c_double),
                ("apply_ms", ctypes.c_double), ("round_gap_ms", ctypes.c_double), ("download_ms", ctypes.c_double),
                ("assemble_ms", ctypes.c_double), ("replay_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class PairRetriangulationOptions(ctypes.Structure):
    """dsm_pair_retriangulation_options: the triangulation options plus Retriangulate's re_* settings
    (src/sfm/incremental_triangulator.h:65-73)."""
    _fields_ = [("tri", TriangulationOptions), ("re_max_angle_error", ctypes.c_double), ("re_min_ratio", ctypes.c_double),
                ("re_max_trials", ctypes.c_int32), ("reserved", ctypes.c_int32)]


PAIR_NOT_UNDER_RECONSTRUCTED, PAIR_CLOSED_BY_ITS_TURN, PAIR_UNREGISTERED, PAIR_TRIALS_EXHAUSTED, PAIR_BOGUS_CAMERA, PAIR_PROCESSED = range(6)


class PairRetriangulationReport(ctypes.Structure):
    _fields_ = [("num_candidates", ctypes.c_uint32), ("num_rounds", ctypes.c_uint32), ("num_pairs_by_status", ctypes.c_uint64 * 6),
                ("num_correspondences", ctypes.c_uint64), ("num_both", ctypes.c_uint64), ("num_continue_tried", ctypes.c_uint64),
                ("num_continue_taken", ctypes.c_uint64), ("num_two_view_skipped", ctypes.c_uint64),
                ("num_create_tried", ctypes.c_uint64), ("num_create_taken", ctypes.c_uint64), ("num_tris", ctypes.c_uint64),
                ("num_new_points", ctypes.c_uint64), ("num_continued", ctypes.c_uint64), ("min_residual_margin", ctypes.c_double),
                ("min_angle_margin", ctypes.c_double), ("min_depth_margin", ctypes.c_double), ("min_continue_margin", ctypes.c_double),
                ("min_bogus_margin", ctypes.c_double), ("setup_ms", ctypes.c_double), ("graph_ms", ctypes.c_double),
                ("schedule_ms", ctypes.c_double), ("rounds_ms", ctypes.c_double), ("gate_ms", ctypes.c_double), ("solve_ms", ctypes.c_double),
                ("round_gap_ms", ctypes.c_double), ("download_ms", ctypes.c_double), ("assemble_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if k == "num_pairs_by_status" else getattr(self, k)) for k, _ in self._fields_}


BA_CONVERGENCE, BA_NO_CONVERGENCE, BA_FAILURE = 0, 1, 2
BA_TRACE_COLUMNS = 6  # cost, radius, rho, CG iterations, accepted, gradient max-norm


# dsm_align_pair as a numpy record (the C layout: no padding beyond the explicit `reserved`)
ALIGN_PAIR_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("num_common_images", "<u4"), ("num_correspondences", "<u4"),
                             ("num_inliers", "<u4", (2,)), ("iterations", "<u4", (2,)), ("edge", "<i4"), ("reserved", "<u4"),
                             ("msd", "<f8", (2,)), ("weight", "<f8"), ("s", "<f8", (2,)), ("R", "<f8", (2, 9)), ("t", "<f8", (2, 3)),
                             ("prosac_cost", "<f8", (2,)), ("prosac_s", "<f8", (2,)), ("prosac_R", "<f8", (2, 9)),
                             ("prosac_t", "<f8", (2, 3))])


class AbsolutePoseOptions(ctypes.Structure):
    """dsm_absolute_pose_options: AbsolutePoseEstimationOptions with its RANSACOptions as IncrementalMapper::RegisterNextImage
    fills them (src/estimators/pose.h:51-77, src/sfm/incremental_mapper.cc:438-449)."""
    _fields_ = [("num_focal_length_samples", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("min_focal_length_ratio", ctypes.c_double), ("max_focal_length_ratio", ctypes.c_double),
                ("max_error", ctypes.c_double), ("min_inlier_ratio", ctypes.c_double), ("confidence", ctypes.c_double),
                ("min_num_trials", ctypes.c_uint64), ("max_num_trials", ctypes.c_uint64), ("random_seed", ctypes.c_uint32),
                ("reserved2", ctypes.c_uint32)]


class AbsolutePoseResult(ctypes.Structure):
    _fields_ = [("success", ctypes.c_int32), ("factor_index", ctypes.c_int32), ("num_inliers", ctypes.c_uint32),
                ("num_trials", ctypes.c_uint32), ("model_is_local", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("focal_length_factor", ctypes.c_double), ("proj_matrix", ctypes.c_double * 12), ("qvec", ctypes.c_double * 4),
                ("tvec", ctypes.c_double * 3), ("focal_params", ctypes.c_double * 2)]


ABSOLUTE_POSE_MARGINS = ("residual", "depth", "support_tie", "root_imag", "root_sign", "rank", "beta_sign", "error_choice", "determinant")


class AbsolutePoseReport(ctypes.Structure):
    _fields_ = [("num_problems", ctypes.c_uint32), ("num_factors", ctypes.c_uint32), ("num_runs", ctypes.c_uint64),
                ("num_trials", ctypes.c_uint64), ("num_models", ctypes.c_uint64), ("num_local_optimizations", ctypes.c_uint64),
                ("min_margin", ctypes.c_double * 9), ("setup_ms", ctypes.c_double), ("prepare_ms", ctypes.c_double),
                ("ransac_ms", ctypes.c_double), ("choice_ms", ctypes.c_double), ("device_ms", ctypes.c_double)]


class PoseRefinementOptions(ctypes.Structure):
    """dsm_pose_refinement_options: AbsolutePoseRefinementOptions (src/estimators/pose.h:80-104); the two refine flags are per
    problem (refine_flags)."""
    _fields_ = [("gradient_tolerance", ctypes.c_double), ("loss_function_scale", ctypes.c_double),
                ("max_num_iterations", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class PoseRefinementResult(ctypes.Structure):
    _fields_ = [("success", ctypes.c_int32), ("termination", ctypes.c_int32), ("num_iterations", ctypes.c_uint32),
                ("num_successful_steps", ctypes.c_uint32), ("num_invalid_steps", ctypes.c_uint32),
                ("num_residual_blocks", ctypes.c_uint32), ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("qvec", ctypes.c_double * 4), ("tvec", ctypes.c_double * 3), ("camera_params", ctypes.c_double * 12)]


POSE_REFINEMENT_MARGINS = ("acceptance", "gradient", "function_tolerance", "parameter_tolerance", "pivot")
POSE_REFINEMENT_MAX_ITERATIONS = 1000
POSE_REFINE_FOCAL_LENGTH, POSE_REFINE_EXTRA_PARAMS = 1, 2
POSE_STEP_ACCEPTED, POSE_STEP_REJECTED, POSE_STEP_INVALID, POSE_STEP_TOLERANCE = 1, 2, 3, 4


class PoseRefinementReport(ctypes.Structure):
    _fields_ = [("num_problems", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("num_points", ctypes.c_uint64),
                ("num_iterations", ctypes.c_uint64), ("min_margin", ctypes.c_double * 5), ("setup_ms", ctypes.c_double),
                ("upload_ms", ctypes.c_double), ("solve_ms", ctypes.c_double), ("download_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double)]


FILTER_NEGATIVE_DEPTH, FILTER_REPROJECTION_ERROR, FILTER_TRIANGULATION_ANGLE, FILTER_MEAN_ERROR = 1, 2, 4, 8


class PointFilterOptions(ctypes.Structure):
    """dsm_point_filter_options: IncrementalMapper::Options' filter_max_reproj_error, filter_min_tri_angle and the three
    HasBogusParams bounds (src/sfm/incremental_mapper.h:96-108), shared by DistributedMapperController::Options."""
    _fields_ = [("max_reproj_error", ctypes.c_double), ("min_tri_angle", ctypes.c_double),
                ("min_focal_length_ratio", ctypes.c_double), ("max_focal_length_ratio", ctypes.c_double),
                ("max_extra_param", ctypes.c_double), ("passes", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PointFilterReport(ctypes.Structure):
    _fields_ = [("num_points", ctypes.c_uint64), ("num_observations", ctypes.c_uint64), ("num_selected", ctypes.c_uint64),
                ("num_filtered", ctypes.c_uint64 * 4), ("points_deleted", ctypes.c_uint64 * 4),
                ("observations_deleted", ctypes.c_uint64 * 4), ("num_points_kept", ctypes.c_uint64),
                ("num_observations_kept", ctypes.c_uint64), ("num_images_filtered", ctypes.c_uint64),
                ("lane_path_tracks", ctypes.c_uint64), ("wave_path_tracks", ctypes.c_uint64), ("pairs_evaluated", ctypes.c_uint64),
                ("mean_error_observations", ctypes.c_uint64), ("mean_reprojection_error", ctypes.c_double),
                ("mean_point_error", ctypes.c_double), ("min_depth_margin", ctypes.c_double), ("min_error_margin", ctypes.c_double),
                ("min_angle_margin", ctypes.c_double), ("min_bogus_margin", ctypes.c_double), ("setup_ms", ctypes.c_double),
                ("upload_ms", ctypes.c_double), ("residuals_ms", ctypes.c_double), ("tracks_ms", ctypes.c_double),
                ("angles_ms", ctypes.c_double), ("compaction_ms", ctypes.c_double), ("download_ms", ctypes.c_double),
                ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_}


LOSS_TRIVIAL, LOSS_SOFT_L1, LOSS_CAUCHY = 0, 1, 2
LOCAL_BUNDLE_MARGINS = ("acceptance", "gradient", "pivot", "point_pivot")
LOCAL_BUNDLE_MAX_REDUCED_DIM = 128
LOCAL_BUNDLE_MAX_ITERATIONS = 1000
LOCAL_BUNDLE_TRACE_COLUMNS = 5  # cost, radius, rho, accepted, gradient max-norm


class LocalBundleOptions(ctypes.Structure):
    """dsm_local_bundle_options: IncrementalMapperOptions::LocalBundleAdjustment()
    (src/controllers/incremental_mapper_controller.cc:234-255)."""
    _fields_ = [("max_num_iterations", ctypes.c_int32), ("max_num_consecutive_invalid_steps", ctypes.c_int32),
                ("gradient_tolerance", ctypes.c_double), ("function_tolerance", ctypes.c_double),
                ("parameter_tolerance", ctypes.c_double), ("refine_focal_length", ctypes.c_int32),
                ("refine_principal_point", ctypes.c_int32), ("refine_extra_params", ctypes.c_int32),
                ("loss_function_type", ctypes.c_int32), ("loss_function_scale", ctypes.c_double)]


class LocalBundleResult(ctypes.Structure):
    _fields_ = [("solved", ctypes.c_int32), ("termination", ctypes.c_int32), ("num_iterations", ctypes.c_uint32),
                ("num_successful_steps", ctypes.c_uint32), ("num_invalid_steps", ctypes.c_uint32), ("reduced_dim", ctypes.c_uint32),
                ("num_residuals", ctypes.c_uint64), ("num_effective_parameters", ctypes.c_uint64),
                ("initial_cost", ctypes.c_double), ("final_cost", ctypes.c_double),
                ("initial_mean_reprojection_error", ctypes.c_double), ("final_mean_reprojection_error", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LocalBundleReport(ctypes.Structure):
    _fields_ = [("num_problems", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("num_points", ctypes.c_uint64),
                ("num_observations", ctypes.c_uint64), ("num_iterations", ctypes.c_uint64), ("min_margin", ctypes.c_double * 4),
                ("setup_ms", ctypes.c_double), ("upload_ms", ctypes.c_double), ("solve_ms", ctypes.c_double),
                ("download_ms", ctypes.c_double), ("device_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: (list(getattr(self, k)) if hasattr(getattr(self, k), "__len__") else getattr(self, k)) for k, _ in self._fields_}


SIFT_L1_ROOT, SIFT_L2 = 0, 1


class SiftOptions(ctypes.Structure):
    """dsm_sift_options: SiftExtractionOptions (src/feature/sift.h) without the covariant / SiftGPU fields."""
    _fields_ = [("num_octaves", ctypes.c_int32), ("octave_resolution", ctypes.c_int32), ("first_octave", ctypes.c_int32),
                ("max_num_orientations", ctypes.c_int32), ("max_num_features", ctypes.c_int32), ("upright", ctypes.c_int32),
                ("normalization", ctypes.c_int32), ("reserved", ctypes.c_int32), ("peak_threshold", ctypes.c_double),
                ("edge_threshold", ctypes.c_double)]


class CovariantSiftOptions(ctypes.Structure):
    """dsm_covariant_sift_options: the fields of SiftExtractionOptions (src/feature/sift.h) ExtractCovariantSiftFeaturesCPU reads."""
    _fields_ = [("octave_resolution", ctypes.c_int32), ("first_octave", ctypes.c_int32), ("max_num_features", ctypes.c_int32),
                ("upright", ctypes.c_int32), ("normalization", ctypes.c_int32), ("estimate_affine_shape", ctypes.c_int32),
                ("domain_size_pooling", ctypes.c_int32), ("dsp_num_scales", ctypes.c_int32), ("peak_threshold", ctypes.c_double),
                ("edge_threshold", ctypes.c_double), ("dsp_min_scale", ctypes.c_double), ("dsp_max_scale", ctypes.c_double)]


class UndistortOptions(ctypes.Structure):
    """dsm_undistort_options: UndistortCameraOptions (src/base/undistortion.h:41-62)."""
    _fields_ = [("blank_pixels", ctypes.c_double), ("min_scale", ctypes.c_double), ("max_scale", ctypes.c_double),
                ("max_image_size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("roi_min_x", ctypes.c_double),
                ("roi_min_y", ctypes.c_double), ("roi_max_x", ctypes.c_double), ("roi_max_y", ctypes.c_double)]


class PatchMatchOptions(ctypes.Structure):
    """dsm_patch_match_options: PatchMatchOptions (src/mvs/patch_match.h:59-139) + the seed of the Philox key."""
    _fields_ = [("window_radius", ctypes.c_int32), ("window_step", ctypes.c_int32), ("num_samples", ctypes.c_int32),
                ("num_iterations", ctypes.c_int32), ("geom_consistency", ctypes.c_int32), ("filter", ctypes.c_int32),
                ("filter_min_num_consistent", ctypes.c_int32), ("seed", ctypes.c_uint32), ("sigma_spatial", ctypes.c_double),
                ("sigma_color", ctypes.c_double), ("ncc_sigma", ctypes.c_double), ("min_triangulation_angle", ctypes.c_double),
                ("incident_angle_sigma", ctypes.c_double), ("geom_consistency_regularizer", ctypes.c_double),
                ("geom_consistency_max_cost", ctypes.c_double), ("filter_min_ncc", ctypes.c_double),
                ("filter_min_triangulation_angle", ctypes.c_double), ("filter_geom_consistency_max_cost", ctypes.c_double)]


class MvsImage(ctypes.Structure):
    """dsm_mvs_image: one image of the undistorted workspace (dsm_patch_match)."""
    _fields_ = [("data", ctypes.c_void_p), ("row_stride", ctypes.c_uint64), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("K", ctypes.c_float * 9), ("R", ctypes.c_float * 9), ("T", ctypes.c_float * 3), ("reserved", ctypes.c_uint32),
                ("depth_map", ctypes.c_void_p), ("normal_map", ctypes.c_void_p)]


PATCH_MATCH_STAGES = ("upload", "reference_filter", "initial_cost", "sweeps", "rotation", "download")


class StereoFusionOptions(ctypes.Structure):
    """dsm_stereo_fusion_options: StereoFusionOptions (src/mvs/fusion.h:55-85) + the scheduling field lane_capacity."""
    _fields_ = [("min_num_pixels", ctypes.c_int32), ("max_num_pixels", ctypes.c_int32), ("max_traversal_depth", ctypes.c_int32),
                ("lane_capacity", ctypes.c_int32), ("max_reproj_error", ctypes.c_double), ("max_depth_error", ctypes.c_double),
                ("max_normal_error", ctypes.c_double)]


class FusionImage(ctypes.Structure):
    """dsm_fusion_image: the maps, the bitmap and the matrices of one image (dsm_fuse_stereo)."""
    _fields_ = [("used", ctypes.c_int32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("bitmap_width", ctypes.c_uint32),
                ("bitmap_height", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("row_stride", ctypes.c_uint64),
                ("depth_map", ctypes.c_void_p), ("normal_map", ctypes.c_void_p), ("rgb", ctypes.c_void_p),
                ("P", ctypes.c_float * 12), ("inv_P", ctypes.c_float * 12), ("inv_R", ctypes.c_float * 9),
                ("bitmap_scale", ctypes.c_float * 2), ("reserved2", ctypes.c_uint32)]


FUSED_POINT_DTYPE = np.dtype([("xyz", "<f4", 3), ("normal", "<f4", 3), ("rgb", "u1", 3), ("reserved", "u1")])  # dsm_fused_point
STEREO_FUSION_STAGES = ("upload", "traversal", "claims_commit", "medians", "download", "rounds", "traversals")
# the host build of csrc/stereo_fusion.h: StereoFusion::Run on one CPU thread from the kernels' text
FUSION_HOST_LIB_PATH = os.path.join(_HERE, "libdsm_stereo_fusion_host.so")


class SourceSelectionOptions(ctypes.Structure):
    """dsm_source_selection_options: the arguments of Model::GetMaxOverlappingImages (src/mvs/model.cc:119-129)."""
    _fields_ = [("max_num_src_images", ctypes.c_int32), ("triangulation_angle_percentile", ctypes.c_float),
                ("min_triangulation_angle", ctypes.c_double)]


IMAGE_OVERLAP_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("count", "<u4"), ("angle", "<f4")])  # dsm_image_overlap
SOURCE_SELECTION_STAGES = ("upload", "depths", "items", "sort", "pairs_select", "download", "items_count", "pairs", "nan_items")
# the host build of csrc/source_selection.h: the queries of mvs::Model on one CPU thread from the kernels' text
SELECTION_HOST_LIB_PATH = os.path.join(_HERE, "libdsm_source_selection_host.so")


class InitialPairOptions(ctypes.Structure):
    """dsm_initial_pair_options (IncrementalMapper::Options, incremental_mapper.h:68-81)."""
    _fields_ = [("init_min_num_inliers", ctypes.c_int32), ("init_max_reg_trials", ctypes.c_int32), ("init_max_error", ctypes.c_double),
                ("init_max_forward_motion", ctypes.c_double), ("init_min_tri_angle", ctypes.c_double), ("user_seed", ctypes.c_uint32),
                ("speculation_window", ctypes.c_uint32)]


class InitialPairResult(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("image_id1", ctypes.c_uint32), ("image_id2", ctypes.c_uint32), ("num_tried", ctypes.c_uint32),
                ("num_points", ctypes.c_uint64), ("two_view_geometry", TwoViewGeometry)]


class InitialPairReport(ctypes.Structure):
    _fields_ = [("num_rounds", ctypes.c_uint32), ("num_batches", ctypes.c_uint32), ("num_candidates", ctypes.c_uint64),
                ("num_verified", ctypes.c_uint64), ("num_speculated", ctypes.c_uint64), ("min_tri_angle_margin", ctypes.c_double),
                ("min_forward_motion_margin", ctypes.c_double), ("min_point_angle_margin", ctypes.c_double),
                ("min_point_depth_margin", ctypes.c_double), ("setup_ms", ctypes.c_double), ("graph_ms", ctypes.c_double),
                ("gather_ms", ctypes.c_double), ("verify_ms", ctypes.c_double), ("pose_ms", ctypes.c_double),
                ("triangulate_ms", ctypes.c_double), ("device_ms", ctypes.c_double)]


NO_IMAGE = 0xFFFFFFFF  # DSM_NO_IMAGE
INITIAL_PAIR_NONE, INITIAL_PAIR_FOUND = 0, 1
INITIAL_PAIR_HOST_LIB_PATH = os.path.join(_HERE, "libdsm_initial_pair_host.so")


class NextImagesOptions(ctypes.Structure):
    """dsm_next_images_options (IncrementalMapper::Options, incremental_mapper.h:87-131)."""
    _fields_ = [("image_selection_method", ctypes.c_int32), ("abs_pose_min_num_inliers", ctypes.c_int32), ("max_reg_trials", ctypes.c_int32)]


class NextImagesReport(ctypes.Structure):
    _fields_ = [("num_eligible", ctypes.c_uint64), ("num_first_bucket", ctypes.c_uint64), ("num_second_bucket", ctypes.c_uint64),
                ("num_batches", ctypes.c_uint32), ("setup_ms", ctypes.c_double), ("graph_ms", ctypes.c_double),
                ("visibility_ms", ctypes.c_double), ("score_ms", ctypes.c_double), ("rank_ms", ctypes.c_double), ("device_ms", ctypes.c_double)]


class LocalBundleSelectionOptions(ctypes.Structure):
    """dsm_local_bundle_selection_options (IncrementalMapper::Options, incremental_mapper.h:98-102)."""
    _fields_ = [("local_ba_num_images", ctypes.c_int32), ("local_ba_min_tri_angle", ctypes.c_double)]


class LocalBundleSelectionReport(ctypes.Structure):
    _fields_ = [("num_copied", ctypes.c_uint64), ("num_chained", ctypes.c_uint64), ("num_angles", ctypes.c_uint64), ("num_filled", ctypes.c_uint64),
                ("min_tri_angle_margin", ctypes.c_double), ("num_batches", ctypes.c_uint32), ("setup_ms", ctypes.c_double),
                ("tracks_ms", ctypes.c_double), ("overlap_ms", ctypes.c_double), ("angles_ms", ctypes.c_double), ("device_ms", ctypes.c_double)]


# the arguments dsm_find_local_bundles and its host build share, from num_images to the overlap capacity
_LOCAL_BUNDLES_ARGTYPES = ([ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 9 + [ctypes.c_uint32]
                           + [ctypes.c_void_p] * 2 + [ctypes.POINTER(LocalBundleSelectionOptions), ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
                           + [ctypes.c_void_p] * 4 + [ctypes.c_uint64])
NEXT_IMAGE_MAX_VISIBLE_POINTS_NUM, NEXT_IMAGE_MAX_VISIBLE_POINTS_RATIO, NEXT_IMAGE_MIN_UNCERTAINTY = 0, 1, 2
NEXT_IMAGES_HOST_LIB_PATH = os.path.join(_HERE, "libdsm_next_images_host.so")
TRACK_UPDATE_HOST_LIB_PATH = os.path.join(_HERE, "libdsm_track_update_host.so")
# the arguments dsm_find_next_images and its host build share, from num_cameras to slot_filtered
_NEXT_IMAGES_SCENE_ARGTYPES = ([ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_void_p] * 4 + [ctypes.c_uint32]
                               + [ctypes.c_void_p] * 3 + [ctypes.c_uint32] + [ctypes.c_void_p] * 7)


class VocabularyBuildOptions(ctypes.Structure):
    """dsm_vocabulary_build_options: VisualIndex::BuildOptions (src/retrieval/visual_index.h:99-118) + the scheduling field."""
    _fields_ = [("num_visual_words", ctypes.c_int32), ("branching", ctypes.c_int32), ("num_iterations", ctypes.c_int32),
                ("workgroup_node_max", ctypes.c_int32)]


class VocabularyTreeNode(ctypes.Structure):
    """dsm_vocabulary_tree_node (dsm_get_vocabulary_tree)."""
    _fields_ = [("parent", ctypes.c_int32), ("first_child", ctypes.c_int32), ("size", ctypes.c_int32),
                ("variance_bits", ctypes.c_uint32), ("radius_bits", ctypes.c_uint32)]


RAND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)  # int (*rand_fn)(void* user) of dsm_retrieval_quantize
VOCABULARY_BUILD_STAGES = ("seeding", "assignment", "centre_update", "statistics", "partition", "embedding")

CAMERA_SIZE_ONLY = -1  # DSM_CAMERA_SIZE_ONLY: a dsm_camera of which dsm_warp_images reads only width and height
UNDISTORTION_STAGES = ("border_scan", "points", "warp_upload", "warp_kernel", "warp_download")


def lib(check=False):
    """Loads the shared library (check=True: the check build); raises if it has not been built (no fallback)."""
    if check not in _libs:
        path = CHECK_LIB_PATH if check else LIB_PATH
        if not os.path.exists(path):
            raise DsmError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(make -C dagsfm_amd/csrc)" % path)
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.dsm_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
        L.dsm_ctx_destroy.argtypes = [vp]
        L.dsm_ctx_destroy.restype = None
        L.dsm_last_error.argtypes = [vp]
        L.dsm_last_error.restype = ctypes.c_char_p
        L.dsm_sync.argtypes = [vp]
        L.dsm_set_images.argtypes = [vp, ctypes.c_uint32, u32p, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                     ctypes.c_uint32, ctypes.POINTER(Camera)]
        L.dsm_match_pairs.argtypes = [vp, ctypes.c_uint32, u32p, ctypes.POINTER(MatchOptions)]
        L.dsm_get_match_counts.argtypes = [vp, vp]
        L.dsm_get_matches.argtypes = [vp, vp, vp, ctypes.c_uint64]
        L.dsm_match_sift_features.argtypes = [vp, ctypes.POINTER(MatchOptions), u8p, ctypes.c_uint32, u8p,
                                              ctypes.c_uint32, u32p, u32p]
        L.dsm_get_match_kernel_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), u32p]
        L.dsm_get_match_resolve_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.dsm_pair_seed.argtypes = [ctypes.c_uint32] * 3
        L.dsm_pair_seed.restype = ctypes.c_uint32
        L.dsm_verify_pairs.argtypes = [vp, ctypes.POINTER(TwoViewOptions), u32p, ctypes.c_uint32, ctypes.c_int32]
        L.dsm_guided_match_pairs.argtypes = [vp, ctypes.POINTER(MatchOptions), ctypes.POINTER(TwoViewOptions), ctypes.c_int32]
        L.dsm_get_two_view_geometries.argtypes = [vp, vp]
        L.dsm_get_inlier_matches.argtypes = [vp, vp, vp, ctypes.c_uint64]
        L.dsm_get_verify_kernel_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.dsm_estimate_two_view_geometry.argtypes = [vp, ctypes.POINTER(Camera), ctypes.POINTER(ctypes.c_double),
                                                     ctypes.c_uint32, ctypes.POINTER(Camera),
                                                     ctypes.POINTER(ctypes.c_double), ctypes.c_uint32, u32p, ctypes.c_uint32,
                                                     ctypes.POINTER(TwoViewOptions), ctypes.c_uint32,
                                                     ctypes.POINTER(TwoViewGeometry), u32p]
        L.dsm_debug_sample_sequence.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p]
        L.dsm_get_device_info.argtypes = [vp, ctypes.POINTER(DeviceInfo)]
        L.dsm_get_match_gather_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.dsm_get_match_tail_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        L.dsm_retrieval_set_vocabulary.argtypes = [vp, ctypes.POINTER(Vocabulary)]
        L.dsm_retrieval_index.argtypes = [vp]
        L.dsm_retrieval_query.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, vp]
        L.dsm_retrieval_debug_word_ids.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp]
        L.dsm_get_retrieval_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.dsm_view_graph_filter_cycles.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_double, vp, vp]
        L.dsm_view_graph_rotation_averaging.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(RotationAveragingOptions)] + [vp] * 7
        L.dsm_default_rotation_averaging_options.argtypes = [ctypes.POINTER(RotationAveragingOptions)]
        L.dsm_default_rotation_averaging_options.restype = None
        L.dsm_default_nonlinear_rotation_options.argtypes = [ctypes.POINTER(NonlinearRotationOptions)]
        L.dsm_default_nonlinear_rotation_options.restype = None
        L.dsm_view_graph_rotation_averaging_nonlinear.argtypes = ([vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, vp, vp,
                                                                  ctypes.POINTER(NonlinearRotationOptions)] + [vp] * 8)
        L.dsm_debug_pairwise_rotation_error.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_double, vp, vp, vp]
        L.dsm_view_graph_cluster.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.POINTER(ClusteringOptions)] + [vp] * 8
        L.dsm_default_clustering_options.argtypes = [ctypes.POINTER(ClusteringOptions)]
        L.dsm_default_clustering_options.restype = None
        L.dsm_get_clustering_spectrum.argtypes = [vp, vp, ctypes.c_uint32, vp, ctypes.c_uint64, vp, vp, vp]
        L.dsm_default_align_options.argtypes = [ctypes.POINTER(AlignOptions)]
        L.dsm_default_align_options.restype = None
        L.dsm_align_seed.argtypes = [ctypes.c_uint32] * 4
        L.dsm_align_seed.restype = ctypes.c_uint32
        L.dsm_align_clusters.argtypes = ([vp, ctypes.c_uint32] + [vp] * 7 + [ctypes.POINTER(AlignOptions), vp, vp, ctypes.c_uint32]
                                         + [vp] * 8)
        L.dsm_default_bundle_adjustment_options.argtypes = [ctypes.POINTER(BundleAdjustmentOptions)]
        L.dsm_default_bundle_adjustment_options.restype = None
        L.dsm_bundle_adjust.argtypes = ([vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32] + [vp] * 5 + [ctypes.c_uint32] + [vp] * 6
                                        + [ctypes.POINTER(BundleAdjustmentOptions), vp, vp])
        L.dsm_default_triangulation_options.argtypes = [ctypes.POINTER(TriangulationOptions)]
        L.dsm_default_triangulation_options.restype = None
        L.dsm_retriangulate.argtypes = ([vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32] + [vp] * 8 + [ctypes.c_uint32, vp, vp, ctypes.c_uint32]
                                        + [vp] * 3 + [ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.POINTER(TriangulationOptions)]
                                        + [vp] * 14)
        L.dsm_default_pair_retriangulation_options.argtypes = [ctypes.POINTER(PairRetriangulationOptions)]
        L.dsm_default_pair_retriangulation_options.restype = None
        L.dsm_retriangulate_pairs.argtypes = ([vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32] + [vp] * 8
                                              + [ctypes.c_uint32, vp, vp, ctypes.c_uint32] + [vp] * 3
                                              + [ctypes.c_uint64, ctypes.POINTER(PairRetriangulationOptions)] + [vp] * 16)
        L.dsm_default_absolute_pose_options.argtypes = [ctypes.POINTER(AbsolutePoseOptions)]
        L.dsm_default_absolute_pose_options.restype = None
        L.dsm_absolute_pose_seed.argtypes = [ctypes.c_uint32] * 3
        L.dsm_absolute_pose_seed.restype = ctypes.c_uint32
        L.dsm_absolute_pose_factors.argtypes = [ctypes.POINTER(AbsolutePoseOptions), vp, ctypes.c_uint32]
        L.dsm_absolute_pose_factors.restype = ctypes.c_uint32
        L.dsm_absolute_pose_max_trials.argtypes = [ctypes.POINTER(AbsolutePoseOptions)]
        L.dsm_absolute_pose_max_trials.restype = ctypes.c_uint64
        L.dsm_estimate_absolute_poses.argtypes = [vp, ctypes.c_uint32] + [vp] * 5 + [ctypes.POINTER(AbsolutePoseOptions)] + [vp] * 5
        L.dsm_default_pose_refinement_options.argtypes = [ctypes.POINTER(PoseRefinementOptions)]
        L.dsm_default_pose_refinement_options.restype = None
        L.dsm_refine_absolute_poses.argtypes = [vp, ctypes.c_uint32] + [vp] * 8 + [ctypes.POINTER(PoseRefinementOptions)] + [vp] * 4
        L.dsm_default_point_filter_options.argtypes = [ctypes.POINTER(PointFilterOptions)]
        L.dsm_default_point_filter_options.restype = None
        L.dsm_filter_points3D.argtypes = ([vp, ctypes.c_uint32, vp, ctypes.c_uint32] + [vp] * 4 + [ctypes.c_uint32] + [vp] * 6
                                          + [ctypes.POINTER(PointFilterOptions)] + [vp] * 7)
        L.dsm_default_local_bundle_options.argtypes = [ctypes.POINTER(LocalBundleOptions)]
        L.dsm_default_local_bundle_options.restype = None
        L.dsm_adjust_local_bundles.argtypes = [vp, ctypes.c_uint32] + [vp] * 18 + [ctypes.POINTER(LocalBundleOptions)] + [vp] * 4
        L.dsm_debug_image_to_world.argtypes = [vp, ctypes.POINTER(Camera), ctypes.c_uint32, ctypes.POINTER(ctypes.c_double),
                                               ctypes.POINTER(ctypes.c_double)]
        L.dsm_sift_default_options.argtypes = [ctypes.POINTER(SiftOptions)]
        L.dsm_sift_default_options.restype = None
        L.dsm_extract_sift.argtypes = [vp, ctypes.POINTER(SiftOptions), vp] + [ctypes.c_uint32] * 4 + [vp, vp, u32p]
        L.dsm_covariant_sift_default_options.argtypes = [ctypes.POINTER(CovariantSiftOptions)]
        L.dsm_covariant_sift_default_options.restype = None
        L.dsm_extract_covariant_sift.argtypes = [vp, ctypes.POINTER(CovariantSiftOptions), vp] + [ctypes.c_uint32] * 4 + [vp, vp, u32p]
        L.dsm_extract_covariant_sift_affine.argtypes = L.dsm_extract_covariant_sift.argtypes
        L.dsm_get_affine_shape_stats.argtypes = [vp, u32p, vp, vp]
        L.dsm_get_covariant_sift_raw.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, u32p]
        L.dsm_get_covariant_sift_time.argtypes = [vp, vp]
        L.dsm_default_undistort_options.argtypes = [ctypes.POINTER(UndistortOptions)]
        L.dsm_default_undistort_options.restype = None
        L.dsm_undistort_cameras.argtypes = [vp, ctypes.POINTER(UndistortOptions), ctypes.c_uint32, vp, vp]
        L.dsm_undistort_points2D.argtypes = [vp, ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp]
        L.dsm_warp_images.argtypes = ([vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32, vp, ctypes.c_uint64, ctypes.c_uint64, vp,
                                       ctypes.c_uint64, ctypes.c_uint64, vp, vp, vp])
        L.dsm_get_undistortion_time.argtypes = [vp, vp]
        L.dsm_default_vocabulary_build_options.argtypes = [ctypes.POINTER(VocabularyBuildOptions)]
        L.dsm_default_vocabulary_build_options.restype = None
        L.dsm_retrieval_quantize.argtypes = [vp, ctypes.POINTER(VocabularyBuildOptions), vp, ctypes.c_uint64, vp, vp, u32p, vp, vp]
        L.dsm_get_vocabulary_tree.argtypes = [vp, u32p, vp, vp, ctypes.c_uint32, vp, ctypes.c_uint64]
        L.dsm_retrieval_train_embedding.argtypes = [vp, vp, ctypes.c_uint64, vp, ctypes.c_uint32, vp, vp, vp, vp]
        L.dsm_get_vocabulary_build_time.argtypes = [vp, vp]
        L.dsm_default_patch_match_options.argtypes = [ctypes.POINTER(PatchMatchOptions)]
        L.dsm_default_patch_match_options.restype = None
        L.dsm_patch_match.argtypes = [vp, ctypes.POINTER(PatchMatchOptions), ctypes.c_uint32, vp, ctypes.c_uint32] + [vp] * 9
        L.dsm_get_patch_match_time.argtypes = [vp, vp]
        L.dsm_default_stereo_fusion_options.argtypes = [ctypes.POINTER(StereoFusionOptions)]
        L.dsm_default_stereo_fusion_options.restype = None
        L.dsm_fuse_stereo.argtypes = [vp, ctypes.POINTER(StereoFusionOptions), ctypes.c_uint32, vp, vp, vp, u64p]
        L.dsm_get_fused_points.argtypes = [vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64]
        L.dsm_get_stereo_fusion_time.argtypes = [vp, vp]
        L.dsm_get_stereo_fusion_rounds.argtypes = [vp, vp, vp, ctypes.c_uint32]
        L.dsm_default_source_selection_options.argtypes = [ctypes.POINTER(SourceSelectionOptions)]
        L.dsm_default_source_selection_options.restype = None
        L.dsm_select_source_images.argtypes = [vp, ctypes.POINTER(SourceSelectionOptions), ctypes.c_uint32, vp, vp, ctypes.c_uint64, vp, vp, vp, vp, vp,
                                               u64p, u64p]
        L.dsm_get_source_images.argtypes = [vp, vp, vp, ctypes.c_uint64]
        L.dsm_get_image_overlap.argtypes = [vp, vp, ctypes.c_uint64]
        L.dsm_get_source_selection_time.argtypes = [vp, vp]
        L.dsm_default_initial_pair_options.argtypes = [ctypes.POINTER(InitialPairOptions)]
        L.dsm_default_initial_pair_options.restype = None
        L.dsm_find_initial_pairs.argtypes = ([vp, ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp, vp, vp, vp, ctypes.c_uint32, vp, vp, vp,
                                              ctypes.c_uint32] + [vp] * 8 + [ctypes.POINTER(InitialPairOptions), vp, vp, vp, ctypes.c_uint64,
                                                                             vp, vp, vp, ctypes.c_uint64, vp, vp, ctypes.c_uint64, vp])
        L.dsm_default_next_images_options.argtypes = [ctypes.POINTER(NextImagesOptions)]
        L.dsm_default_next_images_options.restype = None
        L.dsm_find_next_images.argtypes = ([vp] + _NEXT_IMAGES_SCENE_ARGTYPES + [ctypes.POINTER(NextImagesOptions), vp, vp, ctypes.c_uint64,
                                                                                 vp, vp, vp, vp])
        L.dsm_default_local_bundle_selection_options.argtypes = [ctypes.POINTER(LocalBundleSelectionOptions)]
        L.dsm_default_local_bundle_selection_options.restype = None
        L.dsm_find_local_bundles.argtypes = [vp] + _LOCAL_BUNDLES_ARGTYPES + [vp]
        L.dsm_default_track_update_options.argtypes = [ctypes.POINTER(TrackUpdateOptions)]
        L.dsm_default_track_update_options.restype = None
        L.dsm_update_tracks.argtypes = [vp] + _TRACK_UPDATE_ARGTYPES
        L.dsm_complete_images.argtypes = [vp] + _COMPLETE_IMAGES_ARGTYPES
        L.dsm_default_match_options.argtypes = [ctypes.POINTER(MatchOptions)]
        L.dsm_default_match_options.restype = None
        L.dsm_default_two_view_options.argtypes = [ctypes.POINTER(TwoViewOptions)]
        L.dsm_default_two_view_options.restype = None
        L.dsm_set_debug_option.restype = ctypes.c_int
        L.dsm_set_debug_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
        _libs[check] = L
    return _libs[check]


def pair_seed(id1, id2, user_seed=0):
    return int(lib().dsm_pair_seed(id1, id2, user_seed))


def simple_pinhole(f, cx, cy, width, height, prior=True):
    c = Camera(model_id=0, has_prior_focal_length=int(bool(prior)), width=width, height=height)
    c.params[0], c.params[1], c.params[2] = f, cx, cy
    return c


CAMERA_MODEL_NUM_PARAMS = (3, 4, 4, 5, 8, 8, 12, 5, 4, 5, 12)  # camera_models.h:187-349, ids 0..10


def camera(model_id, params, width, height, prior=True):
    """dsm_camera of any of the reference's camera models (params in the reference's order)."""
    c = Camera(model_id=model_id, has_prior_focal_length=int(bool(prior)), width=width, height=height)
    for k, v in enumerate(params):
        c.params[k] = float(v)
    return c


def copy_camera(c):
    """A Camera of its own memory with c's fields (an element of a ctypes array is a view of the array)."""
    return Camera.from_buffer_copy(bytes(c))


def default_match_options(**kw):
    o = MatchOptions()
    lib().dsm_default_match_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_two_view_options(**kw):
    o = TwoViewOptions()
    lib().dsm_default_two_view_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_rotation_averaging_options(**kw):
    o = RotationAveragingOptions()
    lib().dsm_default_rotation_averaging_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_nonlinear_rotation_options(**kw):
    o = NonlinearRotationOptions()
    lib().dsm_default_nonlinear_rotation_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_clustering_options(**kw):
    o = ClusteringOptions()
    lib().dsm_default_clustering_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_align_options(**kw):
    o = AlignOptions()
    lib().dsm_default_align_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_bundle_adjustment_options(**kw):
    o = BundleAdjustmentOptions()
    lib().dsm_default_bundle_adjustment_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_triangulation_options(**kw):
    o = TriangulationOptions()
    lib().dsm_default_triangulation_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_pair_retriangulation_options(**kw):
    """re_max_angle_error, re_min_ratio, re_max_trials by name; any other keyword is a field of the `tri` member."""
    o = PairRetriangulationOptions()
    lib().dsm_default_pair_retriangulation_options(ctypes.byref(o))
    own = {k for k, _ in PairRetriangulationOptions._fields_}
    for k, v in kw.items():
        setattr(o if k in own else o.tri, k, v)
    return o


def default_absolute_pose_options(**kw):
    o = AbsolutePoseOptions()
    lib().dsm_default_absolute_pose_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_pose_refinement_options(**kw):
    o = PoseRefinementOptions()
    lib().dsm_default_pose_refinement_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_point_filter_options(**kw):
    o = PointFilterOptions()
    lib().dsm_default_point_filter_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_sift_options(**kw):
    o = SiftOptions()
    lib().dsm_sift_default_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_covariant_sift_options(check=False, **kw):
    o = CovariantSiftOptions()
    lib(check).dsm_covariant_sift_default_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_undistort_options(**kw):
    o = UndistortOptions()
    lib().dsm_default_undistort_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def default_patch_match_options(**kw):
    o = PatchMatchOptions()
    lib().dsm_default_patch_match_options(ctypes.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def consistency_graph(mask, src_image_idxs):
    """GetConsistentImageIdxs (src/mvs/patch_match_cuda.cu:1217-1241) of a consistency mask [S][H][W]: the int32 vector
    col, row, count, ids... of every pixel with at least one consistent source image, pixels in row-major order, the ids
    (src_image_idxs[slice]) in slice order -- what the reference writes as its consistency graph."""
    mask = np.asarray(mask)
    ids = np.asarray(src_image_idxs, dtype=np.int32)
    assert mask.ndim == 3 and mask.shape[0] == len(ids)
    on = np.moveaxis(mask != 0, 0, -1)  # [H][W][S]
    count = on.sum(axis=-1)
    rows, cols = np.nonzero(count)
    out = []
    for r, c in zip(rows.tolist(), cols.tolist()):
        out += [c, r, int(count[r, c])] + ids[on[r, c]].tolist()
    return np.array(out, dtype=np.int32)


def write_mvs_array(path, array):
    """Mat<float>::Write (src/mvs/mat.h:179-191): the text header `W&H&C&`, then the floats little-endian, slice by slice.
    array: [H][W] or [C][H][W] float32 -- the layout of dsm_patch_match's depth and normal maps, readable by stereo_fusion."""
    a = np.asarray(array, dtype=np.float32)
    if a.ndim == 2:
        a = a[None]
    assert a.ndim == 3
    with open(path, "wb") as f:
        f.write(("%d&%d&%d&" % (a.shape[2], a.shape[1], a.shape[0])).encode("ascii"))
        f.write(np.ascontiguousarray(a).astype("<f4").tobytes())


def read_mvs_array(path):
    """Mat<float>::Read (src/mvs/mat.h:156-177) -> [C][H][W] float32."""
    with open(path, "rb") as f:
        blob = f.read()
    parts = blob.split(b"&", 3)
    if len(parts) != 4:
        raise DsmError("%s: no W&H&C& header" % path)
    w, h, c = (int(p) for p in parts[:3])
    if w <= 0 or h <= 0 or c <= 0 or len(parts[3]) != 4 * w * h * c:
        raise DsmError("%s: header %dx%dx%d does not match %d bytes of data" % (path, w, h, c, len(parts[3])))
    return np.frombuffer(parts[3], dtype="<f4").astype(np.float32).reshape(c, h, w)


def default_stereo_fusion_options(**kw):
    o = StereoFusionOptions()
    lib().dsm_default_stereo_fusion_options(ctypes.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def fusion_matrices(K, R, T, scale_x=1.0, scale_y=1.0):
    """P [12], inv_P [12], inv_R [9] float32 as StereoFusion::Run composes them (src/mvs/fusion.cc:220-235) from the float K, R,
    T of an mvs::Image and the bitmap scales, by the ruling of DESIGN.md 24 / 26 where Eigen fixes no order: K's focal lengths
    and principal point times the scales in float; P = [K R | K T] with every entry summed left to right in float; inv_P = the
    top rows of [P; 0 0 0 1]^-1 = [M^-1 | -M^-1 p] with M^-1 the adjugate of P's left block over its determinant in double
    (entries and the product summed left to right), rounded to float once; inv_R = R^T.  A host with Eigen passes
    ComposeProjectionMatrix's own bits to dsm_fuse_stereo instead."""
    f32 = np.float32
    K = np.asarray(K, dtype=f32).reshape(3, 3).copy()
    R = np.asarray(R, dtype=f32).reshape(3, 3)
    T = np.asarray(T, dtype=f32).reshape(3)
    sx, sy = f32(scale_x), f32(scale_y)
    K[0, 0] *= sx
    K[0, 2] *= sx
    K[1, 1] *= sy
    K[1, 2] *= sy
    P = np.zeros((3, 4), dtype=f32)
    for r in range(3):
        for c in range(3):
            P[r, c] = (K[r, 0] * R[0, c] + K[r, 1] * R[1, c]) + K[r, 2] * R[2, c]
        P[r, 3] = (K[r, 0] * T[0] + K[r, 1] * T[1]) + K[r, 2] * T[2]
    m = P[:, :3].astype(np.float64)
    adj = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            r1, r2, c1, c2 = (c + 1) % 3, (c + 2) % 3, (r + 1) % 3, (r + 2) % 3
            adj[r, c] = m[r1, c1] * m[r2, c2] - m[r1, c2] * m[r2, c1]
    det = (m[0, 0] * adj[0, 0] + m[0, 1] * adj[1, 0]) + m[0, 2] * adj[2, 0]
    inv = adj / det
    p = P[:, 3].astype(np.float64)
    inv_P = np.zeros((3, 4), dtype=f32)
    inv_P[:, :3] = inv
    for r in range(3):
        inv_P[r, 3] = -((inv[r, 0] * p[0] + inv[r, 1] * p[1]) + inv[r, 2] * p[2])
    return P.reshape(12), inv_P.reshape(12), np.ascontiguousarray(R.T).reshape(9)


def overlapping_images(tracks, n_images, num_images):
    """Model::GetMaxOverlappingImages (src/mvs/model.cc:119-169) with the triangulation-angle gate at fusion's 0 (fusion.cc:
    171-174), where it passes every image: per image the up to num_images images that share the most sparse points with it
    (ComputeSharedPoints :218-233; tracks = the image indices of every point, repeats counted as the reference counts them),
    most shared first.  The reference's std::sort / std::partial_sort leave the order of equal counts open; here a tie goes to
    the lower image index."""
    shared = [dict() for _ in range(n_images)]
    for track in tracks:
        track = [int(t) for t in track]
        for i in range(len(track)):
            for j in range(i):
                a, b = track[i], track[j]
                if a != b:
                    shared[a][b] = shared[a].get(b, 0) + 1
                    shared[b][a] = shared[b].get(a, 0) + 1
    return [[b for b, _ in sorted(s.items(), key=lambda kv: (-kv[1], kv[0]))[:int(num_images)]] for s in shared]


def default_source_selection_options(**kw):
    """The defaults of dsm_source_selection_options with keywords over them.  Needs no device library: the host build has them."""
    o = SourceSelectionOptions()
    selection_host_lib().dsm_ss_host_default_options(ctypes.byref(o))
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def _selection_call_arguments(R, T, xyz, tracks, candidate_mask):
    """The arrays of dsm_select_source_images from R [n][9], T [n][3], xyz [m][3] and tracks (a list of index lists, or the CSR
    pair (offsets, images))."""
    R = np.ascontiguousarray(np.asarray(R, dtype=np.float32).reshape(-1, 9))
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float32).reshape(-1, 3))
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32).reshape(-1, 3))
    assert len(R) == len(T), "one R and one T per image"
    if isinstance(tracks, tuple):
        offs = np.ascontiguousarray(tracks[0], dtype=np.uint64)
        idx = np.ascontiguousarray(tracks[1], dtype=np.uint32)
    else:
        offs = np.zeros(len(tracks) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(t) for t in tracks])
        idx = np.array([int(i) for t in tracks for i in t], dtype=np.uint32)
    assert len(offs) == len(xyz) + 1, "one track per point"
    mask = None
    if candidate_mask is not None:
        mask = np.ascontiguousarray(np.asarray(candidate_mask) != 0, dtype=np.uint8)
        assert len(mask) == len(R), "one mask byte per image"
    return R, T, xyz, offs, idx, mask


def _selection_result(n, ranges, loff, limg, rec, stats):
    return {"sources": [limg[int(loff[a]):int(loff[a + 1])].tolist() for a in range(n)], "depth_ranges": ranges[:n].copy(),
            "pairs": (rec["a"].copy(), rec["b"].copy(), rec["count"].copy(), rec["angle"].copy()), "stats": stats}


def selection_host_lib():
    """libdsm_source_selection_host.so, the host build of csrc/source_selection.h; raises if it has not been built."""
    if "selection_host" not in _libs:
        if not os.path.exists(SELECTION_HOST_LIB_PATH):
            raise DsmError("%s is missing: run make -C dagsfm_amd/csrc" % SELECTION_HOST_LIB_PATH)
        L = ctypes.CDLL(SELECTION_HOST_LIB_PATH)
        vp, u64, u64p = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
        for f in (L.dsm_ss_host_run, L.dsm_ss_host_run_serial):
            f.argtypes = [ctypes.POINTER(SourceSelectionOptions), ctypes.c_uint32, vp, vp, u64, vp, vp, vp, vp, vp, u64p, u64p, vp,
                          ctypes.POINTER(ctypes.c_char_p)]
        L.dsm_ss_host_get.argtypes = [vp, vp, vp]
        L.dsm_ss_host_get.restype = None
        L.dsm_ss_host_default_options.argtypes = [ctypes.POINTER(SourceSelectionOptions)]
        L.dsm_ss_host_default_options.restype = None
        L.dsm_ss_host_acos.argtypes = [ctypes.c_double]
        L.dsm_ss_host_acos.restype = ctypes.c_double
        L.dsm_ss_host_decode_item.argtypes = [u64, u64p, u64p]
        L.dsm_ss_host_decode_item.restype = None
        L.dsm_ss_host_encode_item.argtypes = [u64, u64]
        L.dsm_ss_host_encode_item.restype = u64
        L.dsm_ss_host_depth_index.argtypes = [u64, ctypes.c_float]
        L.dsm_ss_host_depth_index.restype = u64
        L.dsm_ss_host_percentile_index.argtypes = [ctypes.c_float, u64]
        L.dsm_ss_host_percentile_index.restype = u64
        L.dsm_ss_host_min_angle_rad.argtypes = [ctypes.c_double]
        L.dsm_ss_host_min_angle_rad.restype = ctypes.c_float
        L.dsm_ss_host_angle_bits.argtypes = [vp, vp, vp]
        L.dsm_ss_host_angle_bits.restype = ctypes.c_uint32
        _libs["selection_host"] = L
    return _libs["selection_host"]


def selection_host(R, T, xyz, tracks, options=None, candidate_mask=None, serial=False, **kw):
    """dsm_select_source_images' results on one CPU thread by the host build of the kernels' header (no GPU, no context): the
    dict of Context.select_source_images, its "stats" holding items, pairs and nan_items.  serial: the reference's loops over
    dense tables in place of the sorted schedule."""
    L = selection_host_lib()
    assert options is None or not kw, "pass a SourceSelectionOptions or keywords, not both"
    o = options if options is not None else default_source_selection_options(**kw)
    R, T, xyz, offs, idx, mask = _selection_call_arguments(R, T, xyz, tracks, candidate_mask)
    n = len(R)
    ranges = np.zeros((max(n, 1), 2), dtype=np.float32)
    n_list, n_pairs, why = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_char_p()
    counters = np.zeros(3, dtype=np.uint64)
    rc = (L.dsm_ss_host_run_serial if serial else L.dsm_ss_host_run)(
        ctypes.byref(o), n, R.ctypes.data, T.ctypes.data, len(xyz), xyz.ctypes.data, offs.ctypes.data, idx.ctypes.data,
        None if mask is None else mask.ctypes.data, ranges.ctypes.data, ctypes.byref(n_list), ctypes.byref(n_pairs), counters.ctypes.data,
        ctypes.byref(why))
    if rc != 0:
        err = DsmError("dsm_ss_host_run failed (%d): %s" % (rc, (why.value or b"").decode()))
        err.rc = rc
        raise err
    loff = np.zeros(n + 1, dtype=np.uint64)
    limg = np.zeros(max(int(n_list.value), 1), dtype=np.uint32)
    rec = np.zeros(max(int(n_pairs.value), 1), dtype=IMAGE_OVERLAP_DTYPE)
    L.dsm_ss_host_get(loff.ctypes.data, limg.ctypes.data, rec.ctypes.data)
    stats = {"items": int(counters[0]), "pairs": int(counters[1]), "nan_items": int(counters[2])}
    return _selection_result(n, ranges, loff, limg, rec[:int(n_pairs.value)], stats)


def parse_patch_match_config(lines, image_names):
    """patch-match.cfg as PatchMatchController::ReadProblems reads it (src/mvs/patch_match.cc:284-305): lines are trimmed, blank
    lines and lines that start with `#` are skipped, and the rest alternate between a reference image's name and its source
    specification -- `__all__`, `__auto__, N`, or a comma-separated list of image names.  A reference name without a
    specification after it is dropped, as in the reference.  image_names: the model's names in index order.
    -> a list of (ref_index, spec) with spec = ("all",), ("auto", N) or ("list", [indices])."""
    index = {name: i for i, name in enumerate(image_names)}

    def image(name):
        if name not in index:
            raise DsmError("patch-match.cfg names an image the model does not have: %r" % name)
        return index[name]

    out, ref = [], None
    for line in lines:
        line = line.strip()
        if not line or line[0] == "#":
            continue
        if ref is None:
            ref = line
            continue
        names = [v.strip() for v in line.split(",")]  # CSVToVector<std::string>: split at commas, trimmed, empty fields dropped
        names = [v for v in names if v]
        if len(names) == 1 and names[0] == "__all__":
            spec = ("all",)
        elif len(names) == 2 and names[0] == "__auto__":
            spec = ("auto", int(names[1]))
        else:
            spec = ("list", [image(v) for v in names])
        out.append((image(ref), spec))
        ref = None
    return out


def patch_match_problems_from(selection, config, depth_min=-1.0, depth_max=-1.0):
    """ReadProblems' second loop (patch_match.cc:307-388) and the depth limits of ProcessProblem (:455-464) over the results of a
    source selection run with the mask of the configured reference images: -> [(ref, src_images, depth_min, depth_max)], what
    Context.patch_match_stereo takes.  `__all__`: the other configured reference images -- the reference iterates an
    std::unordered_set there, whose order is unspecified; this binding's order is ascending image index.  `__auto__, N`: the
    first N of the selection's list.  A reference image whose source list is empty is dropped.  depth_min / depth_max: the
    options' values; a negative one is replaced by the image's depth range."""
    refs = sorted({ref for ref, _ in config})
    out = []
    for ref, spec in config:
        if spec[0] == "all":
            src = [i for i in refs if i != ref]
        elif spec[0] == "auto":
            src = list(selection["sources"][ref][:max(int(spec[1]), 0)])
        else:
            src = list(spec[1])
        if not src:
            continue
        lo = float(depth_min) if depth_min >= 0 else float(selection["depth_ranges"][ref][0])
        hi = float(depth_max) if depth_max >= 0 else float(selection["depth_ranges"][ref][1])
        out.append((ref, src, lo, hi))
    return out


def patch_match_selection_arguments(config, n_images):
    """(candidate_mask, max_num_src_images) of the source selection ReadProblems needs for `config`: the mask of the configured
    reference images (ref_image_idxs) and the largest N of its `__auto__, N` entries."""
    mask = np.zeros(n_images, dtype=np.uint8)
    for ref, _ in config:
        mask[ref] = 1
    autos = [int(spec[1]) for _, spec in config if spec[0] == "auto"]
    return mask, max([0] + autos)


def write_fused_ply(path, points, normals, colours):
    """WriteBinaryPlyPoints (src/util/ply.cc:329-381) with normals and colours: its header, then per point x, y, z, nx, ny, nz
    as little-endian floats and red, green, blue as bytes -- stereo_fusion's fused.ply."""
    points = np.asarray(points, dtype="<f4").reshape(-1, 3)
    normals = np.asarray(normals, dtype="<f4").reshape(-1, 3)
    colours = np.asarray(colours, dtype=np.uint8).reshape(-1, 3)
    assert len(points) == len(normals) == len(colours)
    rec = np.zeros(len(points), dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    rec["p"], rec["n"], rec["c"] = points, normals, colours
    header = ["ply", "format binary_little_endian 1.0", "element vertex %d" % len(points)]
    header += ["property float %s" % k for k in ("x", "y", "z", "nx", "ny", "nz")]
    header += ["property uchar %s" % k for k in ("red", "green", "blue")] + ["end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(rec.tobytes())


def read_fused_ply(path):
    """What write_fused_ply wrote -> (points [N][3], normals [N][3] float32, colours [N][3] uint8)."""
    with open(path, "rb") as f:
        blob = f.read()
    end = blob.index(b"end_header\n") + len(b"end_header\n")
    header = blob[:end].decode("ascii").split("\n")
    n = int([h for h in header if h.startswith("element vertex")][0].split()[2])
    rec = np.frombuffer(blob[end:], dtype=np.dtype([("p", "<f4", 3), ("n", "<f4", 3), ("c", "u1", 3)]))
    if len(rec) != n:
        raise DsmError("%s: %d vertices announced, %d found" % (path, n, len(rec)))
    return rec["p"].copy(), rec["n"].copy(), rec["c"].copy()


def write_points_visibility(path, visibility):
    """WritePointsVisibility (src/mvs/fusion.cc:475-489, the format of fusion.h:160-171): the number of points as uint64, then
    per point its number of images and their indices as uint32, little endian -- fused.ply.vis."""
    with open(path, "wb") as f:
        f.write(np.array([len(visibility)], dtype="<u8").tobytes())
        for v in visibility:
            f.write(np.array([len(v)] + [int(i) for i in v], dtype="<u4").tobytes())


def read_points_visibility(path):
    """What write_points_visibility wrote -> a list of lists of image indices."""
    with open(path, "rb") as f:
        blob = f.read()
    n = int(np.frombuffer(blob[:8], dtype="<u8")[0])
    words = np.frombuffer(blob[8:], dtype="<u4")
    out, at = [], 0
    for _ in range(n):
        k = int(words[at])
        out.append(words[at + 1:at + 1 + k].tolist())
        at += 1 + k
    if at != len(words):
        raise DsmError("%s: trailing data" % path)
    return out


def _fusion_call_arguments(images, overlap):
    """The dsm_fusion_image array and the overlap lists of a fusion call from image dicts: used, depth [h][w], normal [3][h][w]
    float32, rgb [bh][bw][3] uint8 (any row stride), P [12], inv_P [12], inv_R [9]; scale [2] defaults to the reference's
    float(width) / bitmap_width (fusion.cc:216-218).  An unused image needs no other key.  -> (array, offsets, indices, keep)."""
    arr = (FusionImage * max(len(images), 1))()
    keep = []
    for i, im in enumerate(images):
        a = arr[i]
        a.used = 1 if im.get("used", True) else 0
        if not a.used and "depth" not in im:
            continue
        depth = np.ascontiguousarray(im["depth"], dtype=np.float32)
        normal = np.ascontiguousarray(im["normal"], dtype=np.float32)
        rgb = np.asarray(im["rgb"], dtype=np.uint8)
        assert depth.ndim == 2 and normal.shape == (3,) + depth.shape and rgb.ndim == 3 and rgb.shape[2] == 3
        if rgb.strides[2] != 1 or rgb.strides[1] != 3:
            rgb = np.ascontiguousarray(rgb)
        keep += [depth, normal, rgb]
        a.height, a.width = depth.shape
        a.bitmap_height, a.bitmap_width = rgb.shape[:2]
        a.row_stride = im.get("row_stride", rgb.strides[0])
        a.depth_map, a.normal_map, a.rgb = depth.ctypes.data, normal.ctypes.data, rgb.ctypes.data
        a.P[:] = np.asarray(im["P"], dtype=np.float32).reshape(12).tolist()
        a.inv_P[:] = np.asarray(im["inv_P"], dtype=np.float32).reshape(12).tolist()
        a.inv_R[:] = np.asarray(im["inv_R"], dtype=np.float32).reshape(9).tolist()
        scale = im.get("scale")
        if scale is None:
            scale = (np.float32(a.width) / np.float32(a.bitmap_width), np.float32(a.height) / np.float32(a.bitmap_height))
        a.bitmap_scale[:] = [float(np.float32(scale[0])), float(np.float32(scale[1]))]
    assert len(overlap) == len(images), "one overlap list per image"
    offs = np.zeros(len(images) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(v) for v in overlap])
    idx = np.array([int(i) for v in overlap for i in v] + [0], dtype=np.int64)
    assert idx.min() >= 0 and idx.max() < 2 ** 32
    idx = idx.astype(np.uint32)
    keep += [offs, idx]
    return arr, offs, idx, keep


def fusion_host_lib():
    """libdsm_stereo_fusion_host.so, the host build of csrc/stereo_fusion.h; raises if it has not been built."""
    if "fusion_host" not in _libs:
        if not os.path.exists(FUSION_HOST_LIB_PATH):
            raise DsmError("%s is missing: run make -C dagsfm_amd/csrc" % FUSION_HOST_LIB_PATH)
        L = ctypes.CDLL(FUSION_HOST_LIB_PATH)
        vp = ctypes.c_void_p
        L.dsm_fusion_host_run.argtypes = [ctypes.POINTER(StereoFusionOptions), ctypes.c_uint32, vp, vp, vp, u64p, u64p, ctypes.POINTER(ctypes.c_char_p)]
        L.dsm_fusion_host_get.argtypes = [vp, vp, vp]
        L.dsm_fusion_host_get.restype = None
        L.dsm_fusion_host_default_options.argtypes = [ctypes.POINTER(StereoFusionOptions)]
        L.dsm_fusion_host_default_options.restype = None
        _libs["fusion_host"] = L
    return _libs["fusion_host"]


def fusion_host(images, overlap, options=None, **kw):
    """StereoFusion::Run on one CPU thread by the host build of the kernels' header (no GPU, no context).  The arguments and
    the first four results are Context.stereo_fusion's; then the final masks of all used images back to back and the number
    of seed traversals."""
    L = fusion_host_lib()
    assert options is None or not kw, "pass a StereoFusionOptions or keywords, not both"
    o = options
    if o is None:
        o = StereoFusionOptions()
        L.dsm_fusion_host_default_options(ctypes.byref(o))
        for k, v in kw.items():
            assert hasattr(o, k), k
            setattr(o, k, v)
    arr, offs, idx, keep = _fusion_call_arguments(images, overlap)
    n, trav, why = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_char_p()
    rc = L.dsm_fusion_host_run(ctypes.byref(o), len(images), ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, ctypes.byref(n),
                               ctypes.byref(trav), ctypes.byref(why))
    if rc != 0:
        err = DsmError("dsm_fusion_host_run failed (%d): %s" % (rc, (why.value or b"").decode()))
        err.rc = rc
        raise err
    n = int(n.value)
    words = (len(images) + 31) // 32
    rec = np.zeros(max(n, 1), dtype=FUSED_POINT_DTYPE)
    bits = np.zeros((max(n, 1), max(words, 1)), dtype=np.uint32)
    total = sum(int(a.width) * int(a.height) for a in arr[:len(images)] if a.used)
    masks = np.zeros(max(total, 1), dtype=np.uint8)
    L.dsm_fusion_host_get(rec.ctypes.data, bits.ctypes.data, masks.ctypes.data)
    vis = [[i for i in range(len(images)) if int(bits[k, i // 32]) >> (i % 32) & 1] for k in range(n)]
    rec = rec[:n]
    return rec["xyz"].copy(), rec["rgb"].copy(), rec["normal"].copy(), vis, masks[:total], int(trav.value)


def default_initial_pair_options(**kw):
    o = InitialPairOptions()
    lib().dsm_default_initial_pair_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _initial_pair_problem_arguments(scene, problems):
    """The problems of find_initial_pairs as the C arrays: offsets, ids, num_registrations, init_num_reg_trials, tried offsets and
    pairs, the two seeds; and the bounds of the outputs (tried pairs, points)."""
    ids, regs, trials, tried, poff, toff, s1, s2 = [], [], [], [], [0], [0], [], []
    for pr in problems:
        im = [int(x) for x in pr["image_ids"]]
        ids += im
        regs += [int(x) for x in pr.get("num_registrations", [0] * len(im))]
        trials += [int(x) for x in pr.get("init_num_reg_trials", [0] * len(im))]
        tried += [int(x) for t in pr.get("tried_pairs", []) for x in t]
        poff.append(len(ids))
        toff.append(len(tried) // 2)
        s1.append(NO_IMAGE if pr.get("seed_image1") is None else int(pr["seed_image1"]))
        s2.append(NO_IMAGE if pr.get("seed_image2") is None else int(pr["seed_image2"]))
    if len(regs) != len(ids) or len(trials) != len(ids):
        raise DsmError("find_initial_pairs: num_registrations and init_num_reg_trials must align with a problem's image_ids")
    pairs = np.ascontiguousarray(scene["pairs"], np.int64).reshape(-1, 2)
    counts = np.diff(np.ascontiguousarray(scene["match_offsets"], np.int64))
    max_tried, max_points = 0, 0
    for pr in problems:
        inside = np.isin(pairs[:, 0], pr["image_ids"]) & np.isin(pairs[:, 1], pr["image_ids"]) if len(pairs) else np.zeros(0, bool)
        max_tried += max(int(inside.sum()), 1)
        max_points += int(counts[inside].max()) if inside.any() else 0
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)
    return (u32(poff), u32(ids), u32(regs), u32(trials), np.ascontiguousarray(toff, np.uint64), u32(tried + [0, 0]), u32(s1), u32(s2),
            max_tried, max_points)


def initial_pair_host_lib():
    """libdsm_initial_pair_host.so: the host build of csrc/initial_pair.h (the candidate order, the angle, Median, the gates)."""
    if "initial_pair_host" not in _libs:
        if not os.path.exists(INITIAL_PAIR_HOST_LIB_PATH):
            raise DsmError("%s is missing: run make -C dagsfm_amd/csrc" % INITIAL_PAIR_HOST_LIB_PATH)
        L = ctypes.CDLL(INITIAL_PAIR_HOST_LIB_PATH)
        vp, dbl = ctypes.c_void_p, ctypes.c_double
        L.dsm_ip_host_acos.argtypes, L.dsm_ip_host_acos.restype = [dbl], dbl
        L.dsm_ip_host_default_options.argtypes, L.dsm_ip_host_default_options.restype = [ctypes.POINTER(InitialPairOptions)], None
        L.dsm_ip_host_min_tri_angle_rad.argtypes, L.dsm_ip_host_min_tri_angle_rad.restype = [dbl], dbl
        L.dsm_ip_host_tri_angle.argtypes, L.dsm_ip_host_tri_angle.restype = [vp, vp, vp], dbl
        L.dsm_ip_host_median.argtypes, L.dsm_ip_host_median.restype = [vp, ctypes.c_uint64], dbl
        L.dsm_ip_host_pose.argtypes, L.dsm_ip_host_pose.restype = [vp] * 5, None
        L.dsm_ip_host_accept.argtypes = [ctypes.c_uint32, dbl, dbl, ctypes.POINTER(InitialPairOptions), vp]
        L.dsm_ip_host_point_gates.argtypes = [vp, vp, vp, dbl, vp, vp]
        L.dsm_ip_host_candidates.argtypes = ([ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32, vp, vp, vp, ctypes.c_uint32] + [vp] * 8
                                             + [ctypes.POINTER(InitialPairOptions), ctypes.c_int, vp, vp, ctypes.c_uint64, vp,
                                                ctypes.POINTER(ctypes.c_char_p)])
        _libs["initial_pair_host"] = L
    return _libs["initial_pair_host"]


def initial_pair_host_candidates(scene, problems, options=None, sorted_schedule=False):
    """The candidate lists of find_initial_pairs from the host build: per problem a list of (image_id1, image_id2) in trial order,
    and the matches every pair keeps after the duplicate rule.  sorted_schedule: the device's packed keys instead of the
    reference's nested loops.  Raises DsmError with the library's message on invalid arguments."""
    L = initial_pair_host_lib()
    o = options if options is not None else default_initial_pair_options()
    a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
    cam_of = {int(c): k for k, c in enumerate(a("camera_ids", np.uint32))}
    img_ids, img_cam = a("image_ids", np.uint32), a("image_camera_ids", np.uint32)
    prior = np.array([scene["cameras"][cam_of[int(c)]].has_prior_focal_length != 0 for c in img_cam], np.uint8)
    poff = a("points2D_offsets", np.uint32)
    pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
    prob_off, prob_ids, regs, trials, toff, tried, s1, s2, max_tried, _ = _initial_pair_problem_arguments(scene, problems)
    out_off = np.zeros(len(problems) + 1, np.uint64)
    out = np.zeros((max(max_tried, 1), 2), np.uint32)
    cnt = np.zeros(max(len(pairs), 1), np.uint32)
    why = ctypes.c_char_p()
    ptr = lambda x: x.ctypes.data
    rc = L.dsm_ip_host_candidates(len(img_ids), ptr(img_ids), ptr(prior), ptr(poff), len(pairs), ptr(pairs), ptr(moff), ptr(m), len(problems),
                                  ptr(prob_off), ptr(prob_ids), ptr(regs), ptr(trials), ptr(toff), ptr(tried), ptr(s1), ptr(s2), ctypes.byref(o),
                                  int(bool(sorted_schedule)), ptr(out_off), ptr(out), len(out), ptr(cnt), ctypes.byref(why))
    if rc != 0:
        raise DsmError("dsm_ip_host_candidates failed (%d): %s" % (rc, (why.value or b"").decode()))
    lists = [[(int(x), int(y)) for x, y in out[int(out_off[k]):int(out_off[k + 1])]] for k in range(len(problems))]
    return lists, cnt[:len(pairs)].copy()


def default_next_images_options(**kw):
    o = NextImagesOptions()
    lib().dsm_default_next_images_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _next_images_arguments(scene, problems):
    """The arguments dsm_find_next_images and its host build share, as the C arrays (kept alive by the returned list), and the
    number of slots.  scene: the dict of find_initial_pairs.  problems: a list of dicts with image_ids, registered (0 / 1 per
    image), obs_point3D (one int32 array per image: the point of every point2D or -1) and, optionally, num_reg_trials and
    filtered (per image), obs_offsets (the slots' running sum over the whole call, overriding the one computed here)."""
    a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
    cam_ids = a("camera_ids", np.uint32)
    cams = (Camera * max(len(cam_ids), 1))(*scene["cameras"])
    img_ids, img_cam = a("image_ids", np.uint32), a("image_camera_ids", np.uint32)
    poff, xy = a("points2D_offsets", np.uint32), a("points2D_xy", np.float64, (-1, 2))
    pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
    ids, reg, trials, filt, obs, prob_off, obs_off = [], [], [], [], [], [0], [0]
    for pr in problems:
        im = [int(x) for x in pr["image_ids"]]
        ids += im
        reg += [int(x) for x in pr["registered"]]
        trials += [int(x) for x in pr.get("num_reg_trials", [0] * len(im))]
        filt += [int(x) for x in pr.get("filtered", [0] * len(im))]
        for o3 in pr["obs_point3D"]:
            obs.append(np.ascontiguousarray(o3, np.int32).reshape(-1))
            obs_off.append(obs_off[-1] + len(obs[-1]))
        prob_off.append(len(ids))
    if not (len(reg) == len(trials) == len(filt) == len(ids) == len(obs_off) - 1):
        raise DsmError("find_next_images: registered, num_reg_trials, filtered and obs_point3D must align with a problem's image_ids")
    for pr in problems:
        if "obs_offsets" in pr:
            obs_off = list(pr["obs_offsets"])
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)
    arrays = [cam_ids, cams, img_ids, img_cam, poff, xy, pairs, moff, m, u32(prob_off), u32(ids + [0]), np.ascontiguousarray(reg + [0], np.uint8),
              np.ascontiguousarray(obs_off, np.uint64), np.concatenate(obs + [np.zeros(1, np.int32)]), u32(trials + [0]),
              np.ascontiguousarray(filt + [0], np.uint8)]
    ptr = lambda x: ctypes.addressof(x) if isinstance(x, ctypes.Array) else x.ctypes.data
    args = [len(cam_ids), ptr(cam_ids), ptr(cams), len(img_ids), ptr(img_ids), ptr(img_cam), ptr(poff), ptr(xy), len(pairs), ptr(pairs), ptr(moff),
            ptr(m), len(problems)] + [ptr(x) for x in arrays[9:]]
    return args, arrays, len(ids)


def _next_images_result(problems, n_slots, off, out, nv, no, score):
    res, s = [], 0
    for k, pr in enumerate(problems):
        n = len(pr["image_ids"])
        res.append({"next_image_ids": [int(x) for x in out[int(off[k]):int(off[k + 1])]], "num_visible": nv[s:s + n].copy(),
                    "num_observations": no[s:s + n].copy(), "score": score[s:s + n].copy()})
        s += n
    return res


def _track_update_options(L, default_name, kw):
    """A TrackUpdateOptions with library L's defaults: the struct's own fields by name, any other keyword a field of `tri`."""
    o = TrackUpdateOptions()
    getattr(L, default_name)(ctypes.byref(o))
    own = {k for k, _ in TrackUpdateOptions._fields_}
    for k, v in kw.items():
        setattr(o if k in own else o.tri, k, v)
    return o


def default_track_update_options(**kw):
    """complete_max_reproj_error, merge_max_reproj_error, complete_max_transitivity by name; any other keyword is a field of `tri`."""
    return _track_update_options(lib(), "dsm_default_track_update_options", kw)


def track_update_host_lib():
    """libdsm_track_update_host.so: the host build of csrc/track_update.h (dsm_update_tracks on one CPU thread)."""
    if "track_update_host" not in _libs:
        if not os.path.exists(TRACK_UPDATE_HOST_LIB_PATH):
            raise DsmError("%s is missing: run make -C dagsfm_amd/csrc" % TRACK_UPDATE_HOST_LIB_PATH)
        L = ctypes.CDLL(TRACK_UPDATE_HOST_LIB_PATH)
        L.dsm_tu_host_default_options.argtypes, L.dsm_tu_host_default_options.restype = [ctypes.POINTER(TrackUpdateOptions)], None
        L.dsm_tu_host_update_tracks.argtypes = _TRACK_UPDATE_ARGTYPES
        _libs["track_update_host"] = L
    return _libs["track_update_host"]


def _update_tracks(call, scene, steps, selected, next_point3D_id, options, complete_images=None):
    """The marshalling dsm_update_tracks, its host build and dsm_complete_images share.  call(args) -> the return code.
    complete_images: the image ids of dsm_complete_images (None: the other two)."""
    a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
    cam_ids = a("camera_ids", np.uint32)
    cams = (Camera * max(len(cam_ids), 1))(*scene["cameras"])
    img_ids, img_cam, reg = a("image_ids", np.uint32), a("image_camera_ids", np.uint32), a("registered", np.uint8)
    N = len(img_ids)
    qvec, tvec = a("qvec", np.float64, (N, 4)), a("tvec", np.float64, (N, 3))
    poff, xy = a("points2D_offsets", np.uint32), a("points2D_xy", np.float64, (-1, 2))
    pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
    pids, pxyz = a("point3D_ids", np.uint64), a("point3D_xyz", np.float64, (-1, 3))
    toff, tobs = a("track_offsets", np.uint64), a("track_obs", np.uint32, (-1, 2))
    st = np.ascontiguousarray(steps, np.int32).reshape(-1)
    sel = None if selected is None else np.ascontiguousarray(selected, np.uint64).reshape(-1)
    P, T = len(pids), int(poff[-1]) if len(poff) else 0
    ci = None if complete_images is None else np.ascontiguousarray(complete_images, np.uint32).reshape(-1)
    R = P + (T if ci is not None else 0)  # room of the point arrays: every point2D of a listed image can add a point
    oid, oxyz, ooff = np.zeros(max(R, 1), np.uint64), np.zeros((max(R, 1), 3)), np.zeros(R + 1, np.uint64)
    oobs, omod, counts = np.zeros((max(T, 1), 2), np.uint32), np.zeros(max(R, 1), np.uint64), np.zeros(max(len(st), 1), np.uint64)
    n, nm = ctypes.c_uint64(0), ctypes.c_uint64(0)
    rep = TrackUpdateReport() if ci is None else CompleteImagesReport()
    o = options if options is not None else default_track_update_options()
    ptr = lambda x: x.ctypes.data
    args = [len(cam_ids), ptr(cam_ids), ctypes.addressof(cams), N, ptr(img_ids), ptr(img_cam), ptr(reg), ptr(qvec), ptr(tvec),
            ptr(poff), ptr(xy), len(pairs), ptr(pairs), ptr(moff), ptr(m), P, ptr(pids), ptr(pxyz), ptr(toff), ptr(tobs),
            len(st), ptr(st), 0 if sel is None else len(sel), None if sel is None else ptr(sel), int(next_point3D_id)]
    tris = None
    if ci is not None:
        tris = np.zeros(max(len(ci), 1), np.uint64)
        args += [len(ci), ptr(ci)]
    args += [ctypes.byref(o), ctypes.addressof(n), ptr(oid), ptr(oxyz), ptr(ooff), ptr(oobs), ctypes.addressof(nm), ptr(omod), ptr(counts)]
    if ci is not None:
        args.append(ptr(tris))
    rc = call(args + [ctypes.addressof(rep)])
    k = n.value
    out = {"point_ids": oid[:k].copy(), "xyz": oxyz[:k].copy(), "track_offsets": ooff[:k + 1].copy(),
           "track_obs": oobs[:int(ooff[k])].copy(), "modified": omod[:nm.value].copy(), "step_counts": counts[:len(st)].copy(),
           "report": rep}
    if ci is not None:
        out["image_num_tris"] = tris[:len(ci)].copy()
    return rc, out


def update_tracks_host(scene, steps, selected=None, next_point3D_id=0, options=None, **kw):
    """dsm_update_tracks from the host build on one CPU thread; the dict Context.update_tracks returns."""
    assert options is None or not kw, "pass a TrackUpdateOptions or keywords, not both"
    L = track_update_host_lib()
    if options is None:
        options = _track_update_options(L, "dsm_tu_host_default_options", kw)
    rc, out = _update_tracks(lambda args: L.dsm_tu_host_update_tracks(*args), scene, steps, selected, next_point3D_id, options)
    if rc != 0:
        raise DsmError("dsm_tu_host_update_tracks failed (%d)" % rc)
    return out


def apply_track_update(scene, result):
    """The scene with the result of update_tracks written back: point3D_ids, point3D_xyz, track_offsets, track_obs replaced, and
    points2D_point3D (the index of every point2D's point in the new point list, or -1) as dsm_retriangulate_pairs takes it.
    bundle_arrays(scene) gives the arrays dsm_filter_points3D and dsm_bundle_adjust take."""
    out = dict(scene)
    out["point3D_ids"], out["point3D_xyz"] = result["point_ids"].copy(), result["xyz"].copy()
    out["track_offsets"], out["track_obs"] = result["track_offsets"].copy(), result["track_obs"].copy()
    poff = np.asarray(scene["points2D_offsets"], np.int64).reshape(-1)
    img_of = {int(i): k for k, i in enumerate(np.asarray(scene["image_ids"]).reshape(-1))}
    p3 = np.full(int(poff[-1]) if len(poff) else 0, -1, np.int32)
    toff = np.asarray(result["track_offsets"], np.int64)
    owner = np.repeat(np.arange(len(toff) - 1), toff[1:] - toff[:-1])
    for (im, idx), p in zip(np.asarray(result["track_obs"], np.int64).reshape(-1, 2), owner):
        p3[poff[img_of[int(im)]] + idx] = p
    out["points2D_point3D"] = p3
    return out


def bundle_arrays(scene):
    """The point arrays of a track scene as dsm_bundle_adjust and dsm_filter_points3D take them: xyz, track_offsets, obs_image
    (image index) and obs_xy per track element."""
    poff = np.asarray(scene["points2D_offsets"], np.int64).reshape(-1)
    xy = np.asarray(scene["points2D_xy"], np.float64).reshape(-1, 2)
    img_of = {int(i): k for k, i in enumerate(np.asarray(scene["image_ids"]).reshape(-1))}
    tobs = np.asarray(scene["track_obs"], np.int64).reshape(-1, 2)
    oimg = np.array([img_of[int(i)] for i in tobs[:, 0]], np.uint32)
    return {"xyz": np.asarray(scene["point3D_xyz"], np.float64).reshape(-1, 3).copy(),
            "track_offsets": np.asarray(scene["track_offsets"], np.uint32).copy(), "obs_image": oimg,
            "obs_xy": xy[poff[oimg.astype(np.int64)] + tobs[:, 1]].reshape(-1, 2).copy()}


def next_images_host_lib():
    """libdsm_next_images_host.so: the host build of csrc/next_images.h (the cell, the score, the rank key, the whole call)."""
    if "next_images_host" not in _libs:
        if not os.path.exists(NEXT_IMAGES_HOST_LIB_PATH):
            raise DsmError("%s is missing: run make -C dagsfm_amd/csrc" % NEXT_IMAGES_HOST_LIB_PATH)
        L = ctypes.CDLL(NEXT_IMAGES_HOST_LIB_PATH)
        vp = ctypes.c_void_p
        L.dsm_ni_host_default_options.argtypes, L.dsm_ni_host_default_options.restype = [ctypes.POINTER(NextImagesOptions)], None
        L.dsm_ni_host_cell.argtypes, L.dsm_ni_host_cell.restype = [ctypes.c_double, ctypes.c_uint64], ctypes.c_uint32
        L.dsm_ni_host_score.argtypes, L.dsm_ni_host_score.restype = [vp, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_uint64
        L.dsm_ni_host_rank.argtypes, L.dsm_ni_host_rank.restype = [ctypes.c_int32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64], ctypes.c_float
        L.dsm_ni_host_key.argtypes, L.dsm_ni_host_key.restype = [ctypes.c_uint32, ctypes.c_int, ctypes.c_float, ctypes.c_uint32], ctypes.c_uint64
        L.dsm_lb_host_default_options.argtypes, L.dsm_lb_host_default_options.restype = [ctypes.POINTER(LocalBundleSelectionOptions)], None
        L.dsm_lb_host_percentile_index.argtypes, L.dsm_lb_host_percentile_index.restype = [ctypes.c_uint64], ctypes.c_uint64
        L.dsm_lb_host_percentile.argtypes, L.dsm_lb_host_percentile.restype = [vp, ctypes.c_uint64], ctypes.c_double
        L.dsm_lb_host_find_local_bundles.argtypes = _LOCAL_BUNDLES_ARGTYPES + [vp, ctypes.POINTER(ctypes.c_char_p)]
        L.dsm_ni_host_find_next_images.argtypes = (_NEXT_IMAGES_SCENE_ARGTYPES + [ctypes.POINTER(NextImagesOptions), ctypes.c_int, vp, vp,
                                                                                  ctypes.c_uint64, vp, vp, vp, ctypes.POINTER(ctypes.c_char_p)])
        _libs["next_images_host"] = L
    return _libs["next_images_host"]


def next_images_host(scene, problems, options=None, sorted_schedule=False, capacity=None, **kw):
    """dsm_find_next_images from the host build on one CPU thread: the list find_next_images returns, without the report.
    sorted_schedule: the device's packed keys under a sort instead of the sequential selection.  Raises DsmError with the
    library's message on invalid arguments."""
    L = next_images_host_lib()
    if options is None:
        options = NextImagesOptions()
        L.dsm_ni_host_default_options(ctypes.byref(options))
        for k, v in kw.items():
            setattr(options, k, v)
    args, keep, S = _next_images_arguments(scene, problems)
    B = len(problems)
    off, out = np.zeros(B + 1, np.uint64), np.zeros(max(S if capacity is None else capacity, 1), np.uint32)
    nv, no, score = np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint64)
    why = ctypes.c_char_p()
    ptr = lambda x: x.ctypes.data
    rc = L.dsm_ni_host_find_next_images(*args, ctypes.byref(options), int(bool(sorted_schedule)), ptr(off), ptr(out),
                                        S if capacity is None else capacity, ptr(nv), ptr(no), ptr(score), ctypes.byref(why))
    if rc != 0:
        e = DsmError("dsm_ni_host_find_next_images failed (%d): %s" % (rc, (why.value or b"").decode()))
        e.code, e.outputs = rc, (off, out, nv, no, score)
        raise e
    return _next_images_result(problems, S, off, out, nv, no, score)


def default_local_bundle_selection_options(**kw):
    o = LocalBundleSelectionOptions()
    lib().dsm_default_local_bundle_selection_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _local_bundles_arguments(scene, problems, queries, capacities):
    """The arguments dsm_find_local_bundles and its host build share (from num_images to the overlap capacity, the options
    left out), the arrays that keep them alive, and the outputs.  scene: image_ids and points2D_offsets are read.  problems: as
    find_next_images takes them, with qvec [n, 4] and tvec [n, 3] per image (read for registered images) and point_xyz [m, 3].
    queries: [(problem index, image id)]."""
    a = lambda key, dt: np.ascontiguousarray(scene[key], dt).reshape(-1)
    img_ids, poff = a("image_ids", np.uint32), a("points2D_offsets", np.uint32)
    ids, reg, obs, qv, tv, xyz, prob_off, obs_off, pt_off = [], [], [], [], [], [], [0], [0], [0]
    for pr in problems:
        im = [int(x) for x in pr["image_ids"]]
        ids += im
        reg += [int(x) for x in pr["registered"]]
        for o3 in pr["obs_point3D"]:
            obs.append(np.ascontiguousarray(o3, np.int32).reshape(-1))
            obs_off.append(obs_off[-1] + len(obs[-1]))
        qv.append(np.asarray(pr.get("qvec", np.tile([1.0, 0, 0, 0], (len(im), 1))), np.float64).reshape(-1, 4))
        tv.append(np.asarray(pr.get("tvec", np.zeros((len(im), 3))), np.float64).reshape(-1, 3))
        xyz.append(np.asarray(pr.get("point_xyz", np.zeros((0, 3))), np.float64).reshape(-1, 3))
        prob_off.append(len(ids))
        pt_off.append(pt_off[-1] + len(xyz[-1]))
    if not (len(reg) == len(ids) == len(obs_off) - 1 == sum(len(x) for x in qv) == sum(len(x) for x in tv)):
        raise DsmError("find_local_bundles: registered, obs_point3D, qvec and tvec must align with a problem's image_ids")
    for pr in problems:
        if "obs_offsets" in pr:
            obs_off = list(pr["obs_offsets"])
    u32 = lambda x: np.ascontiguousarray(x, np.uint32).reshape(-1)
    Q = len(queries)
    S_rows = sum(len(problems[p]["image_ids"]) for p, _ in queries if 0 <= p < len(problems))
    cap_b, cap_o = capacities
    out = [np.zeros(Q + 1, np.uint64), np.zeros(max(Q * 64 if cap_b is None else cap_b, 1), np.uint32), np.zeros(Q + 1, np.uint64),
           np.zeros(max(S_rows if cap_o is None else cap_o, 1), np.uint32), np.zeros(max(S_rows if cap_o is None else cap_o, 1), np.uint32),
           np.zeros(max(S_rows if cap_o is None else cap_o, 1), np.float64)]
    arrays = [img_ids, poff, u32(prob_off), u32(ids + [0]), np.ascontiguousarray(reg + [0], np.uint8), np.ascontiguousarray(obs_off, np.uint64),
              np.concatenate(obs + [np.zeros(1, np.int32)]), np.concatenate(qv + [np.zeros((1, 4))]), np.concatenate(tv + [np.zeros((1, 3))]),
              np.ascontiguousarray(pt_off, np.uint64), np.concatenate(xyz + [np.zeros((1, 3))]), u32([p for p, _ in queries] + [0]),
              u32([i for _, i in queries] + [0])]
    ptr = lambda x: x.ctypes.data
    head = [len(img_ids), ptr(arrays[0]), ptr(arrays[1]), len(problems)] + [ptr(x) for x in arrays[2:11]] + [Q, ptr(arrays[11]), ptr(arrays[12])]
    tail = [ptr(out[0]), ptr(out[1]), len(out[1]) if cap_b is None else cap_b, ptr(out[2]), ptr(out[3]), ptr(out[4]), ptr(out[5]),
            len(out[3]) if cap_o is None else cap_o]
    return head, tail, arrays, out


def _local_bundles_result(queries, out):
    boff, bids, ooff, oids, oshared, oangle = out
    res = []
    for k in range(len(queries)):
        b0, b1, o0, o1 = int(boff[k]), int(boff[k + 1]), int(ooff[k]), int(ooff[k + 1])
        res.append({"bundle_image_ids": [int(x) for x in bids[b0:b1]], "overlap_image_ids": [int(x) for x in oids[o0:o1]],
                    "overlap_shared": [int(x) for x in oshared[o0:o1]], "overlap_tri_angle": oangle[o0:o1].copy()})
    return res


def local_bundles_host(scene, problems, queries, options=None, bundle_capacity=None, overlap_capacity=None, **kw):
    """dsm_find_local_bundles from the host build on one CPU thread: (the list find_local_bundles returns as results, the
    smallest tri_angle margin).  Raises DsmError with the library's message on invalid arguments."""
    L = next_images_host_lib()
    if options is None:
        options = LocalBundleSelectionOptions()
        L.dsm_lb_host_default_options(ctypes.byref(options))
        for k, v in kw.items():
            setattr(options, k, v)
    head, tail, keep, out = _local_bundles_arguments(scene, problems, queries, (bundle_capacity, overlap_capacity))
    why, margin = ctypes.c_char_p(), ctypes.c_double(0.0)
    rc = L.dsm_lb_host_find_local_bundles(*head, ctypes.byref(options), *tail, ctypes.addressof(margin), ctypes.byref(why))
    if rc != 0:
        e = DsmError("dsm_lb_host_find_local_bundles failed (%d): %s" % (rc, (why.value or b"").decode()))
        e.code, e.outputs = rc, out
        raise e
    return _local_bundles_result(queries, out), margin.value


def default_vocabulary_build_options(**kw):
    o = VocabularyBuildOptions()
    lib().dsm_default_vocabulary_build_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def size_only_camera(width, height):
    """The dsm_camera that gives dsm_warp_images the size of an image of a warp without cameras (WarpImageWithHomography)."""
    return Camera(model_id=CAMERA_SIZE_ONLY, has_prior_focal_length=0, width=width, height=height)


def default_local_bundle_options(**kw):
    o = LocalBundleOptions()
    lib().dsm_default_local_bundle_options(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def local_bundle_problem(scene, image_id, local_bundle, variable_point_ids, fixed_image_ids=()):
    """Cuts the problem of IncrementalMapper::AdjustLocalBundle (src/sfm/incremental_mapper.cc:562-656) out of a reconstruction
    scene, exactly as BundleAdjuster::SetUp (src/optim/bundle_adjustment.cc:316-526) builds it.  Pure host code.

    scene: the dict of Context.bundle_adjust (image and point *indices* stand for the reference's ids; point_ids optional).
    image_id: the new image; local_bundle: its neighbours in FindLocalBundle's order (best connected first);
    variable_point_ids: indices of the points AddVariablePoint names -- the caller applies the selection of :611-619
    (`!HasError() || Track().Length() <= 15`), because it needs Point3D::error, which a scene does not carry;
    fixed_image_ids: the mapper's fix_existing_images path (:584-590): a neighbour listed there becomes constant-pose.

    - config images: image_id + local_bundle.  Gauge (:592-604): one neighbour -> its pose constant and tvec[0] of image_id
      constant; more -> the last neighbour's pose constant and tvec[0] of the one before it constant unless it is fixed.
    - every point seen from a config image enters with its observations in config images (AddImageToProblem);
    - a variable point additionally brings its observations from outside images as constant-pose images, whose cameras are
      camera_constant unless a config image with observations shares them (AddPointToProblem, :423-470);
    - a point that is not variable and whose track is not fully inside the problem is point_constant (ParameterizePoints);
      one whose track is fully inside stays variable.

    Returns a problem dict for Context.adjust_local_bundles (the scene layout plus camera_constant) with the maps back:
    image_index [n], camera_index [c], point_index [p] into the scene.  An empty local_bundle returns None (the mapper skips
    the adjustment)."""
    local_bundle = [int(i) for i in local_bundle]
    if not local_bundle:
        return None
    image_id = int(image_id)
    config = [image_id] + local_bundle
    if len(set(config)) != len(config):
        raise DsmError("local_bundle_problem: image_id and local_bundle must be distinct images")
    fixed = set(int(i) for i in fixed_image_ids)
    variable = set(int(p) for p in variable_point_ids)
    const_pose = set(i for i in local_bundle if i in fixed)
    const_tvec0 = set()
    if len(local_bundle) == 1:
        const_pose.add(local_bundle[0])
        const_tvec0.add(image_id)
    else:
        const_pose.add(local_bundle[-1])
        if local_bundle[-2] not in fixed:
            const_tvec0.add(local_bundle[-2])
    icam = np.asarray(scene["image_camera"], np.int64).reshape(-1)
    toff = np.asarray(scene["track_offsets"], np.int64).reshape(-1)
    oimg = np.asarray(scene["obs_image"], np.int64).reshape(-1)
    oxy = np.asarray(scene["obs_xy"], np.float64).reshape(-1, 2)
    P = len(toff) - 1
    in_config = np.zeros(len(icam), bool)
    in_config[config] = True
    images, img_new = [], {}

    def image_slot(i):
        if i not in img_new:
            img_new[i] = len(images)
            images.append(i)
        return img_new[i]

    for i in config:
        image_slot(i)
    points, tracks, pconst = [], [], []
    cams_with_config_obs = set()
    for p in range(P):
        el = range(int(toff[p]), int(toff[p + 1]))
        inside = [k for k in el if in_config[oimg[k]]]
        if not inside and p not in variable:
            continue  # (a variable point no config image sees enters through AddPointToProblem with constant poses only)
        for k in inside:
            cams_with_config_obs.add(int(icam[oimg[k]]))
        take = list(el) if p in variable else inside
        points.append(p)
        tracks.append(take)
        pconst.append(0 if len(take) == len(el) else 1)  # ParameterizePoints: Track().Length() > observations in the problem
    outside = []
    for take in tracks:
        for k in take:
            if not in_config[oimg[k]] and int(oimg[k]) not in img_new:
                outside.append(int(oimg[k]))
                image_slot(int(oimg[k]))
    cams, cam_new = [], {}
    for i in images:
        c = int(icam[i])
        if c not in cam_new:
            cam_new[c] = len(cams)
            cams.append(c)
    models = np.asarray(scene["camera_model_ids"], np.int32).reshape(-1)
    poff = np.concatenate([[0], np.cumsum([CAMERA_MODEL_NUM_PARAMS[m] for m in models])]).astype(np.int64)
    params = np.asarray(scene["camera_params"], np.float64).reshape(-1)
    qvec = np.asarray(scene["qvec"], np.float64).reshape(-1, 4)
    tvec = np.asarray(scene["tvec"], np.float64).reshape(-1, 3)
    xyz = np.asarray(scene["xyz"], np.float64).reshape(-1, 3)
    ids = np.asarray(scene["point_ids"], np.uint64).reshape(-1) if scene.get("point_ids") is not None else np.arange(P, dtype=np.uint64)
    cpose = np.array([1 if (i in const_pose or not in_config[i]) else 0 for i in images], np.uint8)
    cmask = np.array([1 if i in const_tvec0 else 0 for i in images], np.uint8)
    return {"camera_model_ids": models[cams].copy(),
            "camera_params": np.concatenate([params[poff[c]:poff[c + 1]] for c in cams]) if cams else np.zeros(0),
            "camera_constant": np.array([0 if c in cams_with_config_obs else 1 for c in cams], np.uint8),
            "image_camera": np.array([cam_new[int(icam[i])] for i in images], np.uint32),
            "qvec": qvec[images].copy(), "tvec": tvec[images].copy(), "image_constant_pose": cpose, "image_constant_tvec": cmask,
            "point_ids": ids[points].copy(), "xyz": xyz[points].copy(), "point_constant": np.array(pconst, np.uint8),
            "track_offsets": np.concatenate([[0], np.cumsum([len(t) for t in tracks])]).astype(np.uint32),
            "obs_image": np.array([img_new[int(oimg[k])] for t in tracks for k in t], np.uint32),
            "obs_xy": (np.concatenate([oxy[t] for t in tracks]) if tracks else np.zeros((0, 2))).reshape(-1, 2),
            "image_index": np.array(images, np.int64), "camera_index": np.array(cams, np.int64),
            "point_index": np.array(points, np.int64)}


def absolute_pose_seed(problem, factor_index, user_seed=0):
    return int(lib().dsm_absolute_pose_seed(problem, factor_index, user_seed))


def absolute_pose_factors(options=None):
    """The focal-length factors of pose.cc:87-102 for these options (what a problem with estimate_focal_length runs over)."""
    o = options if options is not None else default_absolute_pose_options()
    n = int(lib().dsm_absolute_pose_factors(ctypes.byref(o), None, 0))
    out = np.zeros(max(n, 1))
    lib().dsm_absolute_pose_factors(ctypes.byref(o), out.ctypes.data, n)
    return out[:n].copy()


def absolute_pose_max_trials(options=None):
    o = options if options is not None else default_absolute_pose_options()
    return int(lib().dsm_absolute_pose_max_trials(ctypes.byref(o)))


def align_seed(i, j, direction, user_seed=0):
    return int(lib().dsm_align_seed(i, j, direction, user_seed))


# the keys dsm_set_debug_option knows (csrc/ctx.h): scheduling knobs of the product, and the cross-check switches of the check build
PRODUCT_OPTION_KEYS = ("DSM_MATCH_CHUNK_ROWS", "DSM_VERIFY_CHUNK_PAIRS", "DSM_VERIFY_LANES", "DSM_VERIFY_INLINE_LO", "DSM_VERIFY_ITEM_MODE",
                       "DSM_LO_TAIL", "DSM_LO_TAIL_MODE", "DSM_VERIFY_GRID_DIV")
CHECK_OPTION_KEYS = ("DSM_K1_DOT4", "DSM_K1_RESOLVE_KERNEL", "DSM_VERIFY_DEBUG", "DSM_SAMPLER_SERIAL", "DSM_LO_PREPARE_WAVE", "DSM_LO_JACOBI_GROUPS", "DSM_ROOTS_LDS",
                     "DSM_FINAL_WAVES", "DSM_VERIFY_LEGACY", "DSM_VERIFY_FIXED_BATCH", "DSM_VERIFY_LANE_SPLIT", "DSM_DEBUG_SAMPLER_MODE",
                     "DSM_VOCAB_ASSIGN_VALU", "DSM_VERIFY_HOST_LOOP", "DSM_SCORE_PREFILTER", "DSM_VERIFY_REPLAY_GRID", "DSM_REPLAY_LEGACY", "DSM_FLANN_GROUP", "DSM_FLANN_STATS", "DSM_ELU_LDS", "DSM_HYP_GRID", "DSM_SPEC_MARGIN",
                     "DSM_POSE_FULL", "DSM_PATCH_MATCH_LANES", "DSM_NORMS_EXACT", "DSM_FUSION_SERIAL", "DSM_SOURCE_SELECTION_SERIAL",
                     "DSM_INITIAL_PAIR_SERIAL", "DSM_NEXT_IMAGES_SERIAL", "DSM_TRACK_UPDATE_SERIAL", "DSM_COMPLETE_IMAGE_SERIAL")
DEBUG_OPTION_KEYS = PRODUCT_OPTION_KEYS  # what a deployer's library knows


def check_requested():
    """True when the process environment carries a cross-check switch (or DSM_LIBRARY=check): contexts created now use the check build."""
    return os.environ.get("DSM_LIBRARY") == "check" or any(os.environ.get(k) is not None for k in CHECK_OPTION_KEYS)


class Context:
    """One context = one GPU (SiftFeatureMatcher + FeatureMatcherCache of the reference)."""

    def __init__(self, device=0, check=None):
        self._handle = ctypes.c_void_p()
        self._debug = {}
        self.check = check_requested() if check is None else bool(check)
        self._L = lib(self.check)
        rc = self._L.dsm_ctx_create(device, ctypes.byref(self._handle))
        if rc != 0:
            raise DsmError("dsm_ctx_create failed (%d): %s" % (rc, self._L.dsm_last_error(None).decode()))
        self.n_pairs = 0

    @property
    def _h(self):
        """The context handle.  The library itself never reads the environment (dsm_set_debug_option is the only way in);
        this TEST / TOOL binding forwards the DSM_* debug variables of the process to the context before every call, so
        that `DSM_VERIFY_LANES=1 python tools/...` and monkeypatch.setenv in the tests keep working."""
        if self._handle:
            for key in PRODUCT_OPTION_KEYS + CHECK_OPTION_KEYS:  # a check-only switch on a product context fails loudly
                want = os.environ.get(key)
                if self._debug.get(key) != want:
                    self.set_debug_option(key, want)
        return self._handle

    def set_memory_budget(self, nbytes):
        """dsm_ctx_set_memory_budget: bytes of transient chunk scratch the matcher and the verifier may hold (0: the defaults)."""
        self._L.dsm_ctx_set_memory_budget.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
        self._chk(self._L.dsm_ctx_set_memory_budget(self._handle, ctypes.c_uint64(int(nbytes))))

    def memory_footprint(self):
        """dsm_ctx_memory_footprint -> (resident_bytes, scratch_bytes) the context holds on the device right now."""
        r, s = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._L.dsm_ctx_memory_footprint.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
        self._chk(self._L.dsm_ctx_memory_footprint(self._handle, ctypes.byref(r), ctypes.byref(s)))
        return int(r.value), int(s.value)

    def set_debug_option(self, key, value):
        """dsm_set_debug_option: a scheduling / cross-check switch of this context (None removes it)."""
        L = self._L
        rc = L.dsm_set_debug_option(self._handle, key.encode(), None if value is None else str(value).encode())
        if rc != 0:
            raise DsmError("dsm_set_debug_option(%s) failed (%d)" % (key, rc))
        if value is None:
            self._debug.pop(key, None)
        else:
            self._debug[key] = str(value)

    def close(self):
        if self._handle:
            self._L.dsm_ctx_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise DsmError("dsm error %d: %s" % (rc, self._L.dsm_last_error(self._h).decode()))

    def sync(self):
        self._chk(self._L.dsm_sync(self._h))

    def append_images(self, descriptors, keypoints=None, cameras=None):
        """dsm_append_images: adds images behind the resident ones (indices continue), uploading only the new rows."""
        self.set_images(descriptors, keypoints, cameras, _append=True)

    def set_images(self, descriptors, keypoints=None, cameras=None, _append=False):
        """descriptors: list of (n_i,128) uint8; keypoints: list of (n_i,>=2) float32; cameras: list of Camera."""
        n = len(descriptors)
        descs = [np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 128) for d in descriptors]
        nf = np.array([d.shape[0] for d in descs], dtype=np.uint32)
        vp = ctypes.c_void_p
        dptr = (vp * max(n, 1))(*[d.ctypes.data for d in descs])
        kptr = None
        stride = 0
        kps = None
        if keypoints is not None:
            kps = [np.ascontiguousarray(k, dtype=np.float32) for k in keypoints]
            kps = [k.reshape(-1, k.shape[-1] if k.ndim == 2 else 2) for k in kps]
            stride = kps[0].shape[1] if n else 2
            for k, d in zip(kps, descs):
                assert k.shape[0] == d.shape[0] and k.shape[1] == stride
            kptr = (vp * max(n, 1))(*[k.ctypes.data for k in kps])
        cptr = None
        if cameras is not None:
            cptr = (Camera * max(n, 1))(*cameras)
        fn = self._L.dsm_append_images if _append else self._L.dsm_set_images
        fn.argtypes = self._L.dsm_set_images.argtypes
        self._chk(fn(self._h, n, nf.ctypes.data_as(u32p), dptr, kptr, stride, cptr))
        self._keep = (descs, kps)

    def match_pairs(self, pairs, options=None):
        options = options or default_match_options()
        p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        self.n_pairs = p.shape[0]
        self._chk(self._L.dsm_match_pairs(self._h, self.n_pairs, p.ctypes.data_as(u32p), ctypes.byref(options)))

    def set_matches(self, pairs, matches_per_pair):
        """dsm_set_matches: installs given FeatureMatches for the pair list (the verify-only / resume path of
        SiftFeatureMatcher::Match, matching.cc:806-812) instead of running the matcher."""
        pairs = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        off = np.zeros(len(pairs) + 1, dtype=np.uint64)
        for k, m in enumerate(matches_per_pair):
            off[k + 1] = off[k] + len(m)
        flat = np.ascontiguousarray(np.concatenate([np.asarray(m, dtype=np.uint32).reshape(-1, 2) for m in matches_per_pair] +
                                                   [np.zeros((1, 2), np.uint32)]), dtype=np.uint32)
        self._L.dsm_set_matches.argtypes = [ctypes.c_void_p, ctypes.c_uint32, u32p, ctypes.POINTER(ctypes.c_uint64), u32p]
        self._chk(self._L.dsm_set_matches(self._h, len(pairs), pairs.ctypes.data_as(u32p),
                                        off.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), flat.ctypes.data_as(u32p)))
        self.n_pairs = len(pairs)

    def match_counts(self):
        c = np.zeros(max(self.n_pairs, 1), dtype=np.uint32)
        self._chk(self._L.dsm_get_match_counts(self._h, c.ctypes.data))
        return c[:self.n_pairs]

    def matches(self):
        """Returns (offsets[n_pairs+1], matches[total,2])."""
        offs = np.zeros(self.n_pairs + 1, dtype=np.uint64)
        self._chk(self._L.dsm_get_matches(self._h, offs.ctypes.data, None, 0))
        total = int(offs[-1])
        m = np.zeros((max(total, 1), 2), dtype=np.uint32)
        self._chk(self._L.dsm_get_matches(self._h, None, m.ctypes.data, total))
        return offs, m[:total]

    def match_sift_features(self, desc1, desc2, options=None):
        """MatchSiftFeaturesCPU-shaped leaf, /root/reference/src/feature/sift.h:214-217."""
        options = options or default_match_options()
        d1 = np.ascontiguousarray(desc1, dtype=np.uint8).reshape(-1, 128)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8).reshape(-1, 128)
        out = np.zeros((max(d1.shape[0], 1), 2), dtype=np.uint32)
        n = ctypes.c_uint32(0)
        self._chk(self._L.dsm_match_sift_features(self._h, ctypes.byref(options), d1.ctypes.data_as(u8p), d1.shape[0],
                                                d2.ctypes.data_as(u8p), d2.shape[0], out.ctypes.data_as(u32p),
                                                ctypes.byref(n)))
        return out[:n.value].copy()

    def verify_pairs(self, options=None, seeds=None, user_seed=0, stage_filter=True):
        options = options or default_two_view_options()
        sp = None
        if seeds is not None:
            self._seeds = np.ascontiguousarray(seeds, dtype=np.uint32)
            assert len(self._seeds) == self.n_pairs
            sp = self._seeds.ctypes.data_as(u32p)
        self._chk(self._L.dsm_verify_pairs(self._h, ctypes.byref(options), sp, user_seed, int(bool(stage_filter))))

    def two_view_geometries(self):
        arr = (TwoViewGeometry * max(self.n_pairs, 1))()
        self._chk(self._L.dsm_get_two_view_geometries(self._h, ctypes.addressof(arr)))
        return list(arr)[:self.n_pairs]

    def inlier_matches(self):
        offs = np.zeros(self.n_pairs + 1, dtype=np.uint64)
        self._chk(self._L.dsm_get_inlier_matches(self._h, offs.ctypes.data, None, 0))
        total = int(offs[-1])
        m = np.zeros((max(total, 1), 2), dtype=np.uint32)
        self._chk(self._L.dsm_get_inlier_matches(self._h, None, m.ctypes.data, total))
        return offs, m[:total]

    def verify_kernel_time(self):
        ms = ctypes.c_double(0)
        self._chk(self._L.dsm_get_verify_kernel_time(self._h, ctypes.byref(ms)))
        return ms.value

    def estimate_two_view_geometry(self, cam1, pts1, cam2, pts2, matches, options=None, seed=0):
        """TwoViewGeometry::Estimate-shaped leaf, /root/reference/src/estimators/two_view_geometry.h:180-184."""
        options = options or default_two_view_options()
        p1 = np.ascontiguousarray(pts1, dtype=np.float64).reshape(-1, 2)
        p2 = np.ascontiguousarray(pts2, dtype=np.float64).reshape(-1, 2)
        m = np.ascontiguousarray(matches, dtype=np.uint32).reshape(-1, 2)
        out = TwoViewGeometry()
        inl = np.zeros((max(len(m), 1), 2), dtype=np.uint32)
        dp = ctypes.POINTER(ctypes.c_double)
        self._chk(self._L.dsm_estimate_two_view_geometry(self._h, ctypes.byref(cam1), p1.ctypes.data_as(dp), len(p1),
                                                       ctypes.byref(cam2), p2.ctypes.data_as(dp), len(p2),
                                                       m.ctypes.data_as(u32p), len(m), ctypes.byref(options), seed,
                                                       ctypes.byref(out), inl.ctypes.data_as(u32p)))
        return out, inl[:out.num_inliers].copy()

    def debug_sample_sequence(self, seed, k, total, n_draws):
        out = np.zeros((n_draws, k), dtype=np.uint32)
        self._chk(self._L.dsm_debug_sample_sequence(self._h, seed, k, total, n_draws, out.ctypes.data_as(u32p)))
        return out

    def debug_image_to_world(self, cam, xy):
        xy = np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2)
        out = np.zeros_like(xy)
        dp = ctypes.POINTER(ctypes.c_double)
        self._chk(self._L.dsm_debug_image_to_world(self._h, ctypes.byref(cam), len(xy), xy.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return out

    def match_kernel_time(self):
        ms = ctypes.c_double(0)
        n = ctypes.c_uint32(0)
        self._chk(self._L.dsm_get_match_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def guided_match_pairs(self, match_options=None, options=None, stage_filter=False):
        """dsm_guided_match_pairs: replaces the inlier matches of the verified pairs by guided matches."""
        mo = match_options if match_options is not None else default_match_options()
        to = options if options is not None else default_two_view_options()
        self._chk(self._L.dsm_guided_match_pairs(self._h, ctypes.byref(mo), ctypes.byref(to), 1 if stage_filter else 0))

    # ---- vocabulary-tree retrieval (candidate pairs)
    def retrieval_set_vocabulary(self, words, projection, thresholds):
        self._voc = (np.ascontiguousarray(words, np.uint8).reshape(-1, 128), np.ascontiguousarray(projection, np.float32).reshape(64, 128),
                     np.ascontiguousarray(thresholds, np.float32).reshape(-1, 64))
        assert self._voc[2].shape[0] == self._voc[0].shape[0]
        v = Vocabulary(num_words=self._voc[0].shape[0], reserved=0, words=self._voc[0].ctypes.data, projection=self._voc[1].ctypes.data,
                       thresholds=self._voc[2].ctypes.data)
        self._chk(self._L.dsm_retrieval_set_vocabulary(self._h, ctypes.byref(v)))

    def debug_solver_fallbacks(self):
        """dsm_debug_solver_fallbacks: waves of the E / F / H minimal solver that ran the exact pivot norms, then all its waves
        (check build, DSM_VERIFY_DEBUG)."""
        L = self._L
        out = np.zeros(6, np.uint32)
        L.dsm_debug_solver_fallbacks.restype = ctypes.c_int
        L.dsm_debug_solver_fallbacks.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(L.dsm_debug_solver_fallbacks(self._h, out.ctypes.data))
        return out

    def debug_verify_counters(self):
        """dsm_debug_verify_counters: 16 statistics counters of the last verify call (DSM_VERIFY_DEBUG / DSM_SCORE_PREFILTER=check)."""
        out = np.zeros(16, np.uint32)
        L = self._L
        L.dsm_debug_verify_counters.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(L.dsm_debug_verify_counters(self._h, out.ctypes.data))
        return out

    def retrieval_set_word_ids(self, index_ids, query_ids):
        """dsm_retrieval_set_word_ids: the caller's word ids (the reference's FLANN answer) instead of the device's exact
        search; index_ids [features], query_ids [features, k].  (None, None): exact search again."""
        L = self._L
        L.dsm_retrieval_set_word_ids.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
        if index_ids is None:
            self._chk(L.dsm_retrieval_set_word_ids(self._h, None, 0, None))
            return
        a = np.ascontiguousarray(index_ids, np.int32).reshape(-1)
        b = np.ascontiguousarray(query_ids, np.int32).reshape(len(a), -1)
        self._chk(L.dsm_retrieval_set_word_ids(self._h, a.ctypes.data, b.shape[1], b.ctypes.data))

    def retrieval_index(self):
        self._chk(self._L.dsm_retrieval_index(self._h))

    def retrieval_query(self, n_images, num_neighbors=5, max_num_images=100):
        """Returns a list (per query image, in dsm_set_images order) of (image_idx [c], scores [c]) in retrieval order."""
        cnt = np.zeros(n_images, np.uint32)
        idx = np.zeros((n_images, max_num_images), np.uint32)
        sc = np.zeros((n_images, max_num_images), np.float32)
        self._chk(self._L.dsm_retrieval_query(self._h, num_neighbors, max_num_images, cnt.ctypes.data, idx.ctypes.data, sc.ctypes.data))
        return [(idx[q, :cnt[q]].copy(), sc[q, :cnt[q]].copy()) for q in range(n_images)]

    def retrieval_matches(self, query_result, num_neighbors=5, max_num_images=100):
        """dsm_retrieval_matches + dsm_get_retrieval_matches for the retrieved lists of retrieval_query: (offsets [n+1] uint64,
        tuples [total, 5] uint32 = query feature, image, database feature, word << 8 | Hamming distance, entry position)."""
        n = len(query_result)
        cnt = np.array([len(r[0]) for r in query_result], np.uint32)
        idx = np.zeros((n, max_num_images), np.uint32)
        for q, r in enumerate(query_result):
            idx[q, :len(r[0])] = r[0]
        offs = np.zeros(n + 1, np.uint64)
        L = self._L
        L.dsm_retrieval_matches.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        L.dsm_get_retrieval_matches.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        self._chk(L.dsm_retrieval_matches(self._h, num_neighbors, max_num_images, cnt.ctypes.data, idx.ctypes.data, offs.ctypes.data))
        total = int(offs[-1])
        tup = np.zeros((max(total, 1), 5), np.uint32)
        self._chk(L.dsm_get_retrieval_matches(self._h, tup.ctypes.data, total))
        return offs, tup[:total]

    def retrieval_idf(self, num_words):
        out = np.zeros(num_words, np.float32)
        L = self._L
        L.dsm_get_retrieval_idf.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
        self._chk(L.dsm_get_retrieval_idf(self._h, out.ctypes.data, num_words))
        return out

    def retrieval_debug_word_ids(self, image, n_feats, k):
        out = np.zeros((max(n_feats, 1), k), np.int32)
        self._chk(self._L.dsm_retrieval_debug_word_ids(self._h, image, k, out.ctypes.data))
        return out[:n_feats]

    def retrieval_time(self):
        a, b = ctypes.c_double(0), ctypes.c_double(0)
        self._chk(self._L.dsm_get_retrieval_time(self._h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    # ---- training the vocabulary tree (VisualIndex::Build)
    def retrieval_quantize(self, descriptors, options=None, rand=None, with_centers=False):
        """dsm_retrieval_quantize: VisualIndex::Quantize of [n, 128] uint8 descriptors.  rand: a callable returning the next
        rand() value (None: the process's rand()).  Returns words [count, 128] uint8 (and the float centres)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 128)
        o = options if options is not None else default_vocabulary_build_options()
        cap = max(int(o.num_visual_words), 1)
        words = np.zeros((cap, 128), np.uint8)
        centers = np.zeros((cap, 128), np.float32) if with_centers else None
        count = ctypes.c_uint32(0)
        fn = RAND_FN(lambda user: int(rand())) if rand is not None else None
        self._chk(self._L.dsm_retrieval_quantize(self._h, ctypes.byref(o), d.ctypes.data, d.shape[0], fn, None, ctypes.byref(count),
                                                 words.ctypes.data, centers.ctypes.data if with_centers else None))
        return (words[:count.value], centers[:count.value]) if with_centers else words[:count.value]

    def vocabulary_tree(self):
        """dsm_get_vocabulary_tree: (parent, first_child, size, variance bits, radius bits, pivot bits [nodes, 128], indices) of
        the last retrieval_quantize, nodes in depth-first order."""
        n_nodes = ctypes.c_uint32(0)
        self._chk(self._L.dsm_get_vocabulary_tree(self._h, ctypes.byref(n_nodes), None, None, 0, None, 0))
        k = n_nodes.value
        nodes = (VocabularyTreeNode * k)()
        pivots = np.zeros((k, 128), np.float32)
        size_root = ctypes.c_uint32(0)
        self._chk(self._L.dsm_get_vocabulary_tree(self._h, ctypes.byref(size_root), ctypes.addressof(nodes), pivots.ctypes.data, k, None, 0))
        a = np.frombuffer(nodes, np.uint32).reshape(k, 5)
        indices = np.zeros(int(a[0, 2]), np.int32)
        self._chk(self._L.dsm_get_vocabulary_tree(self._h, None, None, None, 0, indices.ctypes.data, len(indices)))
        return (a[:, 0].astype(np.int32), a[:, 1].astype(np.int32), a[:, 2].astype(np.int32), a[:, 3].copy(), a[:, 4].copy(),
                pivots.view(np.uint32), indices)

    def retrieval_train_embedding(self, descriptors, words, projection, word_ids=None):
        """dsm_retrieval_train_embedding: (thresholds [num_words, 64] float32, has_embedding [num_words] uint8)."""
        d = np.ascontiguousarray(descriptors, np.uint8).reshape(-1, 128)
        w = np.ascontiguousarray(words, np.uint8).reshape(-1, 128)
        p = np.ascontiguousarray(projection, np.float32).reshape(64, 128)
        ids = None if word_ids is None else np.ascontiguousarray(word_ids, np.int32)
        assert ids is None or ids.shape == (d.shape[0],)
        thresholds = np.zeros((w.shape[0], 64), np.float32)
        has = np.zeros(w.shape[0], np.uint8)
        self._chk(self._L.dsm_retrieval_train_embedding(self._h, d.ctypes.data, d.shape[0], w.ctypes.data, w.shape[0], p.ctypes.data,
                                                        None if ids is None else ids.ctypes.data, thresholds.ctypes.data, has.ctypes.data))
        return thresholds, has

    def build_vocabulary(self, descriptors, projection, options=None, word_ids=None, rand=None):
        """VisualIndex::Build's numerical part: Quantize, then ComputeHammingEmbedding over the same descriptors.  Returns
        (words, projection, thresholds), what retrieval_set_vocabulary takes.  word_ids: the caller's word of every descriptor
        among the returned words (a callable is given the words first); None: the exact nearest word."""
        words = self.retrieval_quantize(descriptors, options, rand)
        ids = word_ids(words) if callable(word_ids) else word_ids
        thresholds, _ = self.retrieval_train_embedding(descriptors, words, projection, ids)
        return words, np.ascontiguousarray(projection, np.float32).reshape(64, 128), thresholds

    def vocabulary_build_time(self):
        """dsm_get_vocabulary_build_time: {stage: ms} of the last retrieval_quantize / retrieval_train_embedding."""
        ms = (ctypes.c_double * len(VOCABULARY_BUILD_STAGES))()
        self._chk(self._L.dsm_get_vocabulary_build_time(self._h, ctypes.addressof(ms)))
        return dict(zip(VOCABULARY_BUILD_STAGES, list(ms)))

    def view_graph_filter_cycles(self, pairs, qvecs, max_loop_error_degrees=5.0):
        """ViewGraph::FilterViewGraphCyclesByRotation over (pairs, qvecs): returns (keep [n] bool, number of triplets)."""
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        q = np.ascontiguousarray(qvecs, np.float64).reshape(-1, 4)
        assert len(p) == len(q)
        keep = np.zeros(max(len(p), 1), np.uint8)
        nt = ctypes.c_uint64(0)
        self._chk(self._L.dsm_view_graph_filter_cycles(self._h, len(p), p.ctypes.data, q.ctypes.data, max_loop_error_degrees,
                                                     keep.ctypes.data, ctypes.addressof(nt)))
        return keep[:len(p)].astype(bool), nt.value

    def rotation_averaging(self, pairs, qvecs, use=None, options=None):
        """dsm_view_graph_rotation_averaging (GlobalRotationAveraging: largest component, RobustRotationEstimator, orientation
        filter, largest component).  Returns a dict: image_ids [n], orientations [n, 3] (angle-axis), in_final_cc [n] bool,
        edge_state [n_pairs] uint8 (0 unused, 1 outside the component, 2 filtered, 3 kept), relative_rotations [n_pairs, 3],
        report (RotationAveragingReport)."""
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        q = np.ascontiguousarray(qvecs, np.float64).reshape(-1, 4)
        assert len(p) == len(q)
        n = len(p)
        u = None if use is None else np.ascontiguousarray(use, np.uint8).reshape(-1)
        assert u is None or len(u) == n
        cap = max(2 * n, 1)
        ids = np.zeros(cap, np.uint32)
        orient = np.zeros((cap, 3), np.float64)
        fin = np.zeros(cap, np.uint8)
        nimg = ctypes.c_uint32(0)
        state = np.zeros(max(n, 1), np.uint8)
        rel = np.zeros((max(n, 1), 3), np.float64)
        rep = RotationAveragingReport()
        opt = ctypes.byref(options) if options is not None else None
        self._chk(self._L.dsm_view_graph_rotation_averaging(self._h, n, p.ctypes.data, q.ctypes.data, None if u is None else u.ctypes.data,
                                                            opt, ids.ctypes.data, orient.ctypes.data, fin.ctypes.data,
                                                            ctypes.addressof(nimg), state.ctypes.data, rel.ctypes.data, ctypes.addressof(rep)))
        k = nimg.value
        return {"image_ids": ids[:k].copy(), "orientations": orient[:k].copy(), "in_final_cc": fin[:k].astype(bool),
                "edge_state": state[:n].copy(), "relative_rotations": rel[:n].copy(), "report": rep}

    def rotation_averaging_nonlinear(self, pairs, qvecs, use=None, initial=None, options=None):
        """dsm_view_graph_rotation_averaging_nonlinear (GlobalRotationAveraging with the NONLINEAR estimator: largest component,
        NonlinearRotationEstimator, orientation filter, largest component).  initial: None (every orientation starts at zero) or a
        dict with image_ids (ascending) and orientations -- what rotation_averaging returns fits.  Returns the dict of
        rotation_averaging with a NonlinearRotationReport, plus trace [iterations + 1, NLR_TRACE_COLUMNS].  The orientations
        carry a free common rotation: compare them relative to one image."""
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        q = np.ascontiguousarray(qvecs, np.float64).reshape(-1, 4)
        assert len(p) == len(q)
        n = len(p)
        u = None if use is None else np.ascontiguousarray(use, np.uint8).reshape(-1)
        assert u is None or len(u) == n
        n_init, init_ids, init_aa = 0, None, None
        if initial is not None:
            init_ids = np.ascontiguousarray(initial["image_ids"], np.uint32).reshape(-1)
            init_aa = np.ascontiguousarray(initial["orientations"], np.float64).reshape(-1, 3)
            assert len(init_ids) == len(init_aa)
            n_init = len(init_ids)
        opts = options if options is not None else default_nonlinear_rotation_options()
        cap = max(2 * n, 1)
        ids = np.zeros(cap, np.uint32)
        orient = np.zeros((cap, 3), np.float64)
        fin = np.zeros(cap, np.uint8)
        nimg = ctypes.c_uint32(0)
        state = np.zeros(max(n, 1), np.uint8)
        rel = np.zeros((max(n, 1), 3), np.float64)
        rep = NonlinearRotationReport()
        trace = np.full((max(int(opts.max_num_iterations), 0) + 1, NLR_TRACE_COLUMNS), np.nan)
        self._chk(self._L.dsm_view_graph_rotation_averaging_nonlinear(
            self._h, n, p.ctypes.data, q.ctypes.data, None if u is None else u.ctypes.data, n_init,
            init_ids.ctypes.data if n_init else None, init_aa.ctypes.data if n_init else None, ctypes.byref(opts), ids.ctypes.data,
            orient.ctypes.data, fin.ctypes.data, ctypes.addressof(nimg), state.ctypes.data, rel.ctypes.data, ctypes.addressof(rep),
            trace.ctypes.data))
        k = nimg.value
        return {"image_ids": ids[:k].copy(), "orientations": orient[:k].copy(), "in_final_cc": fin[:k].astype(bool),
                "edge_state": state[:n].copy(), "relative_rotations": rel[:n].copy(), "report": rep,
                "trace": trace[:rep.num_iterations + 1].copy() if k else trace[:0].copy()}

    def debug_pairwise_rotation_error(self, rotation1, rotation2, relative_rotation, loss_width=0.1):
        """dsm_debug_pairwise_rotation_error: the per-edge device function of rotation_averaging_nonlinear on n triples of
        angle-axis rotations.  Returns (residuals [n, 3], jacobians [n, 2, 3, 3] with respect to rotation1 and rotation2, both after
        the loss corrector, rho [n, 3] = rho, rho', rho'' at the uncorrected |r|^2)."""
        a = [np.ascontiguousarray(v, np.float64).reshape(-1, 3) for v in (rotation1, rotation2, relative_rotation)]
        n = len(a[0])
        assert len(a[1]) == n and len(a[2]) == n
        res, jac, rho = np.zeros((max(n, 1), 3)), np.zeros((max(n, 1), 2, 3, 3)), np.zeros((max(n, 1), 3))
        self._chk(self._L.dsm_debug_pairwise_rotation_error(self._h, n, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data,
                                                          float(loss_width), res.ctypes.data, jac.ctypes.data, rho.ctypes.data))
        return res[:n], jac[:n], rho[:n]

    def cluster_view_graph(self, pairs, weights, use=None, labels_in=None, options=None):
        """dsm_view_graph_cluster (ClusteringScenes: SPECTRAL on the device, or Cut + Expand over labels_in).  Returns a dict:
        image_ids [n], labels [n] (intra cluster), edge_cluster [n_pairs] int32 (-1 unused / repeat, -2 lost, else the inter
        cluster), clusters (list of sorted image-id arrays, one per inter cluster), offsets, eigenvalues (the final Ritz values)
        and eigenvectors ([n, k]: the vectors the k-means ran on) when the eigen-solver ran, else None; report."""
        p = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
        w = np.ascontiguousarray(weights, np.int32).reshape(-1)
        assert len(p) == len(w)
        n = len(p)
        u = None if use is None else np.ascontiguousarray(use, np.uint8).reshape(-1)
        assert u is None or len(u) == n
        li = None if labels_in is None else np.ascontiguousarray(labels_in, np.uint32).reshape(-1)
        cap = max(2 * n, 1)
        ids = np.zeros(cap, np.uint32)
        lab = np.zeros(cap, np.uint32)
        nimg = ctypes.c_uint32(0)
        ec = np.zeros(max(n, 1), np.int32)
        offs = np.zeros(2 * n + 1, np.uint32)
        imgs = np.zeros(max(3 * n, 1), np.uint32)
        ncl = ctypes.c_uint32(0)
        rep = ClusteringReport()
        opt = ctypes.byref(options) if options is not None else None
        self._chk(self._L.dsm_view_graph_cluster(self._h, n, p.ctypes.data, w.ctypes.data, None if u is None else u.ctypes.data,
                                                 None if li is None else li.ctypes.data, opt, ids.ctypes.data, lab.ctypes.data,
                                                 ctypes.addressof(nimg), ec.ctypes.data, offs.ctypes.data, imgs.ctypes.data,
                                                 ctypes.addressof(ncl), ctypes.addressof(rep)))
        k = nimg.value
        clusters = [imgs[offs[c]:offs[c + 1]].copy() for c in range(ncl.value)]
        ev = vec = None
        if labels_in is None and rep.eigen_iterations > 0:
            nv, nr, nc = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint32(0)
            ev = np.zeros(max(rep.ncv, 1), np.float64)
            vec = np.zeros(k * max(rep.ncv, 1), np.float64)  # k <= ncv columns
            self._chk(self._L.dsm_get_clustering_spectrum(self._h, ev.ctypes.data, len(ev), vec.ctypes.data, vec.size,
                                                          ctypes.addressof(nv), ctypes.addressof(nr), ctypes.addressof(nc)))
            ev = ev[:nv.value]
            vec = vec.reshape(-1)[:nr.value * nc.value].reshape(nr.value, nc.value)
        return {"image_ids": ids[:k].copy(), "labels": lab[:k].copy(), "edge_cluster": ec[:n].copy(), "clusters": clusters,
                "offsets": offs[:ncl.value + 1].copy(), "eigenvalues": ev, "eigenvectors": vec, "report": rep}

    def align_clusters(self, clusters, options=None, seeds=None):
        """dsm_align_clusters (SfMAligner::Align up to the transforms).  clusters: a list of K dicts with
        image_ids [r] (registered images), point_ids [p] (uint64), xyz [p, 3] (float64) and obs [m, 3] (image_id, point2D_idx,
        point index inside the cluster).  seeds: None or a [K, K] uint32 array, seeds[a, b] for the direction a -> b.
        A non-finite xyz coordinate or threshold raises DsmError ("non-finite"), like every other invalid input.
        Returns a dict: pairs (ALIGN_PAIR_DTYPE records in ascending (i, j)), anchor, in_component [K] bool, mst_parent [K],
        sim3_to_anchor as s [K], R [K, 3, 3], t [K, 3], separators (sorted image ids), report."""
        K = len(clusters)
        cat = lambda key, dt, shape: [np.ascontiguousarray(c[key], dt).reshape(shape) for c in clusters]
        imgs, pids = cat("image_ids", np.uint32, -1), cat("point_ids", np.uint64, -1)
        xyz, obs = cat("xyz", np.float64, (-1, 3)), cat("obs", np.uint32, (-1, 3))
        offs = lambda arrs: np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.uint32)
        ioff, poff, ooff = offs(imgs), offs(pids), offs(obs)
        cimg = np.ascontiguousarray(np.concatenate(imgs) if K else np.zeros(0, np.uint32), np.uint32)
        cpid = np.ascontiguousarray(np.concatenate(pids) if K else np.zeros(0, np.uint64), np.uint64)
        cxyz = np.ascontiguousarray(np.concatenate(xyz) if K else np.zeros((0, 3)), np.float64)
        cobs = np.ascontiguousarray(np.concatenate(obs) if K else np.zeros((0, 3), np.uint32), np.uint32)
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint32).reshape(K * K)
        cap = max(K * (K - 1) // 2, 1)
        pairs = np.zeros(cap, ALIGN_PAIR_DTYPE)
        npairs, anchor, nsep = ctypes.c_uint32(0), ctypes.c_int32(0), ctypes.c_uint32(0)
        inc = np.zeros(max(K, 1), np.uint8)
        par = np.zeros(max(K, 1), np.int32)
        sim = np.zeros((max(K, 1), 13), np.float64)
        seps = np.zeros(max(len(cimg), 1), np.uint32)
        rep = AlignReport()
        opt = ctypes.byref(options) if options is not None else None
        self._chk(self._L.dsm_align_clusters(self._h, K, ioff.ctypes.data, cimg.ctypes.data, poff.ctypes.data, cpid.ctypes.data,
                                             cxyz.ctypes.data, ooff.ctypes.data, cobs.ctypes.data, opt,
                                             None if sd is None else sd.ctypes.data, pairs.ctypes.data, cap, ctypes.addressof(npairs),
                                             ctypes.addressof(anchor), inc.ctypes.data, par.ctypes.data, sim.ctypes.data,
                                             seps.ctypes.data, ctypes.addressof(nsep), ctypes.addressof(rep)))
        return {"pairs": pairs[:npairs.value].copy(), "anchor": anchor.value, "in_component": inc[:K].astype(bool),
                "mst_parent": par[:K].copy(), "s": sim[:K, 0].copy(), "R": sim[:K, 1:10].reshape(K, 3, 3).copy(),
                "t": sim[:K, 10:13].copy(), "separators": seps[:nsep.value].copy(), "report": rep}

    def bundle_adjust(self, scene, options=None, trace=True):
        """dsm_bundle_adjust.  scene: a dict with camera_model_ids [C], camera_params (each camera's parameters
        back to back), image_camera [N], qvec [N, 4], tvec [N, 3], image_constant_pose [N] (optional), image_constant_tvec [N]
        (optional, bit mask), point_ids [P] (uint64), xyz [P, 3], point_constant [P] (optional), track_offsets [P + 1],
        obs_image [n], obs_xy [n, 2].  The inputs are not modified.  Returns a dict: camera_params, qvec, tvec, xyz (updated),
        report, trace ([iterations + 1, 6]: cost, radius, rho, CG iterations, accepted, gradient max-norm)."""
        arr = lambda key, dt, shape=-1: np.array(scene[key], dtype=dt, copy=True).reshape(shape)
        opt_u8 = lambda key, n: None if scene.get(key) is None else np.ascontiguousarray(scene[key], np.uint8).reshape(n)
        models = arr("camera_model_ids", np.int32)
        params = arr("camera_params", np.float64)
        icam = arr("image_camera", np.uint32)
        N = len(icam)
        qvec, tvec = arr("qvec", np.float64, (N, 4)), arr("tvec", np.float64, (N, 3))
        pids = arr("point_ids", np.uint64)
        P = len(pids)
        xyz = arr("xyz", np.float64, (P, 3))
        toff = arr("track_offsets", np.uint32)
        oimg, oxy = arr("obs_image", np.uint32), arr("obs_xy", np.float64, (-1, 2))
        cpose, cmask, pconst = opt_u8("image_constant_pose", N), opt_u8("image_constant_tvec", N), opt_u8("point_constant", P)
        o = options if options is not None else default_bundle_adjustment_options()
        tr = np.full((max(int(o.max_num_iterations), 0) + 1, BA_TRACE_COLUMNS), np.nan) if trace else None
        rep = BundleAdjustmentReport()
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self._L.dsm_bundle_adjust(self._h, len(models), ptr(models), ptr(params), N, ptr(icam), ptr(qvec), ptr(tvec),
                                            ptr(cpose), ptr(cmask), P, ptr(pids), ptr(xyz), ptr(pconst), ptr(toff), ptr(oimg),
                                            ptr(oxy), ctypes.byref(o), ctypes.addressof(rep), ptr(tr)))
        out = {"camera_params": params, "qvec": qvec, "tvec": tvec, "xyz": xyz, "report": rep}
        if trace:
            out["trace"] = tr[:rep.num_iterations + 1].copy()
        return out

    def filter_points3D(self, scene, passes=None, point_selected=None, image_selected=None, **options):
        """dsm_filter_points3D.  scene: the dict of bundle_adjust (camera_model_ids, camera_params, image_camera,
        qvec, tvec, xyz, track_offsets, obs_image, obs_xy), optionally with camera_width / camera_height [C] (they feed the bogus
        test of the image verdict; without them the principal point is taken as the image centre: width = 2 cx, height = 2 cy)
        and image_registered [N].  passes: FILTER_* bits (None = the default 2 | 4); options: fields of PointFilterOptions.
        point_selected [P] / image_selected [N]: the selection (both None = every point; image_selected alone selects the points
        seen in those images).  Returns a dict: point_keep [P] (bool), obs_keep [n] (bool), point_error [P] (-1 = none),
        kept_track_offsets [P + 1], kept_obs [kept], image_filtered [N] (bool), camera_sizes_given (False: the sizes behind
        image_filtered and min_bogus_margin were made up as above -- pass camera_width / camera_height where that verdict is to
        be trusted), report."""
        a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
        models, params = a("camera_model_ids", np.int32), a("camera_params", np.float64)
        C = len(models)
        cams = (Camera * max(C, 1))()
        at = 0
        sizes_given = scene.get("camera_width") is not None and scene.get("camera_height") is not None
        for c in range(C):
            m = int(models[c])
            k = CAMERA_MODEL_NUM_PARAMS[m] if 0 <= m < len(CAMERA_MODEL_NUM_PARAMS) else 0
            pr = params[at:at + k]
            at += k
            pp = 2 if m in (1, 4, 5, 6, 7, 10) else 1
            if sizes_given:
                w, h = int(scene["camera_width"][c]), int(scene["camera_height"][c])
            else:
                w, h = (max(int(np.ceil(2 * pr[pp])), 0), max(int(np.ceil(2 * pr[pp + 1])), 0)) if k and np.isfinite(pr[pp:pp + 2]).all() else (0, 0)
            cams[c] = camera(m, pr, w, h)
        icam = a("image_camera", np.uint32)
        N = len(icam)
        qvec, tvec = a("qvec", np.float64, (N, 4)), a("tvec", np.float64, (N, 3))
        xyz = a("xyz", np.float64, (-1, 3))
        P = len(xyz)
        toff = a("track_offsets", np.uint32)
        oimg, oxy = a("obs_image", np.uint32), a("obs_xy", np.float64, (-1, 2))
        n = len(oimg)
        u8 = lambda v, k: None if v is None else np.ascontiguousarray(np.asarray(v) != 0, np.uint8).reshape(k)
        reg, psel, isel = u8(scene.get("image_registered"), N), u8(point_selected, P), u8(image_selected, N)
        if isel is not None and psel is None:
            psel = np.zeros(P, np.uint8)
        o = default_point_filter_options(**options)
        if passes is not None:
            o.passes = int(passes)
        pkeep, okeep, perr = np.zeros(max(P, 1), np.uint8), np.zeros(max(n, 1), np.uint8), np.full(max(P, 1), -1.0)
        koff, kobs, ifilt = np.zeros(P + 1, np.uint32), np.zeros(max(n, 1), np.uint32), np.zeros(max(N, 1), np.uint8)
        rep = PointFilterReport()
        ptr = lambda x: None if x is None else x.ctypes.data
        self._chk(self._L.dsm_filter_points3D(self._h, C, ctypes.addressof(cams), N, ptr(icam), ptr(qvec), ptr(tvec), ptr(reg), P, ptr(xyz),
                                              ptr(toff), ptr(oimg), ptr(oxy), ptr(psel), ptr(isel), ctypes.byref(o), ptr(pkeep), ptr(okeep),
                                              ptr(perr), ptr(koff), ptr(kobs), ptr(ifilt), ctypes.addressof(rep)))
        return {"point_keep": pkeep[:P].astype(bool), "obs_keep": okeep[:n].astype(bool), "point_error": perr[:P].copy(),
                "kept_track_offsets": koff, "kept_obs": kobs[:int(koff[P])].copy(), "image_filtered": ifilt[:N].astype(bool),
                "camera_sizes_given": sizes_given, "report": rep}

    def extract_sift(self, image_u8, options=None, descriptors=True, capacity=None, width=None):
        """dsm_extract_sift: image_u8 [height, row_stride] grey bytes, of which the first `width` of a row are the
        image (None: all of them).  Returns (keypoints float32 [n, 4] = (x, y, sigma, angle), descriptors uint8 [n, 128] in UBC
        order, or None with descriptors=False).  capacity None: room for 32768 features, and a second call with the count the
        first one reports where that is too little; a given capacity below the count raises DsmError with the count in
        .num_features."""
        im = np.ascontiguousarray(image_u8, np.uint8)
        height, row_stride = im.shape
        width = row_stride if width is None else int(width)
        o = options if options is not None else default_sift_options()
        n = ctypes.c_uint32(0)

        def call(cap):
            kp = np.zeros((max(cap, 1), 4), np.float32)
            ds = np.zeros((max(cap, 1), 128), np.uint8) if descriptors else None
            rc = self._L.dsm_extract_sift(self._h, ctypes.byref(o), im.ctypes.data, width, height, row_stride, cap, kp.ctypes.data,
                                          None if ds is None else ds.ctypes.data, ctypes.byref(n))
            return rc, kp, ds

        rc, kp, ds = call(32768 if capacity is None else int(capacity))
        if rc == 4 and capacity is None and n.value > 0:
            rc, kp, ds = call(int(n.value))
        if rc != 0:
            err = DsmError("dsm_extract_sift failed (%d): %s" % (rc, self._L.dsm_last_error(self._handle).decode()))
            err.num_features = int(n.value)
            err.status = rc
            raise err
        return kp[:n.value].copy(), (None if ds is None else ds[:n.value].copy())

    SIFT_STAGES = ("base", "smoothing", "detect", "refine", "gradient", "orientations", "descriptors")

    def sift_time(self):
        """dsm_get_sift_time: {stage: ms} of the last extract_sift (HIP events, summed over the octaves)."""
        ms = (ctypes.c_double * len(self.SIFT_STAGES))()
        self._L.dsm_get_sift_time.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        self._chk(self._L.dsm_get_sift_time(self._h, ctypes.addressof(ms)))
        return dict(zip(self.SIFT_STAGES, list(ms)))

    def extract_covariant_sift(self, image_u8, options=None, descriptors=True, capacity=None, width=None):
        """dsm_extract_covariant_sift: image_u8 [height, row_stride] grey bytes, of which the first `width` of a
        row are the image (None: all of them).  Returns (keypoints float32 [n, 6] = (x, y, a11, a12, a21, a22), descriptors uint8
        [n, 128] in UBC order, or None with descriptors=False).  capacity None: room for 32768 features, and a second call with
        the count the first one reports where that is too little; a given capacity below the count raises DsmError with the
        count in .num_features."""
        im = np.ascontiguousarray(image_u8, np.uint8)
        height, row_stride = im.shape
        width = row_stride if width is None else int(width)
        o = options if options is not None else default_covariant_sift_options()
        n = ctypes.c_uint32(0)

        def call(cap):
            kp = np.zeros((max(cap, 1), 6), np.float32)
            ds = np.zeros((max(cap, 1), 128), np.uint8) if descriptors else None
            rc = self._L.dsm_extract_covariant_sift(self._h, ctypes.byref(o), im.ctypes.data, width, height, row_stride, cap, kp.ctypes.data,
                                                    None if ds is None else ds.ctypes.data, ctypes.byref(n))
            return rc, kp, ds

        rc, kp, ds = call(32768 if capacity is None else int(capacity))
        if rc == 4 and capacity is None and n.value > 0:
            rc, kp, ds = call(int(n.value))
        if rc != 0:
            err = DsmError("dsm_extract_covariant_sift failed (%d): %s" % (rc, self._L.dsm_last_error(self._handle).decode()))
            err.num_features = int(n.value)
            err.status = rc
            err.outputs = (kp, ds)  # as the library left them
            raise err
        return kp[:n.value].copy(), (None if ds is None else ds[:n.value].copy())

    def extract_covariant_sift_affine(self, image_u8, options=None, descriptors=True, capacity=None, width=None):
        """dsm_extract_covariant_sift_affine: extract_covariant_sift's arguments, results and capacity retry;
        options.estimate_affine_shape = 1 adapts every frame to its patch's second-moment matrix (vl_covdet_extract_affine_shape)
        in the place of the orientations."""
        im = np.ascontiguousarray(image_u8, np.uint8)
        height, row_stride = im.shape
        width = row_stride if width is None else int(width)
        o = options if options is not None else default_covariant_sift_options()
        n = ctypes.c_uint32(0)

        def call(cap):
            kp = np.zeros((max(cap, 1), 6), np.float32)
            ds = np.zeros((max(cap, 1), 128), np.uint8) if descriptors else None
            rc = self._L.dsm_extract_covariant_sift_affine(self._h, ctypes.byref(o), im.ctypes.data, width, height, row_stride, cap,
                                                           kp.ctypes.data, None if ds is None else ds.ctypes.data, ctypes.byref(n))
            return rc, kp, ds

        rc, kp, ds = call(32768 if capacity is None else int(capacity))
        if rc == 4 and capacity is None and n.value > 0:
            rc, kp, ds = call(int(n.value))
        if rc != 0:
            err = DsmError("dsm_extract_covariant_sift_affine failed (%d): %s" % (rc, self._L.dsm_last_error(self._handle).decode()))
            err.num_features = int(n.value)
            err.status = rc
            err.outputs = (kp, ds)  # as the library left them
            raise err
        return kp[:n.value].copy(), (None if ds is None else ds[:n.value].copy())

    AFFINE_SHAPE_EXITS = ("diverged", "max_iterations", "zero_moment", "converged")

    def affine_shape_stats(self):
        """dsm_get_affine_shape_stats: the shape adaptation of the last extract_covariant_sift_affine as {"rounds": launches of
        the moment kernel, "exits": {why: features} in the order of AFFINE_SHAPE_EXITS, "active": [features in round r] * 14}."""
        rounds = ctypes.c_uint32(0)
        exits = (ctypes.c_uint32 * 4)()
        active = (ctypes.c_uint32 * 14)()
        self._chk(self._L.dsm_get_affine_shape_stats(self._h, ctypes.byref(rounds), ctypes.addressof(exits), ctypes.addressof(active)))
        return {"rounds": int(rounds.value), "exits": dict(zip(self.AFFINE_SHAPE_EXITS, list(exits))), "active": list(active)}

    def covariant_sift_raw(self, num_scales=None):
        """dsm_get_covariant_sift_raw: the last extract_covariant_sift's features in output order as {"octave_scale": int32 [n, 2],
        "scores": float32 [n, 3] = peak, edge, orientation, "raw": float32 [n, num_scales, 128] = VLFeat's descriptor of every
        pooling scale before the pooling, in VLFeat's bin order}.  num_scales None: no raw descriptors are fetched."""
        n = ctypes.c_uint32(0)
        rc = self._L.dsm_get_covariant_sift_raw(self._h, 0, None, None, None, ctypes.byref(n))
        if rc not in (0, 4):
            self._chk(rc)
        cap = max(int(n.value), 1)
        os_ = np.zeros((cap, 2), np.int32)
        sc = np.zeros((cap, 3), np.float32)
        raw = np.zeros((cap, int(num_scales), 128), np.float32) if num_scales else None
        self._chk(self._L.dsm_get_covariant_sift_raw(self._h, cap, os_.ctypes.data, sc.ctypes.data, None if raw is None else raw.ctypes.data,
                                                     ctypes.byref(n)))
        k = int(n.value)
        return {"octave_scale": os_[:k].copy(), "scores": sc[:k].copy(), "raw": None if raw is None else raw[:k].copy()}

    COVARIANT_SIFT_STAGES = ("scale_space", "detection", "orientations", "descriptors", "pooling")

    def covariant_sift_time(self):
        """dsm_get_covariant_sift_time: {stage: ms} of the last extract_covariant_sift (HIP events)."""
        ms = (ctypes.c_double * len(self.COVARIANT_SIFT_STAGES))()
        self._chk(self._L.dsm_get_covariant_sift_time(self._h, ctypes.addressof(ms)))
        return dict(zip(self.COVARIANT_SIFT_STAGES, list(ms)))

    def _fail(self, name, rc):
        err = DsmError("%s failed (%d): %s" % (name, rc, self._L.dsm_last_error(self._handle).decode()))
        err.rc = rc
        raise err

    def undistort_cameras(self, cameras, options=None, **kw):
        """dsm_undistort_cameras (UndistortCamera): a list of Camera -> the list of their PINHOLE cameras.
        options: an UndistortOptions, or its fields as keywords over the defaults."""
        assert options is None or not kw, "pass an UndistortOptions or keywords, not both"
        o = options if options is not None else default_undistort_options(**kw)
        n = len(cameras)
        arr, out = (Camera * max(n, 1))(*cameras), (Camera * max(n, 1))()
        rc = self._L.dsm_undistort_cameras(self._h, ctypes.byref(o), n, ctypes.addressof(arr), ctypes.addressof(out))
        if rc != 0:
            self._fail("dsm_undistort_cameras", rc)
        return [copy_camera(out[i]) for i in range(n)]

    def undistort_points2D(self, cameras, undistorted_cameras, camera_index, xy):
        """dsm_undistort_points2D (the loop of UndistortReconstruction): xy [n, 2] of the points of camera camera_index[i] ->
        the undistorted xy [n, 2] (a new array)."""
        assert len(cameras) == len(undistorted_cameras)
        nc = len(cameras)
        a, b = (Camera * max(nc, 1))(*cameras), (Camera * max(nc, 1))(*undistorted_cameras)
        idx = np.ascontiguousarray(camera_index, np.uint32).reshape(-1)
        out = np.array(xy, dtype=np.float64, order="C").reshape(-1, 2)
        assert len(idx) == len(out)
        rc = self._L.dsm_undistort_points2D(self._h, nc, ctypes.addressof(a), ctypes.addressof(b), len(out), idx.ctypes.data, out.ctypes.data)
        if rc != 0:
            self._fail("dsm_undistort_points2D", rc)
        return out

    def warp_images(self, source, target, images, H=None, return_map=False, out=None):
        """dsm_warp_images (src/base/warp.cc).  images: uint8 [n, height, width] (grey), [n, height, width, 3], or
        one grey image [height, width]; only the pixels of a row have to be contiguous, so a view with a longer row stride is
        passed as it is.  source / target: Camera; for WarpImageWithHomography (H alone) source is None or a size_only_camera
        (None: the images' size) and target None or the size_only_camera of the target image.  The size of the images must be
        the source camera's (DsmError otherwise, as the reference CHECKs).
        Returns a dict: images (the warp, shaped like the input; at the SOURCE resolution with cameras), scaled_target (Camera),
        needs_rescale (bool: Bitmap::Rescale to the target camera's width x height is still the caller's to do), and with
        return_map source_xy [height, width, 2]."""
        im = np.asarray(images)
        if im.dtype != np.uint8:
            raise DsmError("dsm_warp_images: images must be uint8")
        single = im.ndim == 2
        if single:
            im = im[None]
        if im.ndim not in (3, 4):
            raise DsmError("dsm_warp_images: images must be [n, height, width] or [n, height, width, channels]")
        channels = 1 if im.ndim == 3 else im.shape[3]
        n, height, width = im.shape[:3]
        if source is None:
            source = size_only_camera(width, height)
        if int(source.width) != width or int(source.height) != height:
            raise DsmError("dsm_warp_images failed (%d): the camera's size %d x %d differs from the images' %d x %d"
                           % (DSM_ERR_INVALID_ARGUMENT, source.width, source.height, width, height))
        pix = im.strides[2] if n * height * width else channels
        inner_ok = pix == channels and (im.ndim == 3 or channels == 1 or im.strides[3] == 1)
        if not inner_ok or (height > 1 and im.strides[1] < 0) or (n > 1 and im.strides[0] < 0):
            im = np.ascontiguousarray(im)
        src_row = im.strides[1] if height > 1 else width * channels
        src_img = im.strides[0] if n > 1 else src_row * height
        size_only = int(source.model_id) == CAMERA_SIZE_ONLY
        tw, th = (int(target.width), int(target.height)) if (size_only and target is not None) else (width, height)
        if out is None:
            out = np.zeros((n, th, tw) + ((channels,) if im.ndim == 4 else ()), np.uint8)
        assert out.dtype == np.uint8 and out.shape[0] == n and out.shape[1:3] == (th, tw)
        dst_row = out.strides[1] if th > 1 else tw * channels
        dst_img = out.strides[0] if n > 1 else dst_row * th
        scaled, owed = Camera(), ctypes.c_int32(0)
        Hm = None if H is None else np.ascontiguousarray(H, np.float64).reshape(9)
        smap = np.zeros((th, tw, 2)) if return_map else None
        rc = self._L.dsm_warp_images(self._h, ctypes.addressof(source), None if target is None else ctypes.addressof(target),
                                     None if Hm is None else Hm.ctypes.data, n, channels, im.ctypes.data, src_row, src_img,
                                     out.ctypes.data, dst_row, dst_img, ctypes.addressof(scaled), ctypes.addressof(owed),
                                     None if smap is None else smap.ctypes.data)
        if rc != 0:
            self._fail("dsm_warp_images", rc)
        res = {"images": out[0] if single else out, "scaled_target": scaled, "needs_rescale": bool(owed.value)}
        if return_map:
            res["source_xy"] = smap
        return res

    def undistort_images(self, images, camera, options=None, **kw):
        """UndistortImage (undistortion.cc:844-859) for a batch of images of one camera: undistort_cameras, then warp_images
        into the undistorted camera.  Returns (the warped stack at the SOURCE resolution, the undistorted Camera, whether a
        rescale of every image to (width, height) of that camera is still owed -- Bitmap::Rescale, the caller's)."""
        und = self.undistort_cameras([camera], options, **kw)[0]
        r = self.warp_images(camera, und, images)
        return r["images"], und, r["needs_rescale"]

    def undistortion_time(self):
        """dsm_get_undistortion_time: {stage: ms} of the last call of each kind (HIP events)."""
        ms = (ctypes.c_double * len(UNDISTORTION_STAGES))()
        self._chk(self._L.dsm_get_undistortion_time(self._h, ctypes.addressof(ms)))
        return dict(zip(UNDISTORTION_STAGES, list(ms)))

    def patch_match(self, images, problems, options=None, return_sel_prob=True, **kw):
        """dsm_patch_match (PatchMatchCuda::Run), one pass over a batch of problems.
        images: a list of dicts -- data [h][w] uint8, K [9], R [9], T [3] and, for geom_consistency, depth_map [h][w] and
        normal_map [3][h][w] float32.  problems: a list of (ref_image, src_images, depth_min, depth_max).
        options: a PatchMatchOptions, or its fields as keywords over the defaults.
        Returns a list of dicts per problem: depth [H][W], normal [3][H][W], sel_prob [S][H][W] (None unless asked for),
        mask [S][H][W] uint8 (None without filter)."""
        assert options is None or not kw, "pass a PatchMatchOptions or keywords, not both"
        o = options if options is not None else default_patch_match_options(**kw)
        keep = []
        arr = (MvsImage * max(len(images), 1))()
        for i, im in enumerate(images):
            data = np.ascontiguousarray(im["data"], dtype=np.uint8)
            assert data.ndim == 2
            keep.append(data)
            arr[i].data, arr[i].row_stride = data.ctypes.data, data.strides[0]
            arr[i].height, arr[i].width = data.shape
            for name, n in (("K", 9), ("R", 9), ("T", 3)):
                v = np.asarray(im[name], dtype=np.float32).reshape(-1)
                assert len(v) == n, name
                setattr(arr[i], name, (ctypes.c_float * n)(*v.tolist()))
            for name, shape in (("depth_map", data.shape), ("normal_map", (3,) + data.shape)):
                if im.get(name) is not None:
                    m = np.ascontiguousarray(im[name], dtype=np.float32)
                    assert m.shape == shape, name
                    keep.append(m)
                    setattr(arr[i], name, m.ctypes.data)
        n = len(problems)
        ref = np.array([p[0] for p in problems], dtype=np.uint32)
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(p[1]) for p in problems])
        src = np.array([s for p in problems for s in p[1]], dtype=np.uint32)
        dmin = np.array([p[2] for p in problems], dtype=np.float32)
        dmax = np.array([p[3] for p in problems], dtype=np.float32)
        out = []
        ptrs = [(ctypes.c_void_p * max(n, 1))() for _ in range(4)]
        for k, p in enumerate(problems):
            assert 0 <= p[0] < len(images), "reference image index out of range"
            h, w = np.asarray(images[p[0]]["data"]).shape
            S = len(p[1])
            r = {"depth": np.zeros((h, w), np.float32), "normal": np.zeros((3, h, w), np.float32),
                 "sel_prob": np.zeros((S, h, w), np.float32) if return_sel_prob else None,
                 "mask": np.zeros((S, h, w), np.uint8) if o.filter else None}
            out.append(r)
            ptrs[0][k], ptrs[1][k] = r["depth"].ctypes.data, r["normal"].ctypes.data
            ptrs[2][k] = r["sel_prob"].ctypes.data if return_sel_prob else None
            # (a zero-sized array has no address worth passing: any non-NULL pointer stands for the empty mask)
            ptrs[3][k] = (r["mask"].ctypes.data or r["depth"].ctypes.data) if o.filter else None
        rc = self._L.dsm_patch_match(self._h, ctypes.byref(o), len(images), ctypes.addressof(arr), n, ref.ctypes.data, offs.ctypes.data,
                                     src.ctypes.data if len(src) else None, dmin.ctypes.data, dmax.ctypes.data, ctypes.addressof(ptrs[0]),
                                     ctypes.addressof(ptrs[1]), ctypes.addressof(ptrs[2]), ctypes.addressof(ptrs[3]))
        if rc != 0:
            self._fail("dsm_patch_match", rc)
        return out

    def patch_match_stereo(self, images, problems, options=None, return_sel_prob=True, **kw):
        """The controller's two passes (src/mvs/patch_match.cc:201-215), both batched: the photometric pass of ALL problems
        with geom_consistency = filter = False, then, if geom_consistency is asked for, the geometric pass with the depth and
        normal maps of the first as the images' maps.  Without geom_consistency: the one pass as given."""
        assert options is None or not kw, "pass a PatchMatchOptions or keywords, not both"
        o = options if options is not None else default_patch_match_options(**kw)
        if not o.geom_consistency:
            return self.patch_match(images, problems, o, return_sel_prob)
        photo = PatchMatchOptions.from_buffer_copy(o)
        photo.geom_consistency, photo.filter = 0, 0
        first = self.patch_match(images, problems, photo, return_sel_prob=False)
        fed = [dict(im) for im in images]
        for p, r in zip(problems, first):
            fed[p[0]]["depth_map"], fed[p[0]]["normal_map"] = r["depth"], r["normal"]
        return self.patch_match(fed, problems, o, return_sel_prob)

    def patch_match_time(self):
        """dsm_get_patch_match_time: {stage: ms} of the last patch_match call (HIP events, summed over its chunks)."""
        ms = (ctypes.c_double * len(PATCH_MATCH_STAGES))()
        self._chk(self._L.dsm_get_patch_match_time(self._h, ctypes.addressof(ms)))
        return dict(zip(PATCH_MATCH_STAGES, list(ms)))

    def select_source_images(self, R, T, xyz, tracks, options=None, candidate_mask=None, **kw):
        """dsm_select_source_images: Model::GetMaxOverlappingImages, ComputeDepthRanges, ComputeSharedPoints and
        ComputeTriangulationAngles of one sparse model.  R [n][9], T [n][3], xyz [m][3] float32; tracks: the image indices of
        every point (a list of lists, or the CSR pair (offsets, images)); candidate_mask: only images with a non-zero entry may
        be chosen as sources (ReadProblems' condition); options: a SourceSelectionOptions, or its fields as keywords.
        -> {"sources": a list per image, most shared points first, "depth_ranges": [n][2] float32, "pairs": (a, b, count, angle)
        arrays in ascending (a, b) with a < b, "stats": the counts items, pairs and nan_items}."""
        assert options is None or not kw, "pass a SourceSelectionOptions or keywords, not both"
        o = options if options is not None else default_source_selection_options(**kw)
        R, T, xyz, offs, idx, mask = _selection_call_arguments(R, T, xyz, tracks, candidate_mask)
        n = len(R)
        ranges = np.zeros((max(n, 1), 2), dtype=np.float32)
        n_list, n_pairs = ctypes.c_uint64(0), ctypes.c_uint64(0)
        rc = self._L.dsm_select_source_images(self._h, ctypes.byref(o), n, R.ctypes.data, T.ctypes.data, len(xyz), xyz.ctypes.data, offs.ctypes.data,
                                              idx.ctypes.data, None if mask is None else mask.ctypes.data, ranges.ctypes.data,
                                              ctypes.byref(n_list), ctypes.byref(n_pairs))
        if rc != 0:
            self._fail("dsm_select_source_images", rc)
        loff = np.zeros(n + 1, dtype=np.uint64)
        limg = np.zeros(max(int(n_list.value), 1), dtype=np.uint32)
        rec = np.zeros(max(int(n_pairs.value), 1), dtype=IMAGE_OVERLAP_DTYPE)
        self._chk(self._L.dsm_get_source_images(self._h, loff.ctypes.data, limg.ctypes.data, len(limg)))
        self._chk(self._L.dsm_get_image_overlap(self._h, rec.ctypes.data, len(rec)))
        times = self.source_selection_time()
        stats = {"items": int(times["items_count"]), "pairs": int(times["pairs"]), "nan_items": int(times["nan_items"])}
        return _selection_result(n, ranges, loff, limg, rec[:int(n_pairs.value)], stats)

    def source_selection_time(self):
        """dsm_get_source_selection_time: {stage: ms} of the last select_source_images call, with its counts items_count, pairs
        and nan_items."""
        ms = (ctypes.c_double * len(SOURCE_SELECTION_STAGES))()
        self._chk(self._L.dsm_get_source_selection_time(self._h, ctypes.addressof(ms)))
        return dict(zip(SOURCE_SELECTION_STAGES, list(ms)))

    def patch_match_problems(self, model, config, options=None, select=None):
        """PatchMatchController::ReadWorkspace's depth ranges and ReadProblems (src/mvs/patch_match.cc:255, 258-393) on the device:
        the (ref, src_images, depth_min, depth_max) tuples Context.patch_match_stereo takes.  model: a dict with R, T, xyz,
        tracks and either image_names or nothing (then the names are "0", "1", ...); config: the lines of patch-match.cfg, or
        the list parse_patch_match_config returns; options: a dict with min_triangulation_angle (default 1.0), depth_min and
        depth_max (default -1: from the depth ranges).  The rules are patch_match_problems_from's.  select: the selection to run
        in place of the device's (the CPU tests pass capi.selection_host)."""
        options = dict(options or {})
        n = len(np.asarray(model["R"]).reshape(-1, 9))
        if config and isinstance(config[0], str):
            config = parse_patch_match_config(config, model.get("image_names") or [str(i) for i in range(n)])
        mask, max_num = patch_match_selection_arguments(config, n)
        run = select if select is not None else self.select_source_images
        selection = run(model["R"], model["T"], model["xyz"], model["tracks"], candidate_mask=mask, max_num_src_images=max_num,
                        min_triangulation_angle=float(options.get("min_triangulation_angle", 1.0)))
        return patch_match_problems_from(selection, config, options.get("depth_min", -1.0), options.get("depth_max", -1.0))

    def stereo_fusion(self, images, overlap, options=None, **kw):
        """dsm_fuse_stereo (StereoFusion::Run): the dense point cloud of the depth and normal maps.
        images: a list of dicts -- used, depth [h][w], normal [3][h][w] float32, rgb [bh][bw][3] uint8, P [12], inv_P [12], inv_R
        [9] (capi.fusion_matrices), optionally scale [2]; overlap: overlapping_images_, a list of index lists (capi.
        overlapping_images).  options: a StereoFusionOptions, or its fields as keywords over the defaults.
        -> (points [N][3] float32, colours [N][3] uint8, normals [N][3] float32, visibility: N ascending index lists), the points
        in the reference's order."""
        assert options is None or not kw, "pass a StereoFusionOptions or keywords, not both"
        o = options if options is not None else default_stereo_fusion_options(**kw)
        arr, offs, idx, keep = _fusion_call_arguments(images, overlap)
        n = ctypes.c_uint64(0)
        rc = self._L.dsm_fuse_stereo(self._h, ctypes.byref(o), len(images), ctypes.addressof(arr), offs.ctypes.data, idx.ctypes.data, ctypes.byref(n))
        if rc != 0:
            self._fail("dsm_fuse_stereo", rc)
        n = int(n.value)
        rec = np.zeros(max(n, 1), dtype=FUSED_POINT_DTYPE)
        voff = np.zeros(n + 1, dtype=np.uint64)
        self._chk(self._L.dsm_get_fused_points(self._h, None, 0, voff.ctypes.data, None, 0))
        vimg = np.zeros(max(int(voff[-1]), 1), dtype=np.uint32)
        self._chk(self._L.dsm_get_fused_points(self._h, rec.ctypes.data, len(rec), voff.ctypes.data, vimg.ctypes.data, len(vimg)))
        rec = rec[:n]
        vis = [vimg[int(voff[k]):int(voff[k + 1])].tolist() for k in range(n)]
        return rec["xyz"].copy(), rec["rgb"].copy(), rec["normal"].copy(), vis

    def stereo_fusion_time(self):
        """dsm_get_stereo_fusion_time: {stage: ms} of the last stereo_fusion call, with its rounds and seed traversals (counts)."""
        ms = (ctypes.c_double * len(STEREO_FUSION_STAGES))()
        self._chk(self._L.dsm_get_stereo_fusion_time(self._h, ctypes.addressof(ms)))
        return dict(zip(STEREO_FUSION_STAGES, list(ms)))

    def stereo_fusion_rounds(self, n_images):
        """dsm_get_stereo_fusion_rounds -> (order_pos [n_images], rounds [n_images]) of the last stereo_fusion call."""
        pos = np.zeros(max(n_images, 1), dtype=np.uint32)
        rounds = np.zeros(max(n_images, 1), dtype=np.uint32)
        self._chk(self._L.dsm_get_stereo_fusion_rounds(self._h, pos.ctypes.data, rounds.ctypes.data, len(pos)))
        return pos[:n_images], rounds[:n_images]

    @staticmethod
    def apply_point_filter(scene, result):
        """The scene dict reduced to the survivors of a filter_points3D result, ready for bundle_adjust: the points that are
        kept, their compacted tracks, the per-point arrays gathered; cameras and images as they are."""
        keep = np.asarray(result["point_keep"], bool)
        koff = np.asarray(result["kept_track_offsets"], np.int64)
        kobs = np.asarray(result["kept_obs"], np.int64)
        out = dict(scene)
        out["track_offsets"] = np.concatenate([[0], np.cumsum((koff[1:] - koff[:-1])[keep])]).astype(np.uint32)
        out["obs_image"] = np.ascontiguousarray(scene["obs_image"], np.uint32).reshape(-1)[kobs]
        out["obs_xy"] = np.ascontiguousarray(scene["obs_xy"], np.float64).reshape(-1, 2)[kobs]
        out["xyz"] = np.ascontiguousarray(scene["xyz"], np.float64).reshape(-1, 3)[keep]
        for key in ("point_ids", "point_constant"):
            if scene.get(key) is not None:
                out[key] = np.asarray(scene[key])[keep]
        return out

    def retriangulate(self, scene, separators, options=None, next_point3D_id=0):
        """dsm_retriangulate (IncrementalTriangulator::TriangulateImage over the separators).  scene: a dict with
        camera_ids [C], cameras (a list of Camera), image_ids [N], image_camera_ids [N], registered [N], qvec [N, 4], tvec [N, 3],
        points2D_offsets [N + 1], points2D_xy [T, 2], points2D_point3D [T] (index into the points3D or -1), point3D_ids [P],
        point3D_xyz [P, 3], pairs [K, 2] (image ids), match_offsets [K + 1], matches [m, 2].  separators: image ids.
        Returns a dict: new_point_ids, new_xyz [n, 3], new_track_offsets [n + 1], new_track_obs [., 2] (image_id, point2D_idx),
        continued_obs [c, 2], continued_point_ids [c], touched_obs [t, 2], touched_point_ids [t], num_tris_per_separator,
        num_tris, report."""
        a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
        cam_ids = a("camera_ids", np.uint32)
        cams = (Camera * max(len(cam_ids), 1))(*scene["cameras"])
        img_ids, img_cam, reg = a("image_ids", np.uint32), a("image_camera_ids", np.uint32), a("registered", np.uint8)
        N = len(img_ids)
        qvec, tvec = a("qvec", np.float64, (N, 4)), a("tvec", np.float64, (N, 3))
        poff = a("points2D_offsets", np.uint32)
        xy, p3 = a("points2D_xy", np.float64, (-1, 2)), a("points2D_point3D", np.int32)
        pids, pxyz = a("point3D_ids", np.uint64), a("point3D_xyz", np.float64, (-1, 3))
        pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
        seps = np.ascontiguousarray(separators, np.uint32).reshape(-1)
        T = max(int(poff[-1]) if len(poff) else 0, 1)
        nid, nxyz, noff = np.zeros(T, np.uint64), np.zeros((T, 3)), np.zeros(T + 1, np.uint64)
        nobs, cobs, cid = np.zeros((T, 2), np.uint32), np.zeros((T, 2), np.uint32), np.zeros(T, np.uint64)
        tobs, tid = np.zeros((T, 2), np.uint32), np.zeros(T, np.uint64)
        sep_tris = np.zeros(max(len(seps), 1), np.uint32)
        nn, nc, nt, tris = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rep = TriangulationReport()
        o = options if options is not None else default_triangulation_options()
        ptr = lambda x: x.ctypes.data
        self._chk(self._L.dsm_retriangulate(self._h, len(cam_ids), ptr(cam_ids), ctypes.addressof(cams), N, ptr(img_ids), ptr(img_cam),
                                            ptr(reg), ptr(qvec), ptr(tvec), ptr(poff), ptr(xy), ptr(p3), len(pids), ptr(pids), ptr(pxyz),
                                            len(pairs), ptr(pairs), ptr(moff), ptr(m), len(seps), ptr(seps), int(next_point3D_id),
                                            ctypes.byref(o), ptr(nid), ptr(nxyz), ptr(noff), ptr(nobs), ctypes.addressof(nn), ptr(cobs),
                                            ptr(cid), ctypes.addressof(nc), ptr(tobs), ptr(tid), ctypes.addressof(nt), ptr(sep_tris),
                                            ctypes.addressof(tris), ctypes.addressof(rep)))
        n, c, t = nn.value, nc.value, nt.value
        return {"new_point_ids": nid[:n].copy(), "new_xyz": nxyz[:n].copy(), "new_track_offsets": noff[:n + 1].copy(),
                "new_track_obs": nobs[:int(noff[n])].copy(), "continued_obs": cobs[:c].copy(), "continued_point_ids": cid[:c].copy(),
                "touched_obs": tobs[:t].copy(), "touched_point_ids": tid[:t].copy(),
                "num_tris_per_separator": sep_tris[:len(seps)].copy(), "num_tris": tris.value, "report": rep}

    def retriangulate_pairs(self, scene, options=None, re_num_trials=None, next_point3D_id=0):
        """dsm_retriangulate_pairs (IncrementalTriangulator::Retriangulate).  scene: the dict of retriangulate.
        re_num_trials [K]: the trials every pair has had, in the order of scene["pairs"]; None = zeros.
        Returns a dict: new_point_ids, new_xyz [n, 3], new_track_obs [n, 2, 2] ((image_id, point2D_idx) of image1, then image2),
        continued_obs [c, 2], continued_point_ids [c], touched_obs [t, 2], touched_point_ids [t], pair_num_total_corrs [K],
        pair_num_tri_corrs [K] (after the call), pair_status [K] (PAIR_*), re_num_trials [K] (updated), num_tris, report."""
        a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
        cam_ids = a("camera_ids", np.uint32)
        cams = (Camera * max(len(cam_ids), 1))(*scene["cameras"])
        img_ids, img_cam, reg = a("image_ids", np.uint32), a("image_camera_ids", np.uint32), a("registered", np.uint8)
        N = len(img_ids)
        qvec, tvec = a("qvec", np.float64, (N, 4)), a("tvec", np.float64, (N, 3))
        poff = a("points2D_offsets", np.uint32)
        xy, p3 = a("points2D_xy", np.float64, (-1, 2)), a("points2D_point3D", np.int32)
        pids, pxyz = a("point3D_ids", np.uint64), a("point3D_xyz", np.float64, (-1, 3))
        pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
        K = len(pairs)
        trials = np.zeros(max(K, 1), np.uint32)
        if re_num_trials is not None:
            given = np.ascontiguousarray(re_num_trials, np.uint32).reshape(-1)
            if len(given) != K:
                raise DsmError("retriangulate_pairs: re_num_trials must hold one entry per pair")
            trials[:K] = given
        T = max(int(poff[-1]) if len(poff) else 0, 1)
        nid, nxyz, nobs = np.zeros(T, np.uint64), np.zeros((T, 3)), np.zeros((T, 2, 2), np.uint32)
        cobs, cid = np.zeros((T, 2), np.uint32), np.zeros(T, np.uint64)
        tobs, tid = np.zeros((T, 2), np.uint32), np.zeros(T, np.uint64)
        total, tri, status = np.zeros(max(K, 1), np.uint32), np.zeros(max(K, 1), np.uint32), np.zeros(max(K, 1), np.uint8)
        nn, nc, nt, tris = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        rep = PairRetriangulationReport()
        o = options if options is not None else default_pair_retriangulation_options()
        ptr = lambda x: x.ctypes.data
        self._chk(self._L.dsm_retriangulate_pairs(self._h, len(cam_ids), ptr(cam_ids), ctypes.addressof(cams), N, ptr(img_ids),
                                                  ptr(img_cam), ptr(reg), ptr(qvec), ptr(tvec), ptr(poff), ptr(xy), ptr(p3), len(pids),
                                                  ptr(pids), ptr(pxyz), K, ptr(pairs), ptr(moff), ptr(m), int(next_point3D_id),
                                                  ctypes.byref(o), ptr(trials), ptr(nid), ptr(nxyz), ptr(nobs), ctypes.addressof(nn),
                                                  ptr(cobs), ptr(cid), ctypes.addressof(nc), ptr(tobs), ptr(tid), ctypes.addressof(nt),
                                                  ptr(total), ptr(tri), ptr(status), ctypes.addressof(tris), ctypes.addressof(rep)))
        n, c, t = nn.value, nc.value, nt.value
        return {"new_point_ids": nid[:n].copy(), "new_xyz": nxyz[:n].copy(), "new_track_obs": nobs[:n].copy(),
                "continued_obs": cobs[:c].copy(), "continued_point_ids": cid[:c].copy(), "touched_obs": tobs[:t].copy(),
                "touched_point_ids": tid[:t].copy(), "pair_num_total_corrs": total[:K].copy(), "pair_num_tri_corrs": tri[:K].copy(),
                "pair_status": status[:K].copy(), "re_num_trials": trials[:K].copy(), "num_tris": tris.value, "report": rep}

    def update_tracks(self, scene, steps, selected=None, next_point3D_id=0, options=None, **kw):
        """dsm_update_tracks (CompleteTracks / MergeTracks).  scene: the dict of retriangulate (points2D_point3D is not
        read) with track_offsets [P + 1] and track_obs [n, 2] ((image_id, point2D_idx) per element, in track order).  steps: a list
        of TRACKS_MERGE / TRACKS_COMPLETE; selected: point3D ids (None = all points, a snapshot per step).
        Returns a dict in ascending id: point_ids, xyz [n, 3], track_offsets [n + 1], track_obs [m, 2], modified (ids),
        step_counts (num_merged / num_completed per step), report."""
        assert options is None or not kw, "pass a TrackUpdateOptions or keywords, not both"
        o = options if options is not None else default_track_update_options(**kw)
        rc, out = _update_tracks(lambda args: self._L.dsm_update_tracks(self._h, *args), scene, steps, selected, next_point3D_id, o)
        self._chk(rc)
        return out

    def complete_and_merge_tracks(self, scene, **kw):
        """IncrementalMapper::CompleteAndMergeTracks: COMPLETE, then MERGE, over all points."""
        return self.update_tracks(scene, [TRACKS_COMPLETE, TRACKS_MERGE], None, **kw)

    def merge_and_complete_tracks(self, scene, ids, **kw):
        """The order of AdjustLocalBundle: MERGE, then COMPLETE, over one id set."""
        return self.update_tracks(scene, [TRACKS_MERGE, TRACKS_COMPLETE], ids, **kw)

    def complete_images(self, scene, image_ids, steps=(), selected=None, next_point3D_id=0, options=None, **kw):
        """dsm_complete_images (IncrementalTriangulator::CompleteImage): the steps of update_tracks first (there may
        be none), then CompleteImage of every listed image in the given order, over one state on the device.  Returns the dict
        of update_tracks (new points included, in ascending id) plus image_num_tris (what CompleteImage returns per image) and
        the CompleteImagesReport as report.  capi.apply_track_update takes the result as it is."""
        assert options is None or not kw, "pass a TrackUpdateOptions or keywords, not both"
        o = options if options is not None else default_track_update_options(**kw)
        rc, out = _update_tracks(lambda args: self._L.dsm_complete_images(self._h, *args), scene, list(steps), selected, next_point3D_id, o,
                                 complete_images=image_ids)
        self._chk(rc)
        return out

    def adjust_local_bundle_tracks(self, scene, image_id, variable_ids, **kw):
        """The tail of IncrementalMapper::AdjustLocalBundle in one call: MergeTracks and CompleteTracks over the variable point
        ids, then CompleteImage of the image.  Adds num_merged_observations and num_completed_observations as the reference's
        report sums them (CompleteTracks + CompleteImage)."""
        out = self.complete_images(scene, [image_id], [TRACKS_MERGE, TRACKS_COMPLETE], variable_ids, **kw)
        out["num_merged_observations"] = int(out["step_counts"][0])
        out["num_completed_observations"] = int(out["step_counts"][1]) + int(out["image_num_tris"][0])
        return out

    def find_initial_pairs(self, scene, problems, options=None, **kw):
        """dsm_find_initial_pairs (FindInitialImagePair, EstimateInitialTwoViewGeometry and the triangulation of
        RegisterInitialImagePair for a batch of reconstructions).  scene: the dict of retriangulate (camera_ids,
        cameras, image_ids, image_camera_ids, points2D_offsets, points2D_xy, pairs, match_offsets, matches; its other keys are
        not read).  problems: a list of dicts with image_ids and, optionally, num_registrations and init_num_reg_trials (aligned
        with image_ids), tried_pairs [(id, id)], seed_image1, seed_image2 (None = no seed).
        Returns a dict: results (a list of dicts per problem: found, image_id1, image_id2, two_view_geometry, inlier_matches
        [i, 2], num_tried, tried_pairs [t, 2] in trial order with the successful pair last, new_xyz [n, 3] and new_track_obs [n, 2, 2]
        ((image_id, point2D_idx) of image 1, then image 2, as retriangulate_pairs returns new points)) and report."""
        assert options is None or not kw, "pass an InitialPairOptions or keywords, not both"
        o = options if options is not None else default_initial_pair_options(**kw)
        a = lambda key, dt, shape=-1: np.ascontiguousarray(scene[key], dt).reshape(shape)
        cam_ids = a("camera_ids", np.uint32)
        cams = (Camera * max(len(cam_ids), 1))(*scene["cameras"])
        img_ids, img_cam = a("image_ids", np.uint32), a("image_camera_ids", np.uint32)
        poff, xy = a("points2D_offsets", np.uint32), a("points2D_xy", np.float64, (-1, 2))
        pairs, moff, m = a("pairs", np.uint32, (-1, 2)), a("match_offsets", np.uint64), a("matches", np.uint32, (-1, 2))
        prob_off, prob_ids, regs, trials, toff, tried, s1, s2, max_tried, max_points = _initial_pair_problem_arguments(scene, problems)
        B = len(problems)
        res = (InitialPairResult * max(B, 1))()
        out_toff, out_tried = np.zeros(B + 1, np.uint64), np.zeros((max(max_tried, 1), 2), np.uint32)
        out_poff, out_xyz, out_obs = np.zeros(B + 1, np.uint64), np.zeros((max(max_points, 1), 3)), np.zeros((max(max_points, 1), 2), np.uint32)
        out_ioff, out_inl = np.zeros(B + 1, np.uint64), np.zeros((max(max_points, 1), 2), np.uint32)
        rep = InitialPairReport()
        ptr = lambda x: x.ctypes.data
        self._chk(self._L.dsm_find_initial_pairs(self._h, len(cam_ids), ptr(cam_ids), ctypes.addressof(cams), len(img_ids), ptr(img_ids),
                                                 ptr(img_cam), ptr(poff), ptr(xy), len(pairs), ptr(pairs), ptr(moff), ptr(m), B, ptr(prob_off),
                                                 ptr(prob_ids), ptr(regs), ptr(trials), ptr(toff), ptr(tried), ptr(s1), ptr(s2), ctypes.byref(o),
                                                 ctypes.addressof(res), ptr(out_toff), ptr(out_tried), len(out_tried), ptr(out_poff),
                                                 ptr(out_xyz), ptr(out_obs), len(out_xyz), ptr(out_ioff), ptr(out_inl), len(out_inl),
                                                 ctypes.addressof(rep)))
        results = []
        for k in range(B):
            r = res[k]
            t0, t1, p0, p1 = int(out_toff[k]), int(out_toff[k + 1]), int(out_poff[k]), int(out_poff[k + 1])
            obs = np.zeros((p1 - p0, 2, 2), np.uint32)
            obs[:, 0, 0], obs[:, 1, 0] = r.image_id1, r.image_id2
            obs[:, 0, 1], obs[:, 1, 1] = out_obs[p0:p1, 0], out_obs[p0:p1, 1]
            results.append({"found": r.status == INITIAL_PAIR_FOUND, "image_id1": int(r.image_id1), "image_id2": int(r.image_id2),
                            "two_view_geometry": TwoViewGeometry.from_buffer_copy(bytes(r.two_view_geometry)),
                            "inlier_matches": out_inl[int(out_ioff[k]):int(out_ioff[k + 1])].copy(), "num_tried": int(r.num_tried),
                            "tried_pairs": out_tried[t0:t1].copy(), "new_xyz": out_xyz[p0:p1].copy(), "new_track_obs": obs})
        return {"results": results, "report": rep}

    def find_next_images(self, scene, problems, options=None, capacity=None, **kw):
        """dsm_find_next_images (IncrementalMapper::FindNextImages for a batch of reconstructions, stateless).
        scene: the dict of find_initial_pairs.  problems: a list of dicts with image_ids, registered (0 / 1 per image),
        obs_point3D (one int32 array per image: the point of every point2D or -1) and, optionally, num_reg_trials and filtered
        (per image).  Returns a dict: results (per problem a dict: next_image_ids in the order to try them, and per image of
        the problem num_visible, num_observations, score) and report.  On an error the DsmError carries the output arrays as
        .outputs (untouched by an invalid call)."""
        assert options is None or not kw, "pass a NextImagesOptions or keywords, not both"
        o = options if options is not None else default_next_images_options(**kw)
        args, keep, S = _next_images_arguments(scene, problems)
        B = len(problems)
        off, out = np.zeros(B + 1, np.uint64), np.zeros(max(S if capacity is None else capacity, 1), np.uint32)
        nv, no, score = np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint32), np.zeros(max(S, 1), np.uint64)
        rep = NextImagesReport()
        ptr = lambda x: x.ctypes.data
        try:
            self._chk(self._L.dsm_find_next_images(self._h, *args, ctypes.byref(o), ptr(off), ptr(out), S if capacity is None else capacity,
                                                   ptr(nv), ptr(no), ptr(score), ctypes.addressof(rep)))
        except DsmError as e:
            e.outputs = (off, out, nv, no, score)
            raise
        return {"results": _next_images_result(problems, S, off, out, nv, no, score), "report": rep}

    def find_local_bundles(self, scene, problems, queries, options=None, bundle_capacity=None, overlap_capacity=None, **kw):
        """dsm_find_local_bundles (IncrementalMapper::FindLocalBundle for a batch of registered images, stateless; DESIGN.md
        30).  scene: image_ids and points2D_offsets are read.  problems: as find_next_images takes them, with qvec [n, 4] and
        tvec [n, 3] per image and point_xyz [m, 3].  queries: [(problem index, image id)].  Returns a dict: results (per query
        a dict: bundle_image_ids, and the overlap list in overlap order: overlap_image_ids, overlap_shared, overlap_tri_angle
        with -1 where no threshold could reach the image) and report.  On an error the DsmError carries the output arrays as
        .outputs (untouched by an invalid call)."""
        assert options is None or not kw, "pass a LocalBundleSelectionOptions or keywords, not both"
        o = options if options is not None else default_local_bundle_selection_options(**kw)
        head, tail, keep, out = _local_bundles_arguments(scene, problems, queries, (bundle_capacity, overlap_capacity))
        rep = LocalBundleSelectionReport()
        try:
            self._chk(self._L.dsm_find_local_bundles(self._h, *head, ctypes.byref(o), *tail, ctypes.addressof(rep)))
        except DsmError as e:
            e.outputs = out
            raise
        return {"results": _local_bundles_result(queries, out), "report": rep}

    def estimate_absolute_poses(self, cameras, estimate_focal_length, offsets, points2D, points3D, options=None, seeds=None):
        """dsm_estimate_absolute_poses (EstimateAbsolutePose for a batch of problems).  cameras: a list of Camera
        [B]; estimate_focal_length [B]; offsets [B + 1] (CSR over the problems); points2D [T, 2] pixels; points3D [T, 3]; seeds:
        None or [B, S] with S = len(absolute_pose_factors(options)).  Returns a dict: results (a list of AbsolutePoseResult),
        inlier_mask [T] uint8, margins [B, 9] (ABSOLUTE_POSE_MARGINS), report."""
        B = len(cameras)
        cams = (Camera * max(B, 1))(*cameras)
        flags = np.ascontiguousarray(estimate_focal_length, np.uint8).reshape(-1)
        offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        p2 = np.ascontiguousarray(points2D, np.float64).reshape(-1, 2)
        p3 = np.ascontiguousarray(points3D, np.float64).reshape(-1, 3)
        if len(flags) != B or len(offs) != B + 1 or len(p2) != len(p3) or (B and int(offs[-1]) > len(p2)):
            raise DsmError("estimate_absolute_poses: array sizes do not match")
        o = options if options is not None else default_absolute_pose_options()
        sd = None if seeds is None else np.ascontiguousarray(seeds, np.uint32).reshape(-1)
        if sd is not None and len(sd) != B * len(absolute_pose_factors(o)):
            raise DsmError("estimate_absolute_poses: seeds must hold B * S entries")
        res = (AbsolutePoseResult * max(B, 1))()
        mask = np.zeros(max(len(p2), 1), np.uint8)
        margins = np.zeros((max(B, 1), len(ABSOLUTE_POSE_MARGINS)))
        rep = AbsolutePoseReport()
        ptr = lambda x: x.ctypes.data
        self._chk(self._L.dsm_estimate_absolute_poses(self._h, B, ctypes.addressof(cams), ptr(flags), ptr(offs), ptr(p2), ptr(p3),
                                                      ctypes.byref(o), None if sd is None else ptr(sd), ctypes.addressof(res),
                                                      ptr(mask), ptr(margins), ctypes.addressof(rep)))
        return {"results": [res[b] for b in range(B)], "inlier_mask": mask[:len(p2)].copy(), "margins": margins[:B].copy(),
                "report": rep}

    def refine_absolute_poses(self, cameras, offsets, points2D, points3D, inlier_mask, qvecs, tvecs, refine_flags, options=None):
        """dsm_refine_absolute_poses (RefineAbsolutePose for a batch of problems), on the layout of
        estimate_absolute_poses.  inlier_mask [T]; qvecs [B, 4]; tvecs [B, 3]; refine_flags [B] (POSE_REFINE_* bits).  Returns a
        dict: results (a list of PoseRefinementResult), margins [B, 5] (POSE_REFINEMENT_MARGINS), steps (a list of uint8 arrays,
        POSE_STEP_* per iteration of a problem), report."""
        B = len(cameras)
        cams = (Camera * max(B, 1))(*cameras)
        offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        p2 = np.ascontiguousarray(points2D, np.float64).reshape(-1, 2)
        p3 = np.ascontiguousarray(points3D, np.float64).reshape(-1, 3)
        mask = np.ascontiguousarray(inlier_mask, np.uint8).reshape(-1)
        q = np.ascontiguousarray(qvecs, np.float64).reshape(-1, 4)
        t = np.ascontiguousarray(tvecs, np.float64).reshape(-1, 3)
        flags = np.ascontiguousarray(refine_flags, np.uint8).reshape(-1)
        if (len(offs) != B + 1 or len(p2) != len(p3) or len(mask) != len(p2) or (B and int(offs[-1]) > len(p2)) or len(q) != B
                or len(t) != B or len(flags) != B):
            raise DsmError("refine_absolute_poses: array sizes do not match")
        o = options if options is not None else default_pose_refinement_options()
        cap = max(int(o.max_num_iterations), 0)
        res = (PoseRefinementResult * max(B, 1))()
        margins = np.zeros((max(B, 1), len(POSE_REFINEMENT_MARGINS)))
        steps = np.zeros((max(B, 1), max(cap, 1)), np.uint8)
        rep = PoseRefinementReport()
        ptr = lambda x: x.ctypes.data
        self._chk(self._L.dsm_refine_absolute_poses(self._h, B, ctypes.addressof(cams), ptr(offs), ptr(p2), ptr(p3), ptr(mask), ptr(q),
                                                    ptr(t), ptr(flags), ctypes.byref(o), ctypes.addressof(res), ptr(margins),
                                                    ptr(steps), ctypes.addressof(rep)))
        return {"results": [res[b] for b in range(B)], "margins": margins[:B].copy(),
                "steps": [steps[b, :min(res[b].num_iterations, cap)].copy() for b in range(B)], "report": rep}

    def adjust_local_bundles(self, problems, options=None, trace=True):
        """dsm_adjust_local_bundles: a batch of independent local bundle adjustments in one launch.  problems: a
        list of dicts in bundle_adjust's scene layout plus camera_constant [C] (optional), e.g. from capi.local_bundle_problem;
        a track of length 1 is accepted.  The inputs are not modified.  Returns a dict: problems (a list of dicts with
        camera_params, qvec, tvec, xyz updated, result (LocalBundleResult), margins (a dict by LOCAL_BUNDLE_MARGINS), trace
        [iterations + 1, 5]: cost, radius, rho, accepted, gradient max-norm) and report (LocalBundleReport)."""
        B = len(problems)
        o = options if options is not None else default_local_bundle_options()
        cat = lambda parts, dt: np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0), dt).reshape(-1)
        arr = lambda pr, key, dt: np.asarray(pr[key], dt).reshape(-1)
        flag = lambda pr, key, n: np.zeros(n, np.uint8) if pr.get(key) is None else np.asarray(pr[key], np.uint8).reshape(n)
        nC = [len(arr(pr, "camera_model_ids", np.int32)) for pr in problems]
        nI = [len(arr(pr, "image_camera", np.uint32)) for pr in problems]
        nP = [len(arr(pr, "track_offsets", np.uint32)) - 1 for pr in problems]
        nO = [len(arr(pr, "obs_image", np.uint32)) for pr in problems]
        for b, pr in enumerate(problems):
            ids = pr.get("point_ids")
            mids = arr(pr, "camera_model_ids", np.int32)
            if all(0 <= m < len(CAMERA_MODEL_NUM_PARAMS) for m in mids):  # (an unknown model is refused by the library before it reads a parameter)
                if len(arr(pr, "camera_params", np.float64)) != sum(CAMERA_MODEL_NUM_PARAMS[m] for m in mids):
                    raise DsmError("adjust_local_bundles: camera_params of problem %d does not hold its models' parameter counts" % b)
            if (len(arr(pr, "qvec", np.float64)) != 4 * nI[b] or len(arr(pr, "tvec", np.float64)) != 3 * nI[b]
                    or len(arr(pr, "xyz", np.float64)) != 3 * nP[b] or len(arr(pr, "obs_xy", np.float64)) != 2 * nO[b]
                    or (ids is not None and len(np.asarray(ids).reshape(-1)) != nP[b])):
                raise DsmError("adjust_local_bundles: array sizes of problem %d do not match" % b)
        off = lambda n, dt: np.concatenate([[0], np.cumsum(n)]).astype(dt)
        coff, ioff, poff, ooff = off(nC, np.uint32), off(nI, np.uint32), off(nP, np.uint32), off(nO, np.uint64)
        models = cat([arr(pr, "camera_model_ids", np.int32) for pr in problems], np.int32)
        params = cat([arr(pr, "camera_params", np.float64) for pr in problems], np.float64).copy()
        cconst = cat([flag(pr, "camera_constant", nC[b]) for b, pr in enumerate(problems)], np.uint8)
        icam = cat([arr(pr, "image_camera", np.uint32) for pr in problems], np.uint32)
        qvec = cat([arr(pr, "qvec", np.float64) for pr in problems], np.float64).copy()
        tvec = cat([arr(pr, "tvec", np.float64) for pr in problems], np.float64).copy()
        cpose = cat([flag(pr, "image_constant_pose", nI[b]) for b, pr in enumerate(problems)], np.uint8)
        cmask = cat([flag(pr, "image_constant_tvec", nI[b]) for b, pr in enumerate(problems)], np.uint8)
        pids = cat([np.arange(nP[b], dtype=np.uint64) if pr.get("point_ids") is None else arr(pr, "point_ids", np.uint64)
                    for b, pr in enumerate(problems)], np.uint64)
        xyz = cat([arr(pr, "xyz", np.float64) for pr in problems], np.float64).copy()
        pconst = cat([flag(pr, "point_constant", nP[b]) for b, pr in enumerate(problems)], np.uint8)
        toff = cat([arr(pr, "track_offsets", np.uint32) for pr in problems], np.uint32)
        oimg = cat([arr(pr, "obs_image", np.uint32) for pr in problems], np.uint32)
        oxy = cat([arr(pr, "obs_xy", np.float64) for pr in problems], np.float64)
        rows = max(int(o.max_num_iterations), 0) + 1
        res = (LocalBundleResult * max(B, 1))()
        margins = np.zeros((max(B, 1), len(LOCAL_BUNDLE_MARGINS)))
        tr = np.full((max(B, 1), rows, LOCAL_BUNDLE_TRACE_COLUMNS), np.nan) if trace else None
        rep = LocalBundleReport()
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self._L.dsm_adjust_local_bundles(self._h, B, ptr(coff), ptr(models), ptr(params), ptr(cconst), ptr(ioff), ptr(icam),
                                                   ptr(qvec), ptr(tvec), ptr(cpose), ptr(cmask), ptr(poff), ptr(pids), ptr(xyz),
                                                   ptr(pconst), ptr(toff), ptr(ooff), ptr(oimg), ptr(oxy), ctypes.byref(o),
                                                   ctypes.addressof(res), ptr(margins), ptr(tr), ctypes.addressof(rep)))
        out, pa = [], 0
        for b, pr in enumerate(problems):
            npar = sum(CAMERA_MODEL_NUM_PARAMS[m] for m in models[coff[b]:coff[b + 1]])
            r = LocalBundleResult.from_buffer_copy(bytes(res[b]))
            d = {"camera_params": params[pa:pa + npar].copy(), "qvec": qvec.reshape(-1, 4)[ioff[b]:ioff[b + 1]].copy(),
                 "tvec": tvec.reshape(-1, 3)[ioff[b]:ioff[b + 1]].copy(), "xyz": xyz.reshape(-1, 3)[poff[b]:poff[b + 1]].copy(),
                 "result": r, "margins": dict(zip(LOCAL_BUNDLE_MARGINS, margins[b].tolist()))}
            if trace:
                d["trace"] = tr[b, :min(int(r.num_iterations) + 1, rows)].copy() if r.solved else tr[b, :0].copy()
            pa += npar
            out.append(d)
        return {"problems": out, "report": rep}

    def register_images(self, cameras, offsets, points2D, points3D, estimate_focal_length=None, refine_flags=None,
                        abs_pose_min_num_inliers=30, pose_options=None, refinement_options=None, seeds=None):
        """The numerical core of IncrementalMapper::RegisterNextImage (src/sfm/incremental_mapper.cc:438-535) for a batch of images:
        EstimateAbsolutePose, the abs_pose_min_num_inliers test (incremental_mapper.h:87: 30), RefineAbsolutePose on the estimate's
        pose and mask.  estimate_focal_length [B] (default: not camera.has_prior_focal_length, as :451-483 chooses without the
        bogus-parameter history the host keeps); refine_flags [B] (default: focal length and extra parameters).  An image whose
        estimate failed or found too few inliers is not refined.  Returns a dict: registered [B] bool, qvec [B, 4], tvec [B, 3],
        camera_params [B, 12], num_inliers [B], inlier_mask [T], estimate (estimate_absolute_poses' dict), refinement
        (refine_absolute_poses' dict over the images that reached it, or None), refined_index [B] (row in refinement or -1)."""
        B = len(cameras)
        offs = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        p2 = np.ascontiguousarray(points2D, np.float64).reshape(-1, 2)
        p3 = np.ascontiguousarray(points3D, np.float64).reshape(-1, 3)
        est_focal = ([0 if c.has_prior_focal_length else 1 for c in cameras] if estimate_focal_length is None
                     else [int(f) for f in estimate_focal_length])
        flags = [POSE_REFINE_FOCAL_LENGTH | POSE_REFINE_EXTRA_PARAMS] * B if refine_flags is None else [int(f) for f in refine_flags]
        est = self.estimate_absolute_poses(cameras, est_focal, offs, p2, p3, pose_options, seeds)
        qvec, tvec, prm = np.zeros((B, 4)), np.zeros((B, 3)), np.zeros((B, 12))
        registered, refined_index = np.zeros(B, bool), -np.ones(B, np.int64)
        keep, cams2 = [], []
        for b, r in enumerate(est["results"]):
            prm[b] = list(cameras[b].params)
            if not r.success or r.num_inliers < abs_pose_min_num_inliers:
                continue
            cam = Camera.from_buffer_copy(bytes(cameras[b]))
            two = cameras[b].model_id in (1, 4, 5, 6, 7, 10)
            cam.params[0] = r.focal_params[0]  # the winning factor's focal length (pose.cc:146-151)
            if two:
                cam.params[1] = r.focal_params[1]
            refined_index[b] = len(keep)
            keep.append(b)
            cams2.append(cam)
        ref = None
        if keep:
            sub = np.concatenate([[0], np.cumsum([int(offs[b + 1] - offs[b]) for b in keep])]).astype(np.uint64)
            rows = np.concatenate([np.arange(int(offs[b]), int(offs[b + 1])) for b in keep]).astype(np.int64)
            ref = self.refine_absolute_poses(cams2, sub, p2[rows], p3[rows], est["inlier_mask"][rows],
                                             [list(est["results"][b].qvec) for b in keep], [list(est["results"][b].tvec) for b in keep],
                                             [flags[b] for b in keep], refinement_options)
            for k, b in enumerate(keep):
                r = ref["results"][k]
                registered[b] = bool(r.success)
                qvec[b], tvec[b], prm[b] = list(r.qvec), list(r.tvec), list(r.camera_params)
        return {"registered": registered, "qvec": qvec, "tvec": tvec, "camera_params": prm,
                "num_inliers": np.array([r.num_inliers for r in est["results"]], np.int64), "inlier_mask": est["inlier_mask"],
                "estimate": est, "refinement": ref, "refined_index": refined_index}

    def device_info(self):
        d = DeviceInfo()
        self._chk(self._L.dsm_get_device_info(self._h, ctypes.byref(d)))
        return d

    def match_gather_time(self):
        ms = ctypes.c_double(0)
        self._chk(self._L.dsm_get_match_gather_time(self._h, ctypes.byref(ms)))
        return ms.value

    def match_tail_time(self):
        ms = ctypes.c_double()
        self._chk(self._L.dsm_get_match_tail_time(self._h, ctypes.byref(ms)))
        return ms.value

    def match_resolve_time(self):
        ms = ctypes.c_double(0)
        self._chk(self._L.dsm_get_match_resolve_time(self._h, ctypes.byref(ms)))
        return ms.value


_gather_lib = None


def gather_lib():
    """libdagsfm_gather.so (include/dagsfm_gather.h); maps librccl, so it is loaded on first use only."""
    global _gather_lib
    if _gather_lib is None:
        if not os.path.exists(GATHER_LIB_PATH):
            raise DsmError("%s is missing: make -C dagsfm_amd/csrc" % GATHER_LIB_PATH)
        lib()  # the companion links the product library: resolve it to the in-tree one first
        G = ctypes.CDLL(GATHER_LIB_PATH)
        vp = ctypes.c_void_p
        G.dsm_gather_create.argtypes = [ctypes.POINTER(vp), ctypes.c_uint32, ctypes.POINTER(vp)]
        G.dsm_gather_destroy.argtypes = [vp]
        G.dsm_gather_destroy.restype = None
        G.dsm_gather_last_error.argtypes = [vp]
        G.dsm_gather_last_error.restype = ctypes.c_char_p
        G.dsm_gather_match_graph.argtypes = [vp, u32p, ctypes.c_int32]
        G.dsm_gather_sizes.argtypes = [vp, u64p, u64p, u64p]
        G.dsm_gather_fetch.argtypes = [vp, ctypes.c_uint32, vp, vp, vp, vp, vp]
        G.dsm_gather_device_arrays.argtypes = [vp, ctypes.c_uint32] + [ctypes.POINTER(vp)] * 5
        G.dsm_gather_time.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
        _gather_lib = G
    return _gather_lib


class Gather:
    """dsm_gather over product contexts on distinct devices of this process (one context: a one-rank communicator)."""

    def __init__(self, ctxs):
        self.ctxs = list(ctxs)
        assert all(not c.check for c in self.ctxs), "the companion library links the product build"
        self._G = gather_lib()
        arr = (ctypes.c_void_p * len(self.ctxs))(*[c._h for c in self.ctxs])
        self._g = ctypes.c_void_p()
        rc = self._G.dsm_gather_create(arr, len(self.ctxs), ctypes.byref(self._g))
        if rc != 0:
            raise DsmError("dsm_gather_create failed (%d)" % rc)

    def _chk(self, rc):
        if rc != 0:
            raise DsmError("dsm_gather error %d: %s" % (rc, self._G.dsm_gather_last_error(self._g).decode()))

    def close(self):
        if self._g:
            self._G.dsm_gather_destroy(self._g)
            self._g = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def match_graph(self, n_pairs, with_geometry=True, rank=0):
        """Assembles the shares and fetches the graph from `rank`'s device: (match offsets, matches, records, inlier offsets, inlier matches)."""
        npairs = np.ascontiguousarray(n_pairs, np.uint32)
        assert len(npairs) == len(self.ctxs)
        self._chk(self._G.dsm_gather_match_graph(self._g, npairs.ctypes.data_as(u32p), 1 if with_geometry else 0))
        N, M, I = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self._G.dsm_gather_sizes(self._g, ctypes.byref(N), ctypes.byref(M), ctypes.byref(I)))
        moff = np.zeros(N.value + 1, np.uint64)
        m = np.zeros((max(M.value, 1), 2), np.uint32)
        if not with_geometry:
            self._chk(self._G.dsm_gather_fetch(self._g, rank, moff.ctypes.data, m.ctypes.data, None, None, None))
            return moff, m[:M.value]
        tv = (TwoViewGeometry * max(N.value, 1))()
        ioff = np.zeros(N.value + 1, np.uint64)
        im = np.zeros((max(I.value, 1), 2), np.uint32)
        self._chk(self._G.dsm_gather_fetch(self._g, rank, moff.ctypes.data, m.ctypes.data, ctypes.addressof(tv), ioff.ctypes.data, im.ctypes.data))
        return moff, m[:M.value], list(tv)[:N.value], ioff, im[:I.value]

    def time_ms(self):
        ms = ctypes.c_double()
        self._chk(self._G.dsm_gather_time(self._g, ctypes.byref(ms)))
        return ms.value
