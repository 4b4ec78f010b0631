"""ctypes loader of libsrk_ba.so (built in-tree by surikatoko_amd/csrc/Makefile)."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
# SRK_BA_LIBRARY: development only (tools/*.sh load ablation / stamp builds from a temporary path, so that the product
# library in the tree is never overwritten)
_PATH = os.environ.get("SRK_BA_LIBRARY") or os.path.join(_HERE, "libsrk_ba.so")
_lib = None


class LibraryNotBuilt(RuntimeError):
    pass


def library_path():
    return _PATH


def build_library(jobs=4):
    """hipcc --offload-arch=gfx950 build of every HIP translation unit (cross-compiles without a GPU)."""
    subprocess.check_call(["make", "-s", "-j", str(jobs), "-C", os.path.join(_HERE, "csrc")])
    return _PATH


class Report(C.Structure):
    _fields_ = [("status", C.c_int32), ("optimized", C.c_int32), ("iterations", C.c_int64),
                ("attempts", C.c_int64), ("seen", C.c_int64), ("err_initial", C.c_double),
                ("err_final", C.c_double), ("hessian_factor", C.c_double), ("world_scale", C.c_double),
                ("ms_jacobian", C.c_double), ("ms_schur", C.c_double), ("ms_solve", C.c_double),
                ("ms_backsub", C.c_double), ("ms_apply", C.c_double), ("ms_error", C.c_double),
                ("ms_total", C.c_double), ("schur_launches", C.c_int64), ("jacobian_launches", C.c_int64),
                ("ms_jacobian_kernel", C.c_double), ("ms_solve_syrk", C.c_double),
                ("solve_mfma_flops", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Normalizer(C.Structure):
    _fields_ = [("R0", C.c_double * 9), ("T0", C.c_double * 3), ("world_scale", C.c_double)]


class SceneSpecC(C.Structure):
    _fields_ = [("n_frames", C.c_int32), ("grid_nx", C.c_int32), ("grid_ny", C.c_int32), ("vis_window", C.c_int32),
                ("half_extent_x", C.c_double), ("half_extent_y", C.c_double), ("f0", C.c_double),
                ("noise_x3d_hi", C.c_double), ("noise_r_hi", C.c_double), ("noise_uv_pix", C.c_double),
                ("seed", C.c_uint32)]


class MargCounts(C.Structure):
    _fields_ = [("n_drop", C.c_int32), ("n_kept", C.c_int32), ("n_landmarks", C.c_int64), ("n_landmarks_skipped", C.c_int64),
                ("n_observations", C.c_int64), ("n_factors", C.c_int32), ("n_sets", C.c_int32), ("n_frame_priors", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class MargReport(C.Structure):
    _fields_ = [("landmarks_used", C.c_int64), ("landmarks_skipped", C.c_int64), ("factors", C.c_int32), ("sets", C.c_int32),
                ("frame_priors", C.c_int32), ("defect", C.c_double), ("ms_rows", C.c_double), ("ms_gram", C.c_double),
                ("ms_host", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TriOptions(C.Structure):
    _fields_ = [("refine_attempts", C.c_int32), ("refine_rel_change", C.c_double), ("min_parallax_deg", C.c_double)]


class ResectOptions(C.Structure):
    _fields_ = [("attempts", C.c_int32), ("rel_change", C.c_double), ("loss_kind", C.c_int32), ("loss_delta_pixels", C.c_double)]


class LocateOptions(C.Structure):
    _fields_ = [("hypotheses", C.c_int32), ("inlier_pixels", C.c_double), ("seed", C.c_uint64)]


class RelateOptions(C.Structure):
    _fields_ = [("hypotheses", C.c_int32), ("inlier_pixels", C.c_double), ("seed", C.c_uint64)]


class PairOptions(C.Structure):
    _fields_ = [("attempts", C.c_int32), ("rel_change", C.c_double), ("loss_kind", C.c_int32), ("loss_delta_pixels", C.c_double),
                ("inliers_only", C.c_int32)]


class AlignOptions(C.Structure):
    _fields_ = [("hypotheses", C.c_int32), ("inlier_distance", C.c_double), ("seed", C.c_uint64), ("with_scale", C.c_int32),
                ("refine_rounds", C.c_int32)]


class HomographyOptions(C.Structure):
    _fields_ = [("hypotheses", C.c_int32), ("inlier_pixels", C.c_double), ("seed", C.c_uint64), ("refine_rounds", C.c_int32)]


class FundamentalOptions(C.Structure):
    _fields_ = [("hypotheses", C.c_int32), ("inlier_pixels", C.c_double), ("seed", C.c_uint64), ("refine_rounds", C.c_int32)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)

# every symbol include/srk_ba.h declares (checked by tests/test_abi.py)
EXPORTS = [
    "srk_ba_create", "srk_ba_destroy", "srk_ba_last_error", "srk_ba_status_string", "srk_ba_device_count",
    "srk_ba_set_stream", "srk_ba_set_allreduce", "srk_ba_rccl_get_unique_id", "srk_ba_rccl_init", "srk_ba_rccl_init_second", "srk_ba_rccl_set_comm", "srk_ba_compute_inplace", "srk_ba_compute_inplace_f32", "srk_ba_reproj_error", "srk_ba_reproj_error_mvf", "srk_mvf_estimate_depths", "srk_mvf_relative_motion",
    "srk_mvf_project_onto_so3", "srk_ba_set_schur_precision", "srk_ba_set_storage_precision", "srk_ba_set_speculation", "srk_ba_set_deterministic", "srk_ba_deterministic", "srk_ba_set_multi_schedule", "srk_ba_multi_schedule", "srk_ba_set_frame_reordering", "srk_ba_set_frame_order", "srk_ba_frame_order", "srk_frame_order", "srk_ba_set_solver_fusion", "srk_ba_solver_sync_timeouts", "srk_ba_iteration_log", "srk_ba_solver_fusion", "srk_ba_set_jacobian_mode", "srk_ba_jacobian_kernel", "srk_ba_set_fixed_intrinsics", "srk_ba_frame_vars", "srk_ba_schur_fallback_landmarks",
    "srk_ba_set_robust_loss", "srk_ba_robust_loss", "srk_ba_observation_weights",
    "srk_ba_set_observation_information", "srk_ba_observation_information", "srk_ba_observation_residuals",
    "srk_ba_set_intrinsic_groups", "srk_ba_intrinsic_groups", "srk_ba_download_intrinsics",
    "srk_ba_set_constant_blocks", "srk_ba_constant_blocks", "srk_ba_constant_counts", "srk_ba_constant_pass_ms",
    "srk_ba_set_position_priors", "srk_ba_position_prior_counts", "srk_ba_position_priors", "srk_ba_prior_error",
    "srk_ba_prior_residuals", "srk_ba_normalize_position_priors", "srk_ba_prior_pass_ms",
    "srk_ba_set_relative_pose_factors", "srk_ba_check_relative_pose_factors", "srk_ba_relative_pose_factor_count", "srk_ba_relative_pose_factors",
    "srk_ba_relative_pose_error", "srk_ba_relative_pose_residuals", "srk_ba_normalize_relative_pose_factors",
    "srk_ba_relative_pose_pass_ms",
    "srk_ba_set_joint_pose_priors", "srk_ba_check_joint_pose_priors", "srk_ba_joint_pose_prior_counts", "srk_ba_joint_pose_priors",
    "srk_ba_joint_pose_prior_error", "srk_ba_joint_pose_prior_residuals", "srk_ba_normalize_joint_pose_priors",
    "srk_ba_joint_pose_prior_pass_ms",
    "srk_ba_marginalization_plan", "srk_ba_phase_marginalization", "srk_ba_marginalization_prior", "srk_ba_marginalize_dense",
    "srk_ba_revert_marginalization_prior",
    "srk_tri_default_options", "srk_triangulate_tracks", "srk_ba_triangulate", "srk_ba_triangulate_kernel_ms", "srk_tri_check_tracks", "srk_tri_revert_points",
    "srk_resect_default_options", "srk_resect_frames", "srk_ba_resect", "srk_ba_resect_kernel_ms", "srk_resect_check_frames", "srk_resect_revert",
    "srk_locate_default_options", "srk_locate_frames", "srk_ba_locate", "srk_ba_locate_kernel_ms", "srk_ba_locate_score_ms", "srk_locate_check_frames",
    "srk_ransac_hypotheses",
    "srk_relate_default_options", "srk_relate_frames", "srk_ba_relate_kernel_ms", "srk_ba_relate_score_ms", "srk_relate_check_pairs", "srk_relate_host_pair",
    "srk_pair_default_options", "srk_refine_pairs", "srk_relate_frames_refined", "srk_ba_pair_kernel_ms", "srk_pair_check_pairs", "srk_pair_host_pair",
    "srk_pair_factor",
    "srk_align_default_options", "srk_align_points", "srk_ba_align", "srk_ba_align_kernel_ms", "srk_ba_align_score_ms", "srk_align_check_sets",
    "srk_align_host_set", "srk_similarity_apply",
    "srk_homography_default_options", "srk_relate_homography", "srk_ba_homography_kernel_ms", "srk_ba_homography_score_ms",
    "srk_homography_check_pairs", "srk_homography_host_pair", "srk_homography_decompose",
    "srk_fundamental_default_options", "srk_relate_uncalibrated", "srk_ba_fundamental_kernel_ms", "srk_ba_fundamental_score_ms",
    "srk_ba_fundamental_solve_ms",
    "srk_fundamental_check_pairs", "srk_fundamental_host_pair",
    "srk_ba_phase_covariance", "srk_ba_covariances", "srk_ba_revert_covariances", "srk_ba_set_covariance_batch",
    "srk_ba_phase_cross_covariance", "srk_ba_cross_covariances", "srk_ba_revert_cross_covariances", "srk_ba_relative_pose_covariances",
    "srk_ba_normalize_scene", "srk_ba_revert_normalization", "srk_ba_check_world_is_normalized",
    "srk_ba_upload_scene", "srk_ba_optimize", "srk_ba_download_scene", "srk_ba_reset_scene", "srk_ba_phase_error",
    "srk_ba_phase_derivatives", "srk_ba_phase_schur", "srk_ba_phase_solve", "srk_ba_phase_backsub",
    "srk_ba_phase_accept", "srk_ba_buffer_size", "srk_ba_download", "srk_ba_download_rcs_rows", "srk_ba_set_profile", "srk_ba_dense_spd_solve",
    "srk_ba_set_covisibility", "srk_ba_set_rcs_mode", "srk_ba_rcs_fill", "srk_ba_solve_mfma_flops", "srk_ba_rcs_chunks",
    "srk_scene_num_observations", "srk_scene_generate", "srk_circle_camera_shots",
    "srk_read_matrix_file", "srk_decompose_proj_mat", "srk_triangulate_least_squares", "srk_dino_load",
]


def lib():
    """Load libsrk_ba.so; raises LibraryNotBuilt (never falls back to anything else)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: torch bundles its own libamdhip64.so.7 (same SONAME as /opt/rocm's).  Whichever is
    # loaded first serves both, and torch refuses to see the GPU when it is not its own.  Importing torch first makes
    # device pointers of this library usable by torch.distributed / RCCL (surikatoko_amd/dist.py).  Pure C/C++ users
    # of libsrk_ba.so never load torch and run on the ROCm runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(_PATH):
        raise LibraryNotBuilt(
            f"{_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or make -C surikatoko_amd/csrc).  There is no CPU fallback.")
    L = C.CDLL(_PATH)
    L.srk_ba_create.restype = C.c_void_p
    L.srk_ba_create.argtypes = [C.c_int]
    L.srk_ba_destroy.argtypes = [C.c_void_p]
    L.srk_ba_destroy.restype = None
    L.srk_ba_last_error.restype = C.c_char_p
    L.srk_ba_last_error.argtypes = [C.c_void_p]
    L.srk_ba_status_string.restype = C.c_char_p
    L.srk_ba_status_string.argtypes = [C.c_int]
    L.srk_ba_reproj_error.restype = C.c_double
    L.srk_ba_reproj_error_mvf.restype = C.c_int
    L.srk_ba_buffer_size.restype = C.c_int64
    L.srk_ba_buffer_size.argtypes = [C.c_void_p, C.c_int]
    L.srk_scene_num_observations.restype = C.c_int64
    L.srk_ba_rcs_fill.restype = C.c_double
    L.srk_ba_rcs_fill.argtypes = [C.c_void_p]
    L.srk_ba_solve_mfma_flops.restype = C.c_double
    L.srk_ba_solve_mfma_flops.argtypes = [C.c_void_p]
    L.srk_ba_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    L.srk_ba_set_allreduce.argtypes = [C.c_void_p, ALLREDUCE_FN, C.c_void_p, C.c_int, C.c_int]
    L.srk_ba_set_robust_loss.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.srk_ba_robust_loss.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_double)]
    L.srk_ba_observation_weights.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    L.srk_ba_set_observation_information.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    L.srk_ba_observation_information.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    L.srk_ba_observation_residuals.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int64]
    L.srk_ba_set_intrinsic_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    L.srk_ba_intrinsic_groups.argtypes = [C.c_void_p]
    L.srk_ba_download_intrinsics.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32]
    L.srk_ba_set_constant_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_int]
    L.srk_ba_constant_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.srk_ba_constant_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.srk_ba_constant_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.srk_ba_set_position_priors.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_int]
    L.srk_ba_position_prior_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
    L.srk_ba_position_priors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(C.c_int)]
    L.srk_ba_prior_error.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.srk_ba_prior_residuals.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_normalize_position_priors.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_prior_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.srk_ba_set_relative_pose_factors.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_check_relative_pose_factors.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_char_p)]
    L.srk_ba_relative_pose_factor_count.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
    L.srk_ba_relative_pose_factors.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_relative_pose_error.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.srk_ba_relative_pose_residuals.argtypes = [C.c_void_p, C.c_void_p]
    L.srk_ba_normalize_relative_pose_factors.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_relative_pose_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    L.srk_ba_set_joint_pose_priors.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_int]
    L.srk_ba_check_joint_pose_priors.argtypes = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int, C.POINTER(C.c_char_p)]
    L.srk_ba_joint_pose_prior_counts.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.srk_ba_joint_pose_priors.argtypes = [C.c_void_p] * 7 + [C.POINTER(C.c_int)]
    L.srk_ba_joint_pose_prior_error.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    L.srk_ba_joint_pose_prior_residuals.argtypes = [C.c_void_p, C.c_void_p]
    L.srk_ba_normalize_joint_pose_priors.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 9
    L.srk_ba_joint_pose_prior_pass_ms.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    _marg = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    L.srk_ba_marginalization_plan.argtypes = _marg + [C.POINTER(MargCounts)]
    L.srk_ba_phase_marginalization.argtypes = _marg + [C.POINTER(C.c_int32)] + [C.c_void_p] * 4 + [C.POINTER(MargReport)]
    L.srk_ba_marginalization_prior.argtypes = _marg + [C.POINTER(C.c_int32)] + [C.c_void_p] * 5 + [C.POINTER(MargReport)]
    L.srk_ba_marginalize_dense.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    L.srk_ba_revert_marginalization_prior.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 5
    _tracks = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_tri_default_options.argtypes = [C.POINTER(TriOptions)]
    L.srk_tri_default_options.restype = None
    L.srk_triangulate_tracks.argtypes = [C.c_void_p, C.c_double] + _tracks + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                              C.POINTER(TriOptions), C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_triangulate.argtypes = [C.c_void_p] + _tracks + [C.POINTER(TriOptions), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_tri_check_tracks.argtypes = _tracks + [C.c_int32, C.POINTER(TriOptions), C.POINTER(C.c_char_p)]
    L.srk_ba_triangulate_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_triangulate_kernel_ms.restype = C.c_double
    L.srk_tri_revert_points.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    _frames = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]   # n_frames, row_ptr, point, uv, q
    _poses = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(ResectOptions)]   # K, shared_k, R0, T0, options
    L.srk_resect_default_options.argtypes = [C.POINTER(ResectOptions)]
    L.srk_resect_default_options.restype = None
    L.srk_resect_frames.argtypes = [C.c_void_p, C.c_double] + _frames + [C.c_int64, C.c_void_p] + _poses + [C.c_void_p] * 6
    L.srk_ba_resect.argtypes = [C.c_void_p] + _frames + _poses + [C.c_int] + [C.c_void_p] * 6
    L.srk_resect_check_frames.argtypes = _frames + [C.c_int64, C.c_void_p] + _poses + [C.POINTER(C.c_char_p)]
    L.srk_ba_resect_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_resect_kernel_ms.restype = C.c_double
    L.srk_resect_revert.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    _hyp = [C.c_void_p, C.c_int, C.POINTER(LocateOptions), C.POINTER(ResectOptions)]   # K, shared_k, options, refine
    L.srk_locate_default_options.argtypes = [C.POINTER(LocateOptions)]
    L.srk_locate_default_options.restype = None
    L.srk_locate_frames.argtypes = [C.c_void_p, C.c_double] + _frames + [C.c_int64, C.c_void_p] + _hyp + [C.c_void_p] * 9
    L.srk_ba_locate.argtypes = [C.c_void_p] + _frames + _hyp + [C.c_int] + [C.c_void_p] * 9
    L.srk_locate_check_frames.argtypes = _frames + [C.c_int64, C.c_void_p] + _hyp + [C.POINTER(C.c_char_p)]
    L.srk_ba_locate_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_locate_kernel_ms.restype = C.c_double
    L.srk_ba_locate_score_ms.argtypes = [C.c_void_p]
    L.srk_ba_locate_score_ms.restype = C.c_double
    # n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, options
    _pairs = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.POINTER(RelateOptions)]
    L.srk_relate_default_options.argtypes = [C.POINTER(RelateOptions)]
    L.srk_relate_default_options.restype = None
    L.srk_relate_frames.argtypes = [C.c_void_p, C.c_double] + _pairs + [C.c_void_p] * 6
    L.srk_relate_check_pairs.argtypes = _pairs + [C.POINTER(C.c_char_p)]
    L.srk_relate_host_pair.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.POINTER(RelateOptions)] + [C.c_void_p] * 5
    L.srk_ba_relate_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_relate_kernel_ms.restype = C.c_double
    L.srk_ba_relate_score_ms.argtypes = [C.c_void_p]
    L.srk_ba_relate_score_ms.restype = C.c_double
    L.srk_pair_default_options.argtypes = [C.POINTER(PairOptions)]
    L.srk_pair_default_options.restype = None
    # ... the pairs without relate's options, then R0, T0, options
    _starts = _pairs[:-1] + [C.c_void_p, C.c_void_p, C.POINTER(PairOptions)]
    L.srk_refine_pairs.argtypes = [C.c_void_p, C.c_double] + _starts + [C.c_void_p] * 8
    L.srk_relate_frames_refined.argtypes = [C.c_void_p, C.c_double] + _pairs + [C.POINTER(PairOptions)] + [C.c_void_p] * 11
    L.srk_pair_check_pairs.argtypes = _starts + [C.POINTER(C.c_char_p)]
    L.srk_pair_host_pair.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.c_void_p, C.c_void_p, C.POINTER(PairOptions)] + [C.c_void_p] * 9 + [
        C.POINTER(C.c_int32)]
    L.srk_pair_factor.argtypes = [C.c_void_p] * 4 + [C.c_double] + [C.c_void_p] * 3
    L.srk_ba_pair_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_pair_kernel_ms.restype = C.c_double
    L.srk_align_default_options.argtypes = [C.POINTER(AlignOptions)]
    L.srk_align_default_options.restype = None
    L.srk_align_points.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(AlignOptions)] + [C.c_void_p] * 6
    L.srk_ba_align.argtypes = [C.c_void_p, C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(AlignOptions), C.c_int] + [C.c_void_p] * 6
    L.srk_align_check_sets.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64] + [C.c_void_p] * 3 + [C.POINTER(AlignOptions)] + [C.c_void_p] * 5 + [
        C.POINTER(C.c_char_p)]
    L.srk_align_host_set.argtypes = [C.c_int64] + [C.c_void_p] * 3 + [C.POINTER(AlignOptions)] + [C.c_void_p] * 5
    L.srk_similarity_apply.argtypes = [C.c_double, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.srk_ba_align_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_align_kernel_ms.restype = C.c_double
    L.srk_ba_align_score_ms.argtypes = [C.c_void_p]
    L.srk_ba_align_score_ms.restype = C.c_double
    # n_pairs, row_ptr, uv_a, uv_b, q, K_a, K_b, shared_k, options
    _hpairs = [C.c_int32] + [C.c_void_p] * 6 + [C.c_int, C.POINTER(HomographyOptions)]
    L.srk_homography_default_options.argtypes = [C.POINTER(HomographyOptions)]
    L.srk_homography_default_options.restype = None
    L.srk_relate_homography.argtypes = [C.c_void_p, C.c_double] + _hpairs + [C.c_void_p] * 10
    L.srk_homography_check_pairs.argtypes = _hpairs + [C.POINTER(C.c_char_p)]
    L.srk_homography_host_pair.argtypes = [C.c_int64] + [C.c_void_p] * 5 + [C.c_double, C.POINTER(HomographyOptions)] + [C.c_void_p] * 9
    L.srk_homography_decompose.argtypes = [C.c_void_p, C.c_int64] + [C.c_void_p] * 9
    L.srk_ba_homography_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_homography_kernel_ms.restype = C.c_double
    L.srk_ba_homography_score_ms.argtypes = [C.c_void_p]
    L.srk_ba_homography_score_ms.restype = C.c_double
    # n_pairs, row_ptr, uv_a, uv_b, q, options
    _fpairs = [C.c_int32] + [C.c_void_p] * 4 + [C.POINTER(FundamentalOptions)]
    L.srk_fundamental_default_options.argtypes = [C.POINTER(FundamentalOptions)]
    L.srk_fundamental_default_options.restype = None
    L.srk_relate_uncalibrated.argtypes = [C.c_void_p, C.c_double] + _fpairs + [C.c_void_p] * 8
    L.srk_fundamental_check_pairs.argtypes = _fpairs + [C.POINTER(C.c_char_p)]
    L.srk_fundamental_host_pair.argtypes = [C.c_int64] + [C.c_void_p] * 3 + [C.c_double, C.POINTER(FundamentalOptions)] + [C.c_void_p] * 7
    L.srk_ba_fundamental_kernel_ms.argtypes = [C.c_void_p]
    L.srk_ba_fundamental_kernel_ms.restype = C.c_double
    L.srk_ba_fundamental_score_ms.argtypes = [C.c_void_p]
    L.srk_ba_fundamental_score_ms.restype = C.c_double
    L.srk_ba_fundamental_solve_ms.argtypes = [C.c_void_p]
    L.srk_ba_fundamental_solve_ms.restype = C.c_double
    L.srk_ransac_hypotheses.argtypes = [C.c_int, C.c_double, C.c_double]
    L.srk_ransac_hypotheses.restype = C.c_int64
    L.srk_ba_phase_covariance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    L.srk_ba_covariances.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int]
    L.srk_ba_revert_covariances.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]
    L.srk_ba_set_covariance_batch.argtypes = [C.c_void_p, C.c_int64]
    _pairs = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p] * 3
    L.srk_ba_phase_cross_covariance.argtypes = [C.c_void_p] + _pairs
    L.srk_ba_cross_covariances.argtypes = [C.c_void_p, C.c_double] + _pairs + [C.c_int]
    L.srk_ba_revert_cross_covariances.argtypes = [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]
    L.srk_ba_relative_pose_covariances.argtypes = [C.c_void_p, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.srk_ba_revert_normalization.restype = None
    L.srk_circle_camera_shots.restype = None
    _lib = L
    return L
