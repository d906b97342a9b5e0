"""ctypes binding of the C ABI in include/phovo_hip.h (libphovo_hip.so, built by csrc/Makefile).

There is no fallback: if the library is missing it is built with hipcc, and if that fails, or if no
HIP device is present when an engine is created, the error is raised to the caller.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# The product library, always -- unless a tools/ entry point has opted in to a diagnostic build (tools/_variant.py sets
# PHOVO_TOOLS_LIBRARY_OPT_IN=tools before the package is imported and names the build in PHOVO_HIP_LIBRARY: csrc/Makefile
# `variant`).  PHOVO_HIP_LIBRARY alone is ignored, so nothing in the environment can swap the library under tests, bench.py
# or an application.
_OVERRIDE = os.environ.get("PHOVO_HIP_LIBRARY") if os.environ.get("PHOVO_TOOLS_LIBRARY_OPT_IN") == "tools" else None
_SO = _OVERRIDE or os.path.join(_HERE, "libphovo_hip.so")
_CSRC = os.path.join(_HERE, "csrc")
MAX_LEVELS = 16

ROLE_SOURCE, ROLE_TARGET, ROLE_BOTH = 1, 2, 3
PAIR_NONFINITE = 1
PAIR_WINDOW_FALLBACK = 2
PAIR_RANK_DEFICIENT = 4
# phovo_status
OK, E_INVALID_ARGUMENT, E_CONFIG, E_SHAPE, E_HIP, E_NOT_READY, E_IO, E_UNSUPPORTED = range(8)


class PhovoError(RuntimeError):
    def __init__(self, status, where, message):
        super().__init__(f"{where}: status {status} ({message})")
        self.status = status


class Config(C.Structure):
    _fields_ = [
        ("num_levels", C.c_int),
        ("blur_filter_size", C.c_int * MAX_LEVELS),
        ("image_gradients_scaling_factor", C.c_double * MAX_LEVELS),
        ("lambda_optimization_step", C.c_double * MAX_LEVELS),
        ("max_num_iterations", C.c_int * MAX_LEVELS),
        ("min_gradient_norm", C.c_double * MAX_LEVELS),
        ("visualize_iterations", C.c_int),
    ]


STORAGE_F64, STORAGE_F32, STORAGE_F16 = 0, 1, 2
SAMPLING_NEAREST_SCATTER, SAMPLING_BILINEAR = 0, 1


class Extensions(C.Structure):
    _fields_ = [
        ("plane_storage", C.c_int),
        ("sampling", C.c_int),
        ("jacobian_corrected", C.c_int),
        ("reserved", C.c_int),
        ("huber_delta", C.c_double * MAX_LEVELS),
    ]


class PairReport(C.Structure):
    _fields_ = [
        ("iterations", C.c_int * MAX_LEVELS),
        ("gradient_norm", C.c_double),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
        ("valid_pixels", C.c_int32 * MAX_LEVELS),
    ]


class PairSystem(C.Structure):
    """phovo_pair_system: the Gauss-Newton system of one pair at a given state on one level."""
    _fields_ = [
        ("information", C.c_double * 36),
        ("gradient", C.c_double * 6),
        ("cost", C.c_double),
        ("rows", C.c_int32),
        ("flags", C.c_uint32),
    ]


SYSTEM_MAX_DIM = 8


class SampledSystem(C.Structure):
    """phovo_sampled_system: the Gauss-Newton system of one pair under the sampled aligners (bilinear sampling: dim 6; the
    affine-illumination objective: dim 8) at a given state on one level; information has leading dimension 8."""
    _fields_ = [
        ("information", C.c_double * (SYSTEM_MAX_DIM * SYSTEM_MAX_DIM)),
        ("gradient", C.c_double * SYSTEM_MAX_DIM),
        ("cost", C.c_double),
        ("rows", C.c_int32),
        ("flags", C.c_uint32),
        ("dim", C.c_int32),
        ("reserved", C.c_int32),
    ]


FUSION_AUTO, FUSION_OFF, FUSION_SPLIT = 0, -1, -2
OBJECTIVE_PHOTOMETRIC, OBJECTIVE_BIOBJECTIVE, OBJECTIVE_TRUST_REGION = 0, 1, 2
OBJECTIVE_PHOTOMETRIC_AFFINE = 3
OBJECTIVE_PHOTOMETRIC_GEOMETRIC = 4
OBJECTIVE_INVERSE_COMPOSITIONAL = 5
OBJECTIVE_INVERSE_ROBUST = 6
OBJECTIVE_INVERSE_SEMIDENSE = 7
LAUNCH_KINDS = ("persistent", "fused", "slide", "slide_fallback", "wide", "bilinear", "biobjective", "trust_region",
                "affine", "geometric", "inverse", "inverse_robust", "inverse_prior", "inverse_robust_prior",
                "inverse_semidense")

# phovo_trust_region_level.termination
(TR_SKIPPED, TR_MAX_ITERATIONS, TR_GRADIENT, TR_FUNCTION, TR_PARAMETER, TR_MIN_RADIUS, TR_INVALID_STEP,
 TR_EVALUATION_FAILED) = range(8)
TR_TERMINATIONS = ("skipped", "max_iterations", "gradient", "function", "parameter", "min_radius", "invalid_step",
                   "evaluation_failed")
TR_OPTION_FIELDS = ("function_tolerance", "gradient_tolerance", "parameter_tolerance", "initial_trust_region_radius",
                    "max_trust_region_radius", "min_trust_region_radius", "min_relative_decrease")


class TrustRegionOptions(C.Structure):
    """phovo_trust_region_options: the trust-region objective's per-level solver options."""
    _fields_ = [(name, C.c_double * MAX_LEVELS) for name in TR_OPTION_FIELDS]


class TrustRegionLevel(C.Structure):
    _fields_ = [("steps", C.c_int32), ("accepted", C.c_int32), ("termination", C.c_int32), ("rows", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("final_radius", C.c_double),
                ("jacobi_scaling", C.c_double * 6)]


class TrustRegionReport(C.Structure):
    _fields_ = [("level", TrustRegionLevel * MAX_LEVELS)]


class GeometricOptions(C.Structure):
    """phovo_geometric_options: the photometric-geometric objective's per-level depth weight and residual gate."""
    _fields_ = [("depth_weight", C.c_double * MAX_LEVELS), ("max_depth_residual", C.c_double * MAX_LEVELS)]


class GeometricReport(C.Structure):
    """phovo_geometric_report: depth rows and the two costs of every level's last system."""
    _fields_ = [("depth_rows", C.c_int32 * MAX_LEVELS), ("photometric_cost", C.c_double * MAX_LEVELS),
                ("depth_cost", C.c_double * MAX_LEVELS)]


class RobustOptions(C.Structure):
    """phovo_robust_options: the robust inverse-compositional objective's delta = scale_factor * median |r|."""
    _fields_ = [("scale_factor", C.c_double)]


class RobustReport(C.Structure):
    """phovo_robust_report: the Huber threshold and the outlier rows of every level's last system."""
    _fields_ = [("delta", C.c_double * MAX_LEVELS), ("outliers", C.c_int32 * MAX_LEVELS)]


class SemiDenseOptions(C.Structure):
    """phovo_semidense_options: the semi-dense inverse-compositional objective's per-level gradient threshold tau_L."""
    _fields_ = [("min_pixel_gradient", C.c_double * MAX_LEVELS)]


class SemiDenseReport(C.Structure):
    """phovo_semidense_report: the selected pixels of every level."""
    _fields_ = [("selected", C.c_int32 * MAX_LEVELS)]


class PriorOptions(C.Structure):
    """phovo_prior_options: the pose prior's per-level scale s_L (H' = H + s_L Lambda)."""
    _fields_ = [("level_scale", C.c_double * MAX_LEVELS)]


class PriorReport(C.Structure):
    """phovo_prior_report: e = Log(T_p^-1 T) and e^T Lambda e at the pose the finest executed level ended on."""
    _fields_ = [("error", C.c_double * 6), ("prior_cost", C.c_double)]


class RobustSystem(C.Structure):
    """phovo_robust_system: the weighted twist-basis system of one pair under the robust inverse-compositional objective at a
    given state on one level, with the threshold it was built with, the three costs and the outlier count."""
    _fields_ = [
        ("information", C.c_double * 36),
        ("gradient", C.c_double * 6),
        ("cost", C.c_double),
        ("huber_cost", C.c_double),
        ("squared_cost", C.c_double),
        ("delta", C.c_double),
        ("median", C.c_double),
        ("rows", C.c_int32),
        ("outliers", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_int32),
    ]


GEOMETRIC_SYSTEM_LINE_CAPACITY = 1280


class GeometricSystem(C.Structure):
    """phovo_geometric_system: the Gauss-Newton system of one pair under the photometric-geometric objective at a given state
    on one level, the photometric and the depth block apart and their entry-by-entry sum."""
    _fields_ = [
        ("information", C.c_double * 36),
        ("gradient", C.c_double * 6),
        ("photometric_information", C.c_double * 36),
        ("photometric_gradient", C.c_double * 6),
        ("depth_information", C.c_double * 36),
        ("depth_gradient", C.c_double * 6),
        ("photometric_cost", C.c_double),
        ("depth_cost", C.c_double),
        ("rows", C.c_int32),
        ("depth_rows", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_int32),
    ]


class LaunchRecord(C.Structure):
    _fields_ = [
        ("level_first", C.c_int), ("level_last", C.c_int), ("kind", C.c_int),
        ("threads", C.c_int), ("lds_bytes", C.c_int), ("workgroups", C.c_int),
    ]


# phovo_device_image.format
IMAGE_U8_GRAY, IMAGE_U8_RGB, IMAGE_U8_BGR, IMAGE_F64, IMAGE_F32, IMAGE_F16, IMAGE_U16 = range(7)


class DeviceImage(C.Structure):
    """phovo_device_image: a batch of images in device memory, strides in bytes."""
    _fields_ = [
        ("data", C.c_void_p),
        ("row_stride_bytes", C.c_size_t),
        ("frame_stride_bytes", C.c_size_t),
        ("format", C.c_int),
        ("reserved", C.c_int),
    ]


class IngestRecord(C.Structure):
    """phovo_ingest_record: what the last upload_frames_device launched."""
    _fields_ = [("chunks", C.c_int), ("wide_launches", C.c_int), ("scalar_launches", C.c_int), ("reserved", C.c_int)]


# name -> (restype, argtypes); every symbol include/phovo_hip.h declares
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p
SYMBOLS = {
    "phovo_version": (C.c_char_p, []),
    "phovo_status_string": (C.c_char_p, [C.c_int]),
    "phovo_last_error": (C.c_char_p, []),
    "phovo_device_count": (C.c_int, []),
    "phovo_config_default": (C.c_int, [C.POINTER(Config)]),
    "phovo_config_read_file": (C.c_int, [C.c_char_p, C.POINTER(Config)]),
    "phovo_extensions_default": (C.c_int, [C.POINTER(Extensions)]),
    "phovo_extensions_read_file": (C.c_int, [C.c_char_p, C.POINTER(Extensions)]),
    "phovo_eigen_pose": (C.c_int, [_dp, _dp]),
    "phovo_state_from_pose": (C.c_int, [_dp, _dp]),
    "phovo_trajectory_chain": (C.c_int, [C.c_int, _vp, _dp, _vp]),
    "phovo_trajectory_format_pose": (C.c_int, [C.c_double, _dp, C.c_char_p, C.c_size_t]),
    "phovo_pair_system_format": (C.c_int, [C.c_double, C.POINTER(PairSystem), C.c_char_p, C.c_size_t]),
    "phovo_robust_system_format": (C.c_int, [C.c_double, C.POINTER(RobustSystem), C.c_char_p, C.c_size_t]),
    "phovo_sampled_system_format": (C.c_int, [C.c_double, C.POINTER(SampledSystem), C.c_char_p, C.c_size_t]),
    "phovo_geometric_system_format": (C.c_int, [C.c_double, C.POINTER(GeometricSystem), C.c_char_p, C.c_size_t]),
    "phovo_warp_image": (C.c_int, [C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_int, _dp, _dp, C.c_int,
                                   _vp, C.c_size_t]),
    "phovo_odometry_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "phovo_odometry_destroy": (C.c_int, [_vp]),
    "phovo_odometry_read_configuration_file": (C.c_int, [_vp, C.c_char_p]),
    "phovo_odometry_set_config": (C.c_int, [_vp, C.POINTER(Config)]),
    "phovo_odometry_set_extensions": (C.c_int, [_vp, C.POINTER(Extensions)]),
    "phovo_odometry_set_latency_forms": (C.c_int, [_vp, C.c_int]),
    "phovo_odometry_set_objective": (C.c_int, [_vp, C.c_int]),
    "phovo_odometry_set_min_depth": (C.c_int, [_vp, C.c_double]),
    "phovo_odometry_set_max_depth": (C.c_int, [_vp, C.c_double]),
    "phovo_odometry_set_intrinsic_matrix": (C.c_int, [_vp, _dp]),
    "phovo_odometry_set_source_frame": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_int]),
    "phovo_odometry_set_target_frame": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_int]),
    "phovo_odometry_set_initial_state_vector": (C.c_int, [_vp, _dp]),
    "phovo_odometry_optimize": (C.c_int, [_vp]),
    "phovo_odometry_get_optimal_state_vector": (C.c_int, [_vp, _dp]),
    "phovo_odometry_get_optimal_rigid_transformation_matrix": (C.c_int, [_vp, _dp]),
    "phovo_odometry_get_report": (C.c_int, [_vp, C.POINTER(PairReport)]),
    "phovo_odometry_last_optimize_ms": (C.c_int, [_vp, _dp]),
    "phovo_odometry_get_pair_system": (C.c_int, [_vp, C.POINTER(PairSystem)]),
    "phovo_odometry_get_sampled_system": (C.c_int, [_vp, C.POINTER(SampledSystem)]),
    "phovo_odometry_get_geometric_system": (C.c_int, [_vp, C.POINTER(GeometricSystem)]),
    "phovo_odometry_get_objective_system": (C.c_int, [_vp, C.POINTER(PairSystem)]),
    "phovo_odometry_get_inverse_system": (C.c_int, [_vp, C.POINTER(PairSystem)]),
    "phovo_odometry_get_robust_system": (C.c_int, [_vp, C.POINTER(RobustSystem)]),
    "phovo_engine_create": (C.c_int, [C.c_int, C.POINTER(_vp)]),
    "phovo_engine_destroy": (C.c_int, [_vp]),
    "phovo_engine_set_config": (C.c_int, [_vp, C.POINTER(Config)]),
    "phovo_engine_get_config": (C.c_int, [_vp, C.POINTER(Config)]),
    "phovo_engine_set_extensions": (C.c_int, [_vp, C.POINTER(Extensions)]),
    "phovo_engine_get_extensions": (C.c_int, [_vp, C.POINTER(Extensions)]),
    "phovo_engine_set_intrinsic_matrix": (C.c_int, [_vp, _dp]),
    "phovo_engine_set_depth_range": (C.c_int, [_vp, C.c_double, C.c_double]),
    "phovo_engine_set_build_all_levels": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_set_wide_policy": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_set_level_fusion": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_set_batch_invariant": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_set_latency_forms": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_set_slide_policy": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_level_uses_wide": (C.c_int, [_vp, C.c_int, C.c_int]),
    "phovo_engine_set_objective": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_get_objective": (C.c_int, [_vp, _vp]),
    "phovo_trust_region_read_file": (C.c_int, [C.c_char_p, C.POINTER(Config), C.POINTER(TrustRegionOptions)]),
    "phovo_trust_region_options_default": (C.c_int, [C.POINTER(TrustRegionOptions)]),
    "phovo_engine_set_trust_region_options": (C.c_int, [_vp, C.POINTER(TrustRegionOptions)]),
    "phovo_engine_get_trust_region_options": (C.c_int, [_vp, C.POINTER(TrustRegionOptions)]),
    "phovo_engine_fetch_trust_region_reports": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_odometry_set_trust_region_options": (C.c_int, [_vp, C.POINTER(TrustRegionOptions)]),
    "phovo_odometry_get_trust_region_options": (C.c_int, [_vp, C.POINTER(TrustRegionOptions)]),
    "phovo_odometry_get_trust_region_report": (C.c_int, [_vp, C.POINTER(TrustRegionReport)]),
    "phovo_engine_fetch_illumination": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_odometry_get_illumination": (C.c_int, [_vp, C.POINTER(C.c_double)]),
    "phovo_geometric_options_default": (C.c_int, [C.POINTER(GeometricOptions)]),
    "phovo_geometric_read_file": (C.c_int, [C.c_char_p, C.POINTER(GeometricOptions)]),
    "phovo_engine_set_geometric_options": (C.c_int, [_vp, C.POINTER(GeometricOptions)]),
    "phovo_engine_get_geometric_options": (C.c_int, [_vp, C.POINTER(GeometricOptions)]),
    "phovo_engine_fetch_geometric_reports": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_odometry_set_geometric_options": (C.c_int, [_vp, C.POINTER(GeometricOptions)]),
    "phovo_odometry_get_geometric_options": (C.c_int, [_vp, C.POINTER(GeometricOptions)]),
    "phovo_odometry_get_geometric_report": (C.c_int, [_vp, C.POINTER(GeometricReport)]),
    "phovo_robust_options_default": (C.c_int, [C.POINTER(RobustOptions)]),
    "phovo_engine_set_robust_options": (C.c_int, [_vp, C.POINTER(RobustOptions)]),
    "phovo_engine_get_robust_options": (C.c_int, [_vp, C.POINTER(RobustOptions)]),
    "phovo_engine_fetch_robust_reports": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_odometry_set_robust_options": (C.c_int, [_vp, C.POINTER(RobustOptions)]),
    "phovo_odometry_get_robust_options": (C.c_int, [_vp, C.POINTER(RobustOptions)]),
    "phovo_odometry_get_robust_report": (C.c_int, [_vp, C.POINTER(RobustReport)]),
    "phovo_semidense_options_default": (C.c_int, [C.POINTER(SemiDenseOptions)]),
    "phovo_semidense_read_file": (C.c_int, [C.c_char_p, C.POINTER(SemiDenseOptions)]),
    "phovo_engine_set_semidense_options": (C.c_int, [_vp, C.POINTER(SemiDenseOptions)]),
    "phovo_engine_get_semidense_options": (C.c_int, [_vp, C.POINTER(SemiDenseOptions)]),
    "phovo_engine_fetch_semidense_reports": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_odometry_set_semidense_options": (C.c_int, [_vp, C.POINTER(SemiDenseOptions)]),
    "phovo_odometry_get_semidense_options": (C.c_int, [_vp, C.POINTER(SemiDenseOptions)]),
    "phovo_odometry_get_semidense_report": (C.c_int, [_vp, C.POINTER(SemiDenseReport)]),
    "phovo_prior_options_default": (C.c_int, [C.POINTER(PriorOptions)]),
    "phovo_engine_set_prior_options": (C.c_int, [_vp, C.POINTER(PriorOptions)]),
    "phovo_engine_get_prior_options": (C.c_int, [_vp, C.POINTER(PriorOptions)]),
    "phovo_engine_fetch_prior_reports": (C.c_int, [_vp, C.c_int, _vp]),
    "phovo_engine_enqueue_align_prior": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, _vp, _vp]),
    "phovo_odometry_set_pose_prior": (C.c_int, [_vp, _dp, _dp]),
    "phovo_odometry_clear_pose_prior": (C.c_int, [_vp]),
    "phovo_odometry_set_prior_options": (C.c_int, [_vp, C.POINTER(PriorOptions)]),
    "phovo_odometry_get_prior_options": (C.c_int, [_vp, C.POINTER(PriorOptions)]),
    "phovo_odometry_get_prior_report": (C.c_int, [_vp, C.POINTER(PriorReport)]),
    "phovo_prior_report_format": (C.c_int, [C.c_double, C.POINTER(PriorReport), C.c_char_p, C.c_size_t]),
    "phovo_host_register": (C.c_int, [_vp, C.c_size_t]),
    "phovo_host_unregister": (C.c_int, [_vp]),
    "phovo_engine_reserve_frames": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int]),
    "phovo_engine_level_size": (C.c_int, [_vp, C.c_int, _ip, _ip]),
    "phovo_engine_level_is_stored": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_upload_frame": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t]),
    "phovo_engine_upload_frame_u16": (C.c_int, [_vp, C.c_int, C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_double]),
    "phovo_engine_upload_frames": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t]),
    "phovo_engine_upload_frames_u16": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _vp, C.c_size_t, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_double]),
    "phovo_engine_upload_frames_device": (C.c_int, [_vp, C.c_int, C.c_int, C.c_int, C.POINTER(DeviceImage),
                                                    C.POINTER(DeviceImage), C.c_double, _vp]),
    "phovo_engine_last_ingest": (C.c_int, [_vp, C.POINTER(IngestRecord)]),
    "phovo_odometry_set_source_frame_device": (C.c_int, [_vp, C.POINTER(DeviceImage), C.POINTER(DeviceImage), C.c_double,
                                                         C.c_int, C.c_int, _vp]),
    "phovo_odometry_set_target_frame_device": (C.c_int, [_vp, C.POINTER(DeviceImage), C.POINTER(DeviceImage), C.c_double,
                                                         C.c_int, C.c_int, _vp]),
    "phovo_engine_set_level_planes": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "phovo_engine_get_level_planes": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp]),
    "phovo_engine_get_level_depth_gradients": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "phovo_engine_get_level_depth_gain": (C.c_int, [_vp, C.c_int, C.c_int, _vp]),
    "phovo_engine_align_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, _vp, _vp]),
    "phovo_engine_enqueue_align": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp]),
    "phovo_engine_synchronize": (C.c_int, [_vp]),
    "phovo_engine_fetch_results": (C.c_int, [_vp, C.c_int, _vp, _vp]),
    "phovo_engine_results_device_ptr": (C.c_int, [_vp, C.POINTER(_vp)]),
    "phovo_engine_last_align_ms": (C.c_int, [_vp, _dp, _dp]),
    "phovo_engine_level_launch_info": (C.c_int, [_vp, C.c_int, _ip, _ip, _ip, _ip]),
    "phovo_engine_last_launches": (C.c_int, [_vp, _vp, C.c_int, _ip]),
    "phovo_engine_last_ticket": (C.c_int, [_vp]),
    "phovo_engine_wait": (C.c_int, [_vp, C.c_int]),
    "phovo_engine_fetch": (C.c_int, [_vp, C.c_int, C.c_int, _vp, _vp]),
    "phovo_engine_device_states": (C.c_int, [_vp, C.c_int, C.POINTER(_vp)]),
    "phovo_engine_align_ms": (C.c_int, [_vp, C.c_int, _dp, _dp]),
    "phovo_engine_evaluate_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, C.c_int, _vp]),
    "phovo_engine_evaluate_sampled_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, C.c_int, C.c_int, _vp]),
    "phovo_engine_evaluate_geometric_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, C.c_int, _vp]),
    "phovo_engine_evaluate_objective_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, C.c_int, _vp]),
    "phovo_engine_evaluate_inverse_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, C.c_int, _vp]),
    "phovo_engine_evaluate_robust_pairs": (C.c_int, [_vp, C.c_int, _ip, _ip, _vp, _vp, C.c_int, _vp]),
}


def library_path():
    return _SO


def source_sha256():
    """sha256 over the sources libphovo_hip.so is built from (csrc/*.hip, *.hpp, *.cpp, the Makefile, include/phovo_hip.h), in
    name order: the stamp a rocprofv3 summary under profiles/ carries (tools/profile_round.sh) and bench.py compares with the
    tree it runs from.  (The library file itself is not reproducible bit for bit across build directories.)"""
    import hashlib
    h = hashlib.sha256()
    files = [os.path.join(_CSRC, f) for f in sorted(os.listdir(_CSRC))
             if f.endswith((".hip", ".hpp", ".cpp")) or f == "Makefile"]
    files.append(os.path.join(os.path.dirname(_HERE), "include", "phovo_hip.h"))
    for f in files:
        h.update(os.path.basename(f).encode() + b"\0")
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(force=False):
    """Compile libphovo_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", _CSRC]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    if not os.path.exists(_SO):
        raise RuntimeError("libphovo_hip.so was not produced by csrc/Makefile")
    return _SO


_lib = None


def lib():
    """The loaded library.  Builds it if it is missing; raises if that is impossible."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        L = C.CDLL(_SO)
        for name, (res, args) in SYMBOLS.items():
            if _OVERRIDE and not hasattr(L, name):
                continue                     # a diagnostic / older build named explicitly (tools/ A-B runs): bind what it has
            fn = getattr(L, name)            # AttributeError if the ABI and the header diverge
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def hip_runtimes_mapped():
    """The distinct HIP runtime files (libamdhip64) mapped into this process.  More than one means that torch's wheel
    brought its own runtime AFTER this library had loaded the system's: the two do not share devices or pointers, and the
    device-memory entry points cannot work.  Import torch before the first use of this package and there is one."""
    paths = set()
    try:
        with open("/proc/self/maps") as f:
            for line in f:
                if "libamdhip64" in line:
                    paths.add(os.path.realpath(line.split(None, 5)[-1].strip()))
    except OSError:
        pass
    return sorted(paths)


def check(status, where):
    if status != 0:
        L = lib()
        msg = L.phovo_last_error().decode() or L.phovo_status_string(status).decode()
        raise PhovoError(status, where, msg)


def make_config(num_levels=None, blur=None, grad_scale=None, lam=None, max_iter=None,
                min_grad=None, visualize=0):
    """Constructor defaults (...Analytic.h:430-443) overridden per argument."""
    cfg = Config()
    check(lib().phovo_config_default(C.byref(cfg)), "phovo_config_default")
    if num_levels is not None:
        cfg.num_levels = int(num_levels)
    for name, vals in (("blur_filter_size", blur),
                       ("image_gradients_scaling_factor", grad_scale),
                       ("lambda_optimization_step", lam),
                       ("max_num_iterations", max_iter),
                       ("min_gradient_norm", min_grad)):
        if vals is not None:
            arr = getattr(cfg, name)
            for i, v in enumerate(list(vals)[:MAX_LEVELS]):
                arr[i] = v
    cfg.visualize_iterations = int(visualize)
    return cfg


def make_extensions(plane_storage=STORAGE_F64, huber_delta=None, sampling=SAMPLING_NEAREST_SCATTER,
                    jacobian_corrected=False):
    ext = Extensions()
    check(lib().phovo_extensions_default(C.byref(ext)), "phovo_extensions_default")
    ext.plane_storage = int(plane_storage)
    ext.sampling = int(sampling)
    ext.jacobian_corrected = int(bool(jacobian_corrected))
    if huber_delta is not None:
        for i, v in enumerate(list(huber_delta)[:MAX_LEVELS]):
            ext.huber_delta[i] = float(v)
    return ext


def read_extensions_file(path):
    ext = Extensions()
    check(lib().phovo_extensions_read_file(os.fsencode(path), C.byref(ext)), "phovo_extensions_read_file")
    return ext


def state_from_pose(rt):
    """phovo_state_from_pose: (x, y, z, yaw, pitch, roll) of a 4x4 pose, the inverse of phovo_eigen_pose wherever
    cos(pitch) != 0 (host arithmetic only)."""
    m = np.ascontiguousarray(rt, dtype=np.float64).reshape(16)
    s = np.zeros(6)
    check(lib().phovo_state_from_pose(m.ctypes.data_as(_dp), s.ctypes.data_as(_dp)), "phovo_state_from_pose")
    return s


def read_config_file(path):
    cfg = Config()
    check(lib().phovo_config_read_file(os.fsencode(path), C.byref(cfg)), "phovo_config_read_file")
    return cfg


def format_pair_system(timestamp, system):
    """phovo_pair_system_format: the line the VisualOdometry app writes per pair with --information."""
    buf = C.create_string_buffer(1024)
    check(lib().phovo_pair_system_format(float(timestamp), C.byref(system), buf, len(buf)), "phovo_pair_system_format")
    return buf.value.decode()


def format_robust_system(timestamp, system):
    """phovo_robust_system_format: the line the VisualOdometry app writes per pair with --robust-system."""
    buf = C.create_string_buffer(1024)
    check(lib().phovo_robust_system_format(float(timestamp), C.byref(system), buf, len(buf)), "phovo_robust_system_format")
    return buf.value.decode()


def format_prior_report(timestamp, report):
    """phovo_prior_report_format: `timestamp prior_cost e0 .. e5`."""
    buf = C.create_string_buffer(256)
    check(lib().phovo_prior_report_format(float(timestamp), C.byref(report), buf, len(buf)), "phovo_prior_report_format")
    return buf.value.decode()


def format_sampled_system(timestamp, system):
    """phovo_sampled_system_format: the line the VisualOdometry app writes per pair with --system."""
    buf = C.create_string_buffer(1024)
    check(lib().phovo_sampled_system_format(float(timestamp), C.byref(system), buf, len(buf)),
          "phovo_sampled_system_format")
    return buf.value.decode()


def format_geometric_system(timestamp, system):
    """phovo_geometric_system_format: the line the VisualOdometry app writes per pair with --geometric-system."""
    buf = C.create_string_buffer(GEOMETRIC_SYSTEM_LINE_CAPACITY)
    check(lib().phovo_geometric_system_format(float(timestamp), C.byref(system), buf, len(buf)),
          "phovo_geometric_system_format")
    return buf.value.decode()


def trust_region_options_default():
    opt = TrustRegionOptions()
    check(lib().phovo_trust_region_options_default(C.byref(opt)), "phovo_trust_region_options_default")
    return opt


def make_trust_region_options(**per_level):
    """Ceres's defaults, with any of TR_OPTION_FIELDS given as a per-level list (or one value for every level)."""
    opt = trust_region_options_default()
    for name, vals in per_level.items():
        if name not in TR_OPTION_FIELDS:
            raise KeyError(name)
        arr = getattr(opt, name)
        vals = [vals] * MAX_LEVELS if np.isscalar(vals) else list(vals)
        for i, v in enumerate(vals[:MAX_LEVELS]):
            arr[i] = float(v)
    return opt


def read_trust_region_file(path):
    """phovo_trust_region_read_file: (Config, TrustRegionOptions) from a Ceres-method yml."""
    cfg, opt = Config(), TrustRegionOptions()
    check(lib().phovo_trust_region_read_file(str(path).encode(), C.byref(cfg), C.byref(opt)),
          "phovo_trust_region_read_file")
    return cfg, opt


def make_geometric_options(depth_weight=None, max_depth_residual=None):
    """phovo_geometric_options_default, with either field given as a per-level list (or one value for every level)."""
    opt = GeometricOptions()
    check(lib().phovo_geometric_options_default(C.byref(opt)), "phovo_geometric_options_default")
    for name, vals in (("depth_weight", depth_weight), ("max_depth_residual", max_depth_residual)):
        if vals is None:
            continue
        arr = getattr(opt, name)
        vals = [vals] * MAX_LEVELS if np.isscalar(vals) else list(vals)
        for i, v in enumerate(vals[:MAX_LEVELS]):
            arr[i] = float(v)
    return opt


def make_robust_options(scale_factor=None):
    """phovo_robust_options_default, or with the given scale_factor."""
    opt = RobustOptions()
    check(lib().phovo_robust_options_default(C.byref(opt)), "phovo_robust_options_default")
    if scale_factor is not None:
        opt.scale_factor = float(scale_factor)
    return opt


def make_semidense_options(min_pixel_gradient=None):
    """phovo_semidense_options_default (0 on every level), or with min_pixel_gradient as a per-level list (or one value for
    every level).  A value that is not finite and >= 0 is a ValueError here, before the library sees it."""
    opt = SemiDenseOptions()
    check(lib().phovo_semidense_options_default(C.byref(opt)), "phovo_semidense_options_default")
    if min_pixel_gradient is not None:
        vals = [min_pixel_gradient] * MAX_LEVELS if np.isscalar(min_pixel_gradient) else list(min_pixel_gradient)
        for i, v in enumerate(vals[:MAX_LEVELS]):
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"min_pixel_gradient[{i}] = {v!r}: must be finite and >= 0")
            opt.min_pixel_gradient[i] = float(v)
    return opt


def read_semidense_file(path):
    """phovo_semidense_read_file: SemiDenseOptions from the optional key of an analytic yml."""
    opt = SemiDenseOptions()
    check(lib().phovo_semidense_read_file(os.fsencode(path), C.byref(opt)), "phovo_semidense_read_file")
    return opt


def make_prior_options(level_scale=None):
    """phovo_prior_options_default (1 on every level), or with level_scale as a per-level list (or one value for every level)."""
    opt = PriorOptions()
    check(lib().phovo_prior_options_default(C.byref(opt)), "phovo_prior_options_default")
    if level_scale is not None:
        vals = [level_scale] * MAX_LEVELS if np.isscalar(level_scale) else list(level_scale)
        for i, v in enumerate(vals[:MAX_LEVELS]):
            opt.level_scale[i] = float(v)
    return opt


def read_geometric_file(path):
    """phovo_geometric_read_file: GeometricOptions from the two optional keys of an analytic yml."""
    opt = GeometricOptions()
    check(lib().phovo_geometric_read_file(os.fsencode(path), C.byref(opt)), "phovo_geometric_read_file")
    return opt
