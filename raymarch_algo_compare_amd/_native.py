"""ctypes binding of librm_hip.so (C ABI: include/rm_hip.h).

Fails loudly: a missing library or a missing GPU raises RmError -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# RM_HIP_LIB: a development build (csrc/Makefile DEV=1 -> librm_hip_dev.so, a few kernels only) for tools/; tests and the
# bench never set it
LIB_PATH = os.environ.get("RM_HIP_LIB") or os.path.join(_HERE, "librm_hip.so")

RM_NUM_SCENES = 20
RM_NUM_STRATEGIES = 11
RM_NUM_STRATEGY_KERNELS = 13      # + the two shader-only strategies (ids 11, 12; parity unpinned)
RM_HIST_BINS = 544
RM_MAX_TIMED = 256

ERROR_NAMES = {0: "RM_OK", -1: "RM_E_BAD_SCENE", -2: "RM_E_BAD_STRATEGY", -3: "RM_E_BAD_DIMS",
               -4: "RM_E_NO_DEVICE", -5: "RM_E_HIP", -6: "RM_E_BAD_ARG", -7: "RM_E_RCCL"}

EXPORTS = [
    "rm_init", "rm_shutdown", "rm_last_error", "rm_device_info", "rm_num_scenes", "rm_num_strategies",
    "rm_default_strategy_params",
    "rm_sdf_eval", "rm_march_rays", "rm_march_rays_team", "rm_render", "rm_render_outputs", "rm_render_device", "rm_stats_device_bytes",
    "rm_read_stats", "rm_bench_device", "rm_alloc_frame", "rm_free_frame", "rm_copy_frame_to_host",
    "rm_bench_store_path", "rm_render_batch", "rm_render_batch_outputs", "rm_set_pass_timing", "rm_get_pass_ms", "rm_last_queue_marks", "rm_long_ray_marks", "rm_set_queue_capacity",
    "rm_comm_unique_id", "rm_comm_init", "rm_comm_destroy", "rm_shard_rows", "rm_gather_frame", "rm_assemble_frame", "rm_gather_frame_root",
    "rm_runtime_info", "rm_stream_create", "rm_stream_synchronize", "rm_stream_destroy", "rm_debug_poison_queues",
    "rm_debug_set_trace", "rm_debug_get_trace", "rm_scene_program_create", "rm_scene_program_destroy", "rm_debug_math_eval",
    "rm_debug_bail4_eval",
    "rm_interval_supported", "rm_interval_sdf_eval", "rm_interval_march_rays", "rm_interval_render",
    "rm_segment_supported", "rm_segment_sdf_eval", "rm_segment_march_rays", "rm_segment_render",
    "rm_certify_supported", "rm_certify_march_rays", "rm_certify_render",
    "rm_affine_supported", "rm_affine_range_eval", "rm_affine_march_rays", "rm_affine_render",
    "rm_exact_supported", "rm_exact_march_rays", "rm_exact_render",
    "rm_ssim_scores", "rm_capture", "rm_shade_frames", "rm_score_captures",
    "rm_intrinsic_features", "rm_view_features",
    "rm_strategy_program_create", "rm_strategy_program_destroy",
]
RM_E_BAD_SCENE, RM_E_NO_DEVICE, RM_E_BAD_ARG = -1, -4, -6
RM_INTERVAL_MAX_STEPS = 200000   # RmIntervalConfig.max_steps ceiling
RM_SEGMENT_MAX_STEPS = 40960     # RmSegmentConfig.budget ceiling
RM_CERTIFY_MISS, RM_CERTIFY_HIT, RM_CERTIFY_OPEN = 0, 1, 2   # the `status` of the rm_certify_* calls
RM_RANGE_AFFINE, RM_RANGE_MEET = 1, 2   # the `mode` of the rm_affine_* calls
RM_SCENE_PROGRAM_BASE = 1024
RM_STRATEGY_PROGRAM_BASE = 1024
RM_E_BAD_STRATEGY = -2
# RmMathFn (include/rm_hip.h): the device math routines rm_debug_math_eval evaluates
MATH_FNS = {"POW": 0, "POW2": 1, "POW_HALF_DENSE": 2, "POW_HALF_SPARSE": 3, "POW_HALF_GUARD": 4, "SQRT": 5, "SIN": 6,
            "COS": 7, "SINCOS": 8, "SINCOS_U": 9, "ACOS": 10, "ACOS_U": 11, "ATAN2": 12, "ATAN2_U": 13, "LOG": 14}
MATH_TWO_ARGS = {"POW", "ATAN2", "ATAN2_U"}                          # read b
MATH_TWO_OUTS = {"POW2", "POW_HALF_GUARD", "SINCOS", "SINCOS_U"}     # write out1


class RmError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"{ERROR_NAMES.get(code, code)}: {message}")
        self.code = code


# RmStrategyParams (include/rm_hip.h): the reference strategies' constructor arguments (relaxed_sphere.py:17,
# auto_relaxed.py:21-23, slope_auto_relaxed.py:25, overstep_bisect.py:18, adaptive_hybrid.py:17-19) and four
# literals of their march() bodies; (field, ctype, the reference's default).
STRATEGY_PARAM_FIELDS = [
    ("omega", ctypes.c_double, 1.2), ("ar_omega_min", ctypes.c_double, 1.0), ("ar_omega_max", ctypes.c_double, 2.0),
    ("ar_smoothing", ctypes.c_double, 0.7), ("ar_growth_rate", ctypes.c_double, 1.05),
    ("ar_decay_rate", ctypes.c_double, 0.7), ("beta", ctypes.c_double, 0.3),
    ("overstep_min_step", ctypes.c_double, 0.01), ("hybrid_stuck_step_ratio", ctypes.c_double, 0.001),
    ("hybrid_min_step", ctypes.c_double, 0.005), ("margin", ctypes.c_double, 0.05),
    ("ar_omega_init", ctypes.c_double, 1.2),
    ("overstep_bisection_steps", ctypes.c_int32, 16), ("hybrid_stuck_threshold", ctypes.c_int32, 5),
    ("segment_bisection_steps", ctypes.c_int32, 8), ("revaa_bisection_steps", ctypes.c_int32, 8),
    # uniforms only the reference's fragment shader has (strategies.glsl:24,47,570); the defaults change no bit
    ("step_scale", ctypes.c_double, 1.0), ("dense_min_step", ctypes.c_double, 1e-4),
]
DEFAULT_STRATEGY_PARAMS = {n: d for n, _, d in STRATEGY_PARAM_FIELDS}


class RmStrategyParams(ctypes.Structure):
    _fields_ = [(n, t) for n, t, _ in STRATEGY_PARAM_FIELDS]


class RmMarchConfig(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int32), ("full", ctypes.c_int32),
                ("hit_threshold", ctypes.c_double), ("max_distance", ctypes.c_double),
                ("lipschitz", ctypes.c_double), ("use_params", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("params", RmStrategyParams)]


def fill_params(cfg: RmMarchConfig, params: dict | None) -> None:
    """Set cfg.params from a dict of RmStrategyParams overrides ({} / None: the reference's defaults)."""
    if not params:
        cfg.use_params = 0
        return
    vals = dict(DEFAULT_STRATEGY_PARAMS)
    for k, v in params.items():
        if k not in vals:
            raise KeyError(f"unknown strategy parameter {k!r} (RmStrategyParams has {sorted(vals)})")
        vals[k] = v
    for n, t, _ in STRATEGY_PARAM_FIELDS:
        setattr(cfg.params, n, int(vals[n]) if t is ctypes.c_int32 else float(vals[n]))
    cfg.use_params = 1


def march_config(max_iterations=512, full=False, hit_threshold=1e-4, max_distance=100.0, lipschitz=1.0,
                 params: dict | None = None) -> RmMarchConfig:
    c = RmMarchConfig()
    c.max_iterations, c.full = int(max_iterations), 1 if full else 0
    c.hit_threshold, c.max_distance, c.lipschitz = float(hit_threshold), float(max_distance), float(lipschitz)
    fill_params(c, params)
    return c


class RmFrameDesc(ctypes.Structure):
    _fields_ = [("scene_id", ctypes.c_int32), ("strategy_id", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("row0", ctypes.c_int32), ("rows", ctypes.c_int32),
                ("cam", ctypes.c_double * 14), ("march", RmMarchConfig),
                ("tile_rows", ctypes.c_int32), ("refill_min", ctypes.c_int32),
                ("grid_waves", ctypes.c_int32), ("band_rows", ctypes.c_int32),
                ("band_stride", ctypes.c_int32), ("band_offset", ctypes.c_int32),
                ("tile_order_mode", ctypes.c_int32), ("eval_mode", ctypes.c_int32),
                ("suspend_after", ctypes.c_int32 * 2),
                ("resume_grid", ctypes.c_int32), ("resume_mode", ctypes.c_int32),
                ("pipeline", ctypes.c_int32), ("team_grid", ctypes.c_int32), ("queue_first", ctypes.c_int32),
                ("team_steal", ctypes.c_int32), ("queue_refill_min", ctypes.c_int32), ("queue_retry", ctypes.c_int32),
                ("team_retry", ctypes.c_int32), ("age_priority", ctypes.c_int32),
                ("late_teams", ctypes.c_int32), ("exit_backlog", ctypes.c_int32),
                ("keep_busy", ctypes.c_int32), ("early_handover", ctypes.c_int32),
                ("early_trips", ctypes.c_int32), ("pipeline_form", ctypes.c_int32)]


class RmOutputs(ctypes.Structure):
    _fields_ = [("depth", ctypes.c_void_p), ("iters", ctypes.c_void_p), ("hit", ctypes.c_void_p),
                ("t_raw", ctypes.c_void_p), ("final_sdf", ctypes.c_void_p), ("block_var", ctypes.c_void_p),
                ("evals", ctypes.c_void_p)]


class RmStats(ctypes.Structure):
    _fields_ = [("total_rays", ctypes.c_uint64), ("hit_count", ctypes.c_uint64),
                ("sum_iters", ctypes.c_uint64), ("iter_max", ctypes.c_int32), ("iter_min", ctypes.c_int32),
                ("iter_hist", ctypes.c_uint64 * RM_HIST_BINS), ("sum_evals", ctypes.c_uint64)]


class RmTiming(ctypes.Structure):
    _fields_ = [("warmup", ctypes.c_int32), ("repeats", ctypes.c_int32),
                ("ms_median", ctypes.c_float), ("ms_mean", ctypes.c_float),
                ("ms_min", ctypes.c_float), ("ms_max", ctypes.c_float),
                ("ms_each", ctypes.c_float * RM_MAX_TIMED)]


class RmSceneOp(ctypes.Structure):
    """One instruction of a scene program (include/rm_hip.h; built by scene_program.py)."""
    _fields_ = [("op", ctypes.c_int32), ("arg", ctypes.c_int32), ("f", ctypes.c_double * 8)]


class RmStrategyOp(ctypes.Structure):
    """One instruction or block marker of a strategy program (include/rm_hip.h; built by strategy_program.py)."""
    _fields_ = [("op", ctypes.c_int32), ("dst", ctypes.c_int32), ("a", ctypes.c_int32), ("b", ctypes.c_int32),
                ("c", ctypes.c_int32), ("reserved", ctypes.c_int32), ("k", ctypes.c_double)]


class RmIntervalConfig(ctypes.Structure):
    """The interval oracle's constants (include/rm_hip.h); every field 0 = the reference's value."""
    _fields_ = [("t_max", ctypes.c_double), ("tol", ctypes.c_double), ("h0", ctypes.c_double), ("growth", ctypes.c_double),
                ("h_max", ctypes.c_double), ("normal_eps", ctypes.c_double), ("bound_radius", ctypes.c_double),
                ("max_steps", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RmExactConfig(ctypes.Structure):
    """The exact first hit's constants (include/rm_hip.h): t_min 0 = 1e-6, t_max 0 = no limit."""
    _fields_ = [("t_min", ctypes.c_double), ("t_max", ctypes.c_double), ("reserved", ctypes.c_int32 * 2)]


class RmSegmentConfig(ctypes.Structure):
    """The sound segment tracer's constants (include/rm_hip.h); every field 0 = the reference's value."""
    _fields_ = [("t_max", ctypes.c_double), ("tol", ctypes.c_double), ("h0", ctypes.c_double), ("kappa", ctypes.c_double),
                ("h_min", ctypes.c_double), ("h_max", ctypes.c_double), ("k_min", ctypes.c_double), ("l_global", ctypes.c_double),
                ("bound_radius", ctypes.c_double), ("budget", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RmCertifyConfig(ctypes.Structure):
    """The certified first hit's constants (include/rm_hip.h); every field 0 = its default."""
    _fields_ = [("t_max", ctypes.c_double), ("tol", ctypes.c_double), ("h0", ctypes.c_double), ("growth", ctypes.c_double),
                ("h_max", ctypes.c_double), ("bound_radius", ctypes.c_double), ("width", ctypes.c_double),
                ("l_global", ctypes.c_double), ("k_min", ctypes.c_double), ("max_steps", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class RmCaptureMaps(ctypes.Structure):
    """The host maps of one capture (include/rm_hip.h): float32 depth / normal / color, uint8 hit; normal and color may be NULL."""
    _fields_ = [("depth", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("color", ctypes.c_void_p), ("hit", ctypes.c_void_p)]


class RmScoreMaps(ctypes.Structure):
    """The host maps of one capture as rm_score_captures reads them (include/rm_hip.h): depth and normal hold float64 when
    fp64 != 0, float32 otherwise; uint8 hit; normal may be NULL."""
    _fields_ = [("depth", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("hit", ctypes.c_void_p), ("fp64", ctypes.c_int32)]


class RmScoreResult(ctypes.Structure):
    """One method's counts, depth error and normal angle against the reference (include/rm_hip.h)."""
    _fields_ = [(k, ctypes.c_int64) for k in ("n_method_hit", "n_reference_hit", "n_co_hit", "n_union", "n_co_hit_core",
                                              "n_union_core", "n_nan_depth", "n_nan_angle")] + \
               [(k, ctypes.c_double) for k in ("depth_mae", "depth_rmse", "depth_signed", "depth_p95", "depth_med",
                                               "normal_mean_deg", "normal_p95_deg")]


class RmIntrinsicFeatures(ctypes.Structure):
    """One sample set's intrinsic features (include/rm_hip.h); slab_median is a length, not yet in box diagonals."""
    _fields_ = [("lipschitz_p99", ctypes.c_double), ("slab_median", ctypes.c_double), ("n_finite", ctypes.c_int64),
                ("n_slabs", ctypes.c_int64)]


class RmViewMaps(ctypes.Structure):
    """The host maps of one capture as rm_view_features reads them (include/rm_hip.h): float32 depth / normal / evals,
    uint8 hit; all required."""
    _fields_ = [("depth", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("evals", ctypes.c_void_p), ("hit", ctypes.c_void_p)]


class RmViewFeatures(ctypes.Structure):
    """One capture's view features (include/rm_hip.h)."""
    _fields_ = [(k, ctypes.c_int64) for k in ("n_hit", "n_grazing", "n_perimeter", "sum_evals")] + \
               [(k, ctypes.c_double) for k in ("hit_rate", "grazing_frac", "silhouette_cplx", "hardness_mean", "hardness_cv")] + \
               [("box_lo", ctypes.c_double * 3), ("box_hi", ctypes.c_double * 3)]


class RmCaptureOutputs(ctypes.Structure):
    """The host maps rm_capture writes (include/rm_hip.h): float32 geom / normal / depth / color / evals, uint8 hit; any but
    hit may be NULL."""
    _fields_ = [("geom", ctypes.c_void_p), ("normal", ctypes.c_void_p), ("depth", ctypes.c_void_p), ("color", ctypes.c_void_p),
                ("evals", ctypes.c_void_p), ("hit", ctypes.c_void_p)]


class RmDeviceInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 128), ("arch", ctypes.c_char * 64),
                ("device_id", ctypes.c_int32), ("compute_units", ctypes.c_int32),
                ("clock_mhz", ctypes.c_int32), ("wavefront_size", ctypes.c_int32),
                ("total_mem_bytes", ctypes.c_uint64)]


class RmRuntimeInfo(ctypes.Structure):
    _fields_ = [("hip_runtime_path", ctypes.c_char * 512), ("hip_runtime_version", ctypes.c_int32),
                ("hip_driver_version", ctypes.c_int32), ("hip_runtimes_loaded", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("other_runtime_path", ctypes.c_char * 512)]


_lib = None
_lock = threading.Lock()
_device = None


def load() -> ctypes.CDLL:
    """dlopen librm_hip.so and declare the prototypes (no GPU call is made)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RmError(-4, f"{LIB_PATH} is missing: build it with "
                              f"`make -C {os.path.join(_HERE, 'csrc')} -j8` (or __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        vp, dp = ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)
        L.rm_init.argtypes = [ctypes.c_int]
        L.rm_shutdown.restype = None
        L.rm_last_error.restype = ctypes.c_char_p
        L.rm_device_info.argtypes = [ctypes.POINTER(RmDeviceInfo)]
        L.rm_default_strategy_params.argtypes = [ctypes.POINTER(RmStrategyParams)]
        L.rm_default_strategy_params.restype = None
        L.rm_sdf_eval.argtypes = [ctypes.c_int, dp, ctypes.c_size_t, dp]
        L.rm_scene_program_create.argtypes = [ctypes.POINTER(RmSceneOp), ctypes.c_int32, ctypes.c_double,
                                              ctypes.POINTER(ctypes.c_int32)]
        L.rm_scene_program_destroy.argtypes = [ctypes.c_int32]
        L.rm_strategy_program_create.argtypes = [ctypes.POINTER(RmStrategyOp), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
        L.rm_strategy_program_destroy.argtypes = [ctypes.c_int32]
        L.rm_march_rays.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(RmMarchConfig), dp, dp,
                                    ctypes.c_size_t, vp, dp, vp, dp]
        L.rm_march_rays_team.argtypes = L.rm_march_rays.argtypes
        L.rm_render.argtypes = [ctypes.POINTER(RmFrameDesc), vp, vp, vp, vp, vp, vp,
                                ctypes.POINTER(RmStats), ctypes.POINTER(RmTiming)]
        L.rm_render_outputs.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmOutputs), ctypes.POINTER(RmStats),
                                        ctypes.POINTER(RmTiming)]
        L.rm_render_device.argtypes = [ctypes.POINTER(RmFrameDesc), vp, vp, vp, vp, vp]
        L.rm_stats_device_bytes.restype = ctypes.c_size_t
        L.rm_read_stats.argtypes = [vp, vp, ctypes.POINTER(RmStats)]
        L.rm_bench_device.argtypes = [ctypes.POINTER(RmFrameDesc), vp, vp, vp, ctypes.POINTER(RmStats),
                                      ctypes.POINTER(RmTiming)]
        L.rm_render_batch.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.c_int32, dp, ctypes.POINTER(RmMarchConfig),
                                      vp, vp, vp, ctypes.POINTER(RmStats), ctypes.POINTER(ctypes.c_float)]
        L.rm_render_batch_outputs.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.c_int32, dp, ctypes.POINTER(RmMarchConfig),
                                              ctypes.POINTER(RmOutputs), ctypes.POINTER(RmStats), ctypes.POINTER(ctypes.c_float)]
        L.rm_alloc_frame.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp), ctypes.POINTER(vp),
                                     ctypes.POINTER(vp)]
        L.rm_free_frame.argtypes = [vp, vp, vp]
        L.rm_copy_frame_to_host.argtypes = [ctypes.c_int32, ctypes.c_int32, vp, vp, vp, vp, vp, vp]
        L.rm_bench_store_path.argtypes = [ctypes.c_int32, ctypes.c_int32, vp, vp, vp, ctypes.POINTER(RmTiming)]
        L.rm_set_pass_timing.argtypes = [ctypes.c_int]
        L.rm_set_queue_capacity.argtypes = [ctypes.c_int64]
        L.rm_get_pass_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)]
        L.rm_last_queue_marks.argtypes = [ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_float)]
        L.rm_long_ray_marks.argtypes = [ctypes.POINTER(ctypes.c_float)]
        L.rm_comm_unique_id.argtypes = [ctypes.c_char_p]
        L.rm_comm_init.argtypes = [ctypes.c_char_p, ctypes.c_int32, ctypes.c_int32]
        L.rm_shard_rows.argtypes = [ctypes.c_int32, ctypes.c_int32]
        L.rm_gather_frame.argtypes = [ctypes.POINTER(RmFrameDesc), vp, vp, vp, vp, vp, vp, vp]
        L.rm_assemble_frame.argtypes = [ctypes.c_int32] * 6 + [vp, vp, vp]
        L.rm_gather_frame_root.argtypes = [ctypes.POINTER(RmFrameDesc), vp, vp, vp, vp, vp, vp, ctypes.c_int32, vp]
        L.rm_runtime_info.argtypes = [ctypes.POINTER(RmRuntimeInfo)]
        L.rm_stream_create.argtypes = [ctypes.POINTER(vp)]
        L.rm_stream_synchronize.argtypes = [vp]
        L.rm_stream_destroy.argtypes = [vp]
        L.rm_debug_poison_queues.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
        L.rm_debug_set_trace.argtypes = [ctypes.c_int]
        L.rm_debug_get_trace.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64), vp, vp, ctypes.c_int64,
                                         ctypes.POINTER(ctypes.c_uint32)]
        L.rm_debug_math_eval.argtypes = [ctypes.c_int32, dp, dp, ctypes.c_size_t, ctypes.c_uint64, dp, dp]
        L.rm_debug_bail4_eval.argtypes = [dp, ctypes.c_size_t, ctypes.c_uint64, ctypes.c_int32, dp, dp]
        L.rm_interval_supported.argtypes = [ctypes.c_int]
        L.rm_interval_sdf_eval.argtypes = [ctypes.c_int, dp, dp, ctypes.c_size_t, dp, dp]
        L.rm_interval_march_rays.argtypes = [ctypes.c_int, ctypes.POINTER(RmIntervalConfig), dp, dp, ctypes.c_size_t, dp, vp, vp]
        L.rm_interval_render.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmIntervalConfig), vp, vp, vp, vp,
                                         ctypes.POINTER(RmTiming)]
        L.rm_segment_supported.argtypes = [ctypes.c_int]
        L.rm_segment_sdf_eval.argtypes = [ctypes.c_int, dp, ctypes.c_size_t, dp]
        L.rm_segment_march_rays.argtypes = [ctypes.c_int, ctypes.POINTER(RmSegmentConfig), dp, dp, ctypes.c_size_t, dp, vp, vp]
        L.rm_segment_render.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmSegmentConfig), vp, vp, vp, vp,
                                        ctypes.POINTER(RmTiming)]
        L.rm_certify_supported.argtypes = [ctypes.c_int]
        L.rm_certify_march_rays.argtypes = [ctypes.c_int, ctypes.POINTER(RmCertifyConfig), dp, dp, ctypes.c_size_t, dp, dp, vp, vp]
        L.rm_certify_render.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmCertifyConfig), vp, vp, vp, vp,
                                        ctypes.POINTER(RmTiming)]
        L.rm_affine_supported.argtypes = [ctypes.c_int]
        L.rm_affine_range_eval.argtypes = [ctypes.c_int, ctypes.c_int, dp, ctypes.c_size_t, dp, vp]
        L.rm_affine_march_rays.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(RmIntervalConfig), dp, dp, ctypes.c_size_t, dp, vp]
        L.rm_affine_render.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.c_int, ctypes.POINTER(RmIntervalConfig), vp, vp, vp,
                                       ctypes.POINTER(RmTiming)]
        L.rm_exact_supported.argtypes = [ctypes.c_int]
        L.rm_exact_march_rays.argtypes = [ctypes.c_int, ctypes.POINTER(RmExactConfig), dp, dp, ctypes.c_size_t, dp, vp, vp]
        L.rm_exact_render.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmExactConfig), vp, vp, vp, vp,
                                      ctypes.POINTER(RmTiming)]
        L.rm_ssim_scores.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(RmCaptureMaps), ctypes.POINTER(RmCaptureMaps),
                                     ctypes.c_int32, dp, ctypes.POINTER(RmTiming)]
        L.rm_score_captures.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(RmScoreMaps),
                                        ctypes.POINTER(RmScoreMaps), ctypes.c_int32, ctypes.POINTER(RmScoreResult), ctypes.POINTER(RmTiming)]
        L.rm_capture.argtypes = [ctypes.POINTER(RmFrameDesc), ctypes.POINTER(RmCaptureOutputs), ctypes.POINTER(RmStats),
                                 ctypes.POINTER(RmTiming)]
        L.rm_shade_frames.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, dp, vp, vp, vp, vp, vp,
                                      ctypes.POINTER(RmTiming)]
        L.rm_intrinsic_features.argtypes = [ctypes.c_int, ctypes.c_int32, ctypes.c_int32, dp, ctypes.c_double, ctypes.c_int32, dp, dp,
                                            ctypes.c_int32, dp, ctypes.POINTER(RmIntrinsicFeatures), dp, vp, ctypes.POINTER(RmTiming)]
        L.rm_view_features.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, dp, ctypes.POINTER(RmViewMaps),
                                       ctypes.POINTER(RmViewFeatures), ctypes.POINTER(RmTiming)]
        for name in EXPORTS:
            if name not in ("rm_shutdown", "rm_last_error", "rm_stats_device_bytes", "rm_default_strategy_params"):
                getattr(L, name).restype = ctypes.c_int
        _lib = L
        return L


def check(rc: int) -> None:
    if rc != 0:
        raise RmError(rc, load().rm_last_error().decode("utf-8", "replace"))


def init(device_id: int | None = None) -> ctypes.CDLL:
    """Bind the library to a GPU (default: $LOCAL_RANK or 0).  Raises RmError without one."""
    global _device
    L = load()
    if device_id is None:
        device_id = _device if _device is not None else int(os.environ.get("LOCAL_RANK", "0"))
    if _device == device_id:
        return L
    if _device is not None:
        L.rm_shutdown()
        _device = None
    check(L.rm_init(int(device_id)))
    _device = device_id
    return L


def runtime_info() -> dict:
    """The HIP runtime librm_hip.so is bound to (no device needed): stream handles must come from this one."""
    L = load()
    info = RmRuntimeInfo()
    check(L.rm_runtime_info(ctypes.byref(info)))
    return {"hip_runtime_path": info.hip_runtime_path.decode(), "hip_runtime_version": int(info.hip_runtime_version),
            "hip_driver_version": int(info.hip_driver_version), "hip_runtimes_loaded": int(info.hip_runtimes_loaded),
            "other_runtime_path": info.other_runtime_path.decode()}


def device_info() -> dict:
    L = init()
    info = RmDeviceInfo()
    check(L.rm_device_info(ctypes.byref(info)))
    return {"name": info.name.decode(), "arch": info.arch.decode(), "device_id": info.device_id,
            "compute_units": info.compute_units, "clock_mhz": info.clock_mhz,
            "wavefront_size": info.wavefront_size, "total_mem_bytes": int(info.total_mem_bytes)}


def make_desc(scene_id, strategy_id, cam14, width, height, row0=0, rows=None, max_iterations=512,
              hit_threshold=1e-4, max_distance=100.0, lipschitz=1.0, full=False, tile_rows=0, refill_min=0,
              grid_waves=0, band_rows=0, band_stride=0, band_offset=0, tile_order_mode=0, eval_mode=0,
              suspend_after=(0, 0), resume_grid=0, resume_mode=0, params: dict | None = None, pipeline=0, team_grid=0,
              queue_first=0, team_steal=0, queue_refill_min=0, queue_retry=0, team_retry=0, age_priority=0, late_teams=0,
              exit_backlog=0, keep_busy=0, early_handover=0, early_trips=0, pipeline_form=0) -> RmFrameDesc:
    d = RmFrameDesc()
    d.scene_id, d.strategy_id = int(scene_id), int(strategy_id)
    d.width, d.height = int(width), int(height)
    d.row0 = int(row0)
    d.rows = int(height - row0 if rows is None else rows)
    cam14 = np.asarray(cam14, dtype=np.float64).ravel()
    if cam14.size != 14:
        raise ValueError("cam14 must hold 14 doubles")
    for i in range(14):
        d.cam[i] = float(cam14[i])
    d.march.max_iterations = int(max_iterations)
    d.march.full = 1 if full else 0
    d.march.hit_threshold = float(hit_threshold)
    d.march.max_distance = float(max_distance)
    d.march.lipschitz = float(lipschitz)
    fill_params(d.march, params)
    d.tile_rows, d.refill_min, d.grid_waves = int(tile_rows), int(refill_min), int(grid_waves)
    d.band_rows, d.band_stride, d.band_offset = int(band_rows), int(band_stride), int(band_offset)
    d.tile_order_mode = int(tile_order_mode)
    d.eval_mode = int(eval_mode)
    d.suspend_after[0], d.suspend_after[1] = int(suspend_after[0]), int(suspend_after[1])
    d.resume_grid = int(resume_grid)
    d.resume_mode = int(resume_mode)
    d.pipeline, d.team_grid, d.queue_first, d.team_steal = int(pipeline), int(team_grid), int(queue_first), int(team_steal)
    d.queue_refill_min, d.queue_retry, d.team_retry = int(queue_refill_min), int(queue_retry), int(team_retry)
    d.age_priority = int(age_priority)
    d.late_teams, d.exit_backlog = int(late_teams), int(exit_backlog)
    d.keep_busy = int(keep_busy)
    d.early_handover = int(early_handover)
    d.early_trips = int(early_trips)
    d.pipeline_form = int(pipeline_form)
    return d


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ref(record):
    """byref of an optional ctypes record (NULL for None)"""
    return ctypes.byref(record) if record is not None else None


def _timing(warmup, repeats):
    """RmTiming for repeats > 0, else None (an untimed call)"""
    if repeats <= 0:
        return None
    tm = RmTiming()
    tm.warmup, tm.repeats = int(warmup), int(repeats)
    return tm


def _rays(origins, dirs):
    """(origins, dirs) as contiguous (n, 3) float64 arrays of one shape"""
    origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    if origins.shape != dirs.shape:
        raise ValueError("origins and dirs differ in shape")
    return origins, dirs


def _frame_maps(d: RmFrameDesc, tm, **maps) -> dict:
    """the flat per-pixel outputs of a render of `d` as (rows, width[, 3]) arrays, with `timing` for a timed call"""
    shape = (int(d.rows), int(d.width))
    out = {k: a.reshape(shape + a.shape[1:]) for k, a in maps.items()}
    if tm is not None:
        out["timing"] = timing_dict(tm)
    return out


def timing_dict(t: RmTiming) -> dict:
    return {"warmup": t.warmup, "repeats": t.repeats, "ms_median": float(t.ms_median),
            "ms_mean": float(t.ms_mean), "ms_min": float(t.ms_min), "ms_max": float(t.ms_max),
            "ms_each": [float(t.ms_each[i]) for i in range(t.repeats)]}


def stats_dict(s: RmStats) -> dict:
    return {"total_rays": int(s.total_rays), "hit_count": int(s.hit_count), "sum_iters": int(s.sum_iters),
            "iter_max": int(s.iter_max), "iter_min": int(s.iter_min), "sum_evals": int(s.sum_evals),
            "iter_hist": np.ctypeslib.as_array(s.iter_hist).astype(np.int64).copy()}


def render(desc: RmFrameDesc, want_t_raw=False, want_final_sdf=False, want_block_var=False, warmup=0,
           repeats=0, want_evals=False) -> dict:
    """rm_render_outputs into fresh NumPy arrays.  Returns depth (f32), iters (i32), hit (u8), optional
    t_raw / final_sdf (f64) / block_var (i64) / evals (i32), stats (dict) and timing (dict or None)."""
    L = init()
    rows, W = desc.rows, desc.width
    out = {"depth": np.empty((rows, W), np.float32), "iters": np.empty((rows, W), np.int32),
           "hit": np.empty((rows, W), np.uint8), "t_raw": None, "final_sdf": None, "block_var": None, "evals": None}
    if want_evals:
        out["evals"] = np.empty((rows, W), np.int32)
    if want_t_raw:
        out["t_raw"] = np.empty((rows, W), np.float64)
    if want_final_sdf:
        out["final_sdf"] = np.empty((rows, W), np.float64)
    if want_block_var:
        out["block_var"] = np.empty((rows // 4, W // 8), np.int64)
    st = RmStats()
    tm = _timing(warmup, repeats)
    def addr(a):
        return None if a is None else a.ctypes.data
    o = RmOutputs(addr(out["depth"]), addr(out["iters"]), addr(out["hit"]), addr(out["t_raw"]), addr(out["final_sdf"]),
                  addr(out["block_var"]), addr(out["evals"]))
    check(L.rm_render_outputs(ctypes.byref(desc), ctypes.byref(o), ctypes.byref(st), _ref(tm)))
    out["stats"] = stats_dict(st)
    out["timing"] = timing_dict(tm) if tm is not None else None
    return out


def render_batch(shape: RmFrameDesc, cams, configs=None, want_evals=False) -> dict:
    """rm_render_batch_outputs: `cams` is (n, 14); `configs` an optional list of dicts / RmMarchConfig (one per
    frame).  Returns frame-major depth / iters / hit (/ evals) arrays (n, rows, W), per-frame stats and ms_total."""
    L = init()
    cams = np.ascontiguousarray(cams, dtype=np.float64).reshape(-1, 14)
    n = len(cams)
    rows, W = shape.rows, shape.width
    out = {"depth": np.empty((n, rows, W), np.float32), "iters": np.empty((n, rows, W), np.int32),
           "hit": np.empty((n, rows, W), np.uint8)}
    cfg_arr = None
    if configs is not None:
        if len(configs) != n:
            raise ValueError("one march config per frame")
        cfg_arr = (RmMarchConfig * n)()
        for i, c in enumerate(configs):
            if isinstance(c, RmMarchConfig):
                cfg_arr[i] = c
            else:
                cfg_arr[i] = march_config(c.get("max_iterations", 512), c.get("full"), c.get("hit_threshold", 1e-4),
                                          c.get("max_distance", 100.0), c.get("lipschitz", 1.0), c.get("params"))
    st = (RmStats * n)()
    ms = ctypes.c_float(0.0)
    out["evals"] = np.empty((n, rows, W), np.int32) if want_evals else None
    o = RmOutputs(out["depth"].ctypes.data, out["iters"].ctypes.data, out["hit"].ctypes.data, None, None, None,
                  out["evals"].ctypes.data if want_evals else None)
    check(L.rm_render_batch_outputs(ctypes.byref(shape), n, cams.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), cfg_arr,
                                    ctypes.byref(o), st, ctypes.byref(ms)))
    out["stats"] = [stats_dict(st[i]) for i in range(n)]
    out["ms_total"] = float(ms.value)
    return out


def scene_program_create(ops, nops: int, lipschitz: float = 1.0) -> int:
    """rm_scene_program_create: validate and register a program (RmSceneOp array); its scene id.  Needs no GPU."""
    L = load()
    sid = ctypes.c_int32(-1)
    check(L.rm_scene_program_create(ops, int(nops), float(lipschitz), ctypes.byref(sid)))
    return int(sid.value)


def scene_program_destroy(scene_id: int) -> None:
    check(load().rm_scene_program_destroy(int(scene_id)))


def strategy_program_create(ops, nops: int) -> int:
    """rm_strategy_program_create: validate and register a step program (RmStrategyOp array); its strategy id.  Needs no GPU."""
    L = load()
    sid = ctypes.c_int32(-1)
    check(L.rm_strategy_program_create(ops, int(nops), ctypes.byref(sid)))
    return int(sid.value)


def strategy_program_destroy(strategy_id: int) -> None:
    check(load().rm_strategy_program_destroy(int(strategy_id)))


def sdf_eval(scene_id: int, pts) -> np.ndarray:
    L = init()
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(pts), np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_sdf_eval(int(scene_id), pts.ctypes.data_as(dp), len(pts), out.ctypes.data_as(dp)))
    return out


def march_rays(scene_id, strategy_id, origins, dirs, max_iterations=512, hit_threshold=1e-4, max_distance=100.0,
               lipschitz=1.0, team=False, params: dict | None = None):
    L = init()
    origins = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = len(origins)
    cfg = march_config(max_iterations, True, hit_threshold, max_distance, lipschitz, params)
    hit, t = np.empty(n, np.uint8), np.empty(n, np.float64)
    iters, fs = np.empty(n, np.int32), np.empty(n, np.float64)
    dp = ctypes.POINTER(ctypes.c_double)
    fn = L.rm_march_rays_team if team else L.rm_march_rays
    check(fn(int(scene_id), int(strategy_id), ctypes.byref(cfg), origins.ctypes.data_as(dp),
             dirs.ctypes.data_as(dp), n, _ptr(hit), t.ctypes.data_as(dp), _ptr(iters), fs.ctypes.data_as(dp)))
    return hit, t, iters, fs


def debug_math_eval(fn, a, b=None, lane_mask=(1 << 64) - 1):
    """rm_debug_math_eval: the device math routine `fn` (a MATH_FNS name or id) on every element of `a` (and `b`), one
    element per live lane of `lane_mask`.  Returns (out0, out1); out1 is None for routines with one result."""
    L = init()
    name = fn if isinstance(fn, str) else {v: k for k, v in MATH_FNS.items()}.get(int(fn))
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1)
    if b is not None:
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        if len(b) != len(a):
            raise ValueError("a and b differ in length")
    out0 = np.empty_like(a)
    out1 = np.empty_like(a) if name in MATH_TWO_OUTS else None
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda x: None if x is None else x.ctypes.data_as(dp)      # noqa: E731
    check(L.rm_debug_math_eval(MATH_FNS[name] if name in MATH_FNS else int(fn), ptr(a), ptr(b), len(a),
                               int(lane_mask), ptr(out0), ptr(out1)))
    return out0, out1


def debug_bail4_eval(s, sparse, lane_mask=(1 << 64) - 1):
    """rm_debug_bail4_eval: the Mandelbulb's bail-out decision from the squared length (csrc/rm_math_pow.h rm_bail4) on the
    device, one element per live lane of `lane_mask`.  Returns (decision, band) as bool arrays."""
    L = init()
    s = np.ascontiguousarray(s, dtype=np.float64).reshape(-1)
    out0, out1 = np.empty_like(s), np.empty_like(s)
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_debug_bail4_eval(s.ctypes.data_as(dp), len(s), int(lane_mask), int(bool(sparse)), out0.ctypes.data_as(dp),
                                out1.ctypes.data_as(dp)))
    return out0 != 0.0, out1 != 0.0


def interval_config(t_max=0.0, tol=0.0, h0=0.0, growth=0.0, h_max=0.0, normal_eps=0.0, bound_radius=0.0,
                    max_steps=0) -> RmIntervalConfig:
    """RmIntervalConfig; 0 = the reference's constant (bound_radius 0: the library's bound for the scene, < 0: no prune)."""
    c = RmIntervalConfig()
    c.t_max, c.tol, c.h0, c.growth, c.h_max = float(t_max), float(tol), float(h0), float(growth), float(h_max)
    c.normal_eps, c.bound_radius, c.max_steps = float(normal_eps), float(bound_radius), int(max_steps)
    return c


def interval_supported(scene_id: int) -> bool:
    """rm_interval_supported (no GPU needed)."""
    return load().rm_interval_supported(int(scene_id)) == 1


def interval_sdf_eval(scene_id: int, lo, hi):
    """rm_interval_sdf_eval: the enclosure (lo, hi) of the scene's SDF over each box [lo, hi] (n x 3 corners)."""
    L = init()
    lo = np.ascontiguousarray(lo, dtype=np.float64).reshape(-1, 3)
    hi = np.ascontiguousarray(hi, dtype=np.float64).reshape(-1, 3)
    if lo.shape != hi.shape:
        raise ValueError("lo and hi differ in shape")
    out_lo, out_hi = np.empty(len(lo)), np.empty(len(lo))
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_interval_sdf_eval(int(scene_id), lo.ctypes.data_as(dp), hi.ctypes.data_as(dp), len(lo),
                                 out_lo.ctypes.data_as(dp), out_hi.ctypes.data_as(dp)))
    return out_lo, out_hi


def interval_march_rays(scene_id: int, origins, dirs, cfg: RmIntervalConfig | None = None, want_normals=True):
    """rm_interval_march_rays: (t (+inf on a miss), steps, normals or None) of n explicit rays."""
    L = init()
    origins, dirs = _rays(origins, dirs)
    n = len(dirs)
    t, steps = np.empty(n), np.empty(n, np.int32)
    normals = np.empty((n, 3)) if want_normals else None
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_interval_march_rays(int(scene_id), _ref(cfg), origins.ctypes.data_as(dp),
                                   dirs.ctypes.data_as(dp), n, t.ctypes.data_as(dp), _ptr(steps), _ptr(normals)))
    return t, steps, normals


def interval_render(scene_id: int, cam14, width: int, height: int, cfg: RmIntervalConfig | None = None, row0=0, rows=None,
                    warmup=0, repeats=0, want_normal=True) -> dict:
    """rm_interval_render: depth (0 on a miss), hit, normal (unless want_normal is False), steps of rows [row0, row0 + rows);
    `timing` with repeats > 0."""
    L = init()
    d = make_desc(scene_id, 0, cam14, width, height, row0, rows)
    n = int(width) * int(d.rows)
    depth, hit = np.empty(n), np.empty(n, np.uint8)
    normal, steps = np.empty((n, 3)) if want_normal else None, np.empty(n, np.int32)
    tm = _timing(warmup, repeats)
    check(L.rm_interval_render(ctypes.byref(d), _ref(cfg), _ptr(depth), _ptr(hit), _ptr(normal), _ptr(steps), _ref(tm)))
    maps = dict(depth=depth, hit=hit, normal=normal, steps=steps) if want_normal else dict(depth=depth, hit=hit, steps=steps)
    return _frame_maps(d, tm, **maps)


def exact_config(t_min=0.0, t_max=0.0) -> RmExactConfig:
    """RmExactConfig; t_min 0 = 1e-6, t_max 0 or inf = no limit."""
    c = RmExactConfig()
    c.t_min, c.t_max = float(t_min), 0.0 if t_max == float("inf") else float(t_max)
    return c


def exact_supported(scene_id: int) -> bool:
    """rm_exact_supported (no GPU needed); exact_refusal has the reason."""
    return load().rm_exact_supported(int(scene_id)) == 1


def exact_refusal(scene_id: int) -> str | None:
    """Why rm_exact_supported refuses the scene (rm_last_error's text); None when it does not."""
    L = load()
    if L.rm_exact_supported(int(scene_id)) == 1:
        return None
    return L.rm_last_error().decode("utf-8", "replace")


def exact_march_rays(scene_id: int, origins, dirs, cfg: RmExactConfig | None = None, want_normals=True):
    """rm_exact_march_rays: (t (+inf on a miss), normals or None, leaf (-1 on a miss)) of n explicit rays."""
    L = init()
    origins, dirs = _rays(origins, dirs)
    n = len(dirs)
    t, leaf = np.empty(n), np.empty(n, np.int32)
    normals = np.empty((n, 3)) if want_normals else None
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_exact_march_rays(int(scene_id), _ref(cfg), origins.ctypes.data_as(dp), dirs.ctypes.data_as(dp), n,
                                t.ctypes.data_as(dp), _ptr(normals), _ptr(leaf)))
    return t, normals, leaf


def exact_render(scene_id: int, cam14, width: int, height: int, cfg: RmExactConfig | None = None, row0=0, rows=None,
                 warmup=0, repeats=0) -> dict:
    """rm_exact_render: depth (0 on a miss), hit, normal, leaf of rows [row0, row0 + rows); `timing` with repeats > 0."""
    L = init()
    d = make_desc(scene_id, 0, cam14, width, height, row0, rows)
    n = int(width) * int(d.rows)
    depth, hit, normal, leaf = np.empty(n), np.empty(n, np.uint8), np.empty((n, 3)), np.empty(n, np.int32)
    tm = _timing(warmup, repeats)
    check(L.rm_exact_render(ctypes.byref(d), _ref(cfg), _ptr(depth), _ptr(hit), _ptr(normal), _ptr(leaf), _ref(tm)))
    return _frame_maps(d, tm, depth=depth, hit=hit, normal=normal, leaf=leaf)


def segment_config(t_max=0.0, tol=0.0, h0=0.0, kappa=0.0, h_min=0.0, h_max=0.0, k_min=0.0, l_global=0.0, bound_radius=0.0,
                   budget=0) -> RmSegmentConfig:
    """RmSegmentConfig; 0 = the reference's constant (bound_radius 0: the library's bound for the scene, < 0: no prune)."""
    c = RmSegmentConfig()
    c.t_max, c.tol, c.h0, c.kappa, c.h_min, c.h_max = float(t_max), float(tol), float(h0), float(kappa), float(h_min), float(h_max)
    c.k_min, c.l_global, c.bound_radius, c.budget = float(k_min), float(l_global), float(bound_radius), int(budget)
    return c


def segment_supported(scene_id: int) -> bool:
    """rm_segment_supported (no GPU needed)."""
    return load().rm_segment_supported(int(scene_id)) == 1


def segment_sdf_eval(scene_id: int, segs):
    """rm_segment_sdf_eval: (n, 4) val.lo, val.hi, der.lo, der.hi of the scene's SDF over each ray segment (n x 8: origin,
    direction, t0, t1)."""
    L = init()
    segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 8)
    out = np.empty((len(segs), 4))
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_segment_sdf_eval(int(scene_id), segs.ctypes.data_as(dp), len(segs), out.ctypes.data_as(dp)))
    return out


def segment_march_rays(scene_id: int, origins, dirs, cfg: RmSegmentConfig | None = None):
    """rm_segment_march_rays: (t (+inf on a miss), iters, cursor) of n explicit rays."""
    L = init()
    origins, dirs = _rays(origins, dirs)
    n = len(dirs)
    t, iters, cursor = np.empty(n), np.empty(n, np.int32), np.empty(n)
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_segment_march_rays(int(scene_id), _ref(cfg), origins.ctypes.data_as(dp),
                                  dirs.ctypes.data_as(dp), n, t.ctypes.data_as(dp), _ptr(iters), _ptr(cursor)))
    return t, iters, cursor


def segment_render(scene_id: int, cam14, width: int, height: int, cfg: RmSegmentConfig | None = None, row0=0, rows=None,
                   warmup=0, repeats=0) -> dict:
    """rm_segment_render: depth (0 on a miss), hit, iters, cursor of rows [row0, row0 + rows); `timing` with repeats > 0."""
    L = init()
    d = make_desc(scene_id, 0, cam14, width, height, row0, rows)
    n = int(width) * int(d.rows)
    depth, hit, iters, cursor = np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32), np.empty(n)
    tm = _timing(warmup, repeats)
    check(L.rm_segment_render(ctypes.byref(d), _ref(cfg), _ptr(depth), _ptr(hit), _ptr(iters), _ptr(cursor), _ref(tm)))
    return _frame_maps(d, tm, depth=depth, hit=hit, iters=iters, cursor=cursor)


def certify_config(t_max=0.0, tol=0.0, h0=0.0, growth=0.0, h_max=0.0, bound_radius=0.0, width=0.0, l_global=0.0, k_min=0.0,
                   max_steps=0) -> RmCertifyConfig:
    """RmCertifyConfig; 0 = the default (width 0: 1e-10 (1 + t_lo); bound_radius 0: the library's bound, < 0: no prune)."""
    c = RmCertifyConfig()
    c.t_max, c.tol, c.h0, c.growth, c.h_max = float(t_max), float(tol), float(h0), float(growth), float(h_max)
    c.bound_radius, c.width, c.l_global, c.k_min, c.max_steps = float(bound_radius), float(width), float(l_global), float(k_min), int(max_steps)
    return c


def certify_supported(scene_id: int) -> bool:
    """rm_certify_supported (no GPU needed)."""
    return load().rm_certify_supported(int(scene_id)) == 1


def certify_march_rays(scene_id: int, origins, dirs, cfg: RmCertifyConfig | None = None):
    """rm_certify_march_rays: (t_lo, t_hi, status (RM_CERTIFY_*), steps) of n explicit rays."""
    L = init()
    origins, dirs = _rays(origins, dirs)
    n = len(dirs)
    t_lo, t_hi, status, steps = np.empty(n), np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_certify_march_rays(int(scene_id), _ref(cfg), origins.ctypes.data_as(dp), dirs.ctypes.data_as(dp), n,
                                  t_lo.ctypes.data_as(dp), t_hi.ctypes.data_as(dp), _ptr(status), _ptr(steps)))
    return t_lo, t_hi, status, steps


def certify_render(scene_id: int, cam14, width: int, height: int, cfg: RmCertifyConfig | None = None, row0=0, rows=None,
                   warmup=0, repeats=0) -> dict:
    """rm_certify_render: t_lo, t_hi, status, steps of rows [row0, row0 + rows); `timing` with repeats > 0."""
    L = init()
    d = make_desc(scene_id, 0, cam14, width, height, row0, rows)
    n = int(width) * int(d.rows)
    t_lo, t_hi, status, steps = np.empty(n), np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32)
    tm = _timing(warmup, repeats)
    check(L.rm_certify_render(ctypes.byref(d), _ref(cfg), _ptr(t_lo), _ptr(t_hi), _ptr(status), _ptr(steps), _ref(tm)))
    return _frame_maps(d, tm, t_lo=t_lo, t_hi=t_hi, status=status, steps=steps)


def affine_supported(scene_id: int) -> bool:
    """rm_affine_supported (no GPU needed)."""
    return load().rm_affine_supported(int(scene_id)) == 1


def affine_range_eval(scene_id: int, segs, mode: int = RM_RANGE_AFFINE, want_form=None):
    """rm_affine_range_eval: ((n, 2) lo, hi; (n, 3) x0, x1, e or None) of the scene's SDF over each ray segment (n x 8:
    origin, direction, t0, t1).  The form is returned in RM_RANGE_AFFINE unless want_form is False."""
    L = init()
    segs = np.ascontiguousarray(segs, dtype=np.float64).reshape(-1, 8)
    if want_form is None:
        want_form = int(mode) == RM_RANGE_AFFINE
    rng = np.empty((len(segs), 2))
    form = np.empty((len(segs), 3)) if want_form else None
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_affine_range_eval(int(scene_id), int(mode), segs.ctypes.data_as(dp), len(segs), rng.ctypes.data_as(dp), _ptr(form)))
    return rng, form


def affine_march_rays(scene_id: int, origins, dirs, mode: int = RM_RANGE_AFFINE, cfg: RmIntervalConfig | None = None):
    """rm_affine_march_rays: (t (+inf on a miss), steps) of n explicit rays."""
    L = init()
    origins, dirs = _rays(origins, dirs)
    n = len(dirs)
    t, steps = np.empty(n), np.empty(n, np.int32)
    dp = ctypes.POINTER(ctypes.c_double)
    check(L.rm_affine_march_rays(int(scene_id), int(mode), _ref(cfg), origins.ctypes.data_as(dp), dirs.ctypes.data_as(dp), n,
                                 t.ctypes.data_as(dp), _ptr(steps)))
    return t, steps


def affine_render(scene_id: int, cam14, width: int, height: int, mode: int = RM_RANGE_AFFINE, cfg: RmIntervalConfig | None = None,
                  row0=0, rows=None, warmup=0, repeats=0) -> dict:
    """rm_affine_render: depth (0 on a miss), hit, steps of rows [row0, row0 + rows); `timing` with repeats > 0."""
    L = init()
    d = make_desc(scene_id, 0, cam14, width, height, row0, rows)
    n = int(width) * int(d.rows)
    depth, hit, steps = np.empty(n), np.empty(n, np.uint8), np.empty(n, np.int32)
    tm = _timing(warmup, repeats)
    check(L.rm_affine_render(ctypes.byref(d), int(mode), _ref(cfg), _ptr(depth), _ptr(hit), _ptr(steps), _ref(tm)))
    return _frame_maps(d, tm, depth=depth, hit=hit, steps=steps)


def capture_maps(capture: dict, width: int, height: int):
    """(RmCaptureMaps, the arrays it points into) of a capture dict: depth / normal / color as contiguous float32, hit
    (non-zero = hit) as uint8; a missing or None map is NULL."""
    shape = (int(height), int(width))
    keep = []

    def addr(key, tail=()):
        a = capture.get(key)
        if a is None:
            return None
        a = np.ascontiguousarray(np.asarray(a) != 0, np.uint8) if key == "hit" else np.ascontiguousarray(a, np.float32)
        if a.shape != shape + tail:
            raise ValueError(f"{key} has shape {a.shape}, not {shape + tail}")
        keep.append(a)
        return a.ctypes.data

    return RmCaptureMaps(addr("depth"), addr("normal", (3,)), addr("color", (3,)), addr("hit")), keep


def ssim_scores(width: int, height: int, reference: dict, methods, warmup=0, repeats=0):
    """rm_ssim_scores: the (n, 4) float64 array {depth_ssim, normal_ssim, color_ssim, color_rmse} of the capture dicts
    `methods` against `reference` (NaN where the captures carry no normal / color); with repeats > 0 also the kernels'
    timing dict."""
    L = init()
    n = len(methods)
    keep = []
    ref, k = capture_maps(reference, width, height)
    keep.append(k)
    marr = (RmCaptureMaps * max(n, 1))()
    for i, c in enumerate(methods):
        marr[i], k = capture_maps(c, width, height)
        keep.append(k)
    out = np.empty((n, 4), np.float64)
    tm = _timing(warmup, repeats)
    check(L.rm_ssim_scores(int(width), int(height), ctypes.byref(ref), marr, n, out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                           _ref(tm)))
    return (out, timing_dict(tm)) if tm is not None else out


def score_maps(capture: dict, width: int, height: int):
    """(RmScoreMaps, the arrays it points into) of a capture dict.  depth and normal stay float32 when both are (the
    flag fp64 = 0) and are float64 otherwise; a uint8 hit map is passed as it is (non-zero = hit), any other as `!= 0`; a
    missing or None normal is NULL."""
    shape = (int(height), int(width))
    depth, normal, hit = np.asarray(capture["depth"]), capture.get("normal"), np.asarray(capture["hit"])
    normal = None if normal is None else np.asarray(normal)
    single = depth.dtype == np.float32 and (normal is None or normal.dtype == np.float32)
    dtype = np.float32 if single else np.float64
    keep = [np.ascontiguousarray(depth, dtype), None if normal is None else np.ascontiguousarray(normal, dtype),
            np.ascontiguousarray(hit if hit.dtype == np.uint8 else hit != 0, np.uint8)]
    for a, key, tail in zip(keep, ("depth", "normal", "hit"), ((), (3,), ())):
        if a is not None and a.shape != shape + tail:
            raise ValueError(f"{key} has shape {a.shape}, not {shape + tail}")
    return RmScoreMaps(keep[0].ctypes.data, None if normal is None else keep[1].ctypes.data, keep[2].ctypes.data, int(not single)), keep


def score_captures(width: int, height: int, reference: dict, methods, band_k=2, warmup=0, repeats=0):
    """rm_score_captures: one dict of RmScoreResult's fields (int counts, float statistics) per capture dict of `methods`
    against `reference`; band_k < 0: no silhouette band.  With repeats > 0 also the kernels' timing dict."""
    L = init()
    n = len(methods)
    keep = []
    ref, k = score_maps(reference, width, height)
    keep.append(k)
    marr = (RmScoreMaps * max(n, 1))()
    for i, c in enumerate(methods):
        marr[i], k = score_maps(c, width, height)
        keep.append(k)
    res = (RmScoreResult * max(n, 1))()
    tm = _timing(warmup, repeats)
    check(L.rm_score_captures(int(width), int(height), int(band_k), ctypes.byref(ref), marr, n, res, _ref(tm)))
    out = [{name: getattr(res[i], name) for name, _ in RmScoreResult._fields_} for i in range(n)]
    return (out, timing_dict(tm)) if tm is not None else out


CAPTURE_MAPS = {"geom": (4,), "normal": (3,), "depth": (), "color": (3,), "evals": ()}


def capture(desc: RmFrameDesc, want=("geom", "normal", "depth", "color", "evals"), warmup=0, repeats=0) -> dict:
    """rm_capture into fresh NumPy arrays: the float32 maps named in `want` (CAPTURE_MAPS) of the rows of `desc`, hit (u8),
    stats (dict) and timing (dict or None).  `desc` must have been made with full=True."""
    L = init()
    shape = (int(desc.rows), int(desc.width))
    unknown = [k for k in want if k not in CAPTURE_MAPS]
    if unknown:
        raise ValueError(f"unknown capture maps {unknown}")
    out = {k: np.empty(shape + CAPTURE_MAPS[k], np.float32) for k in CAPTURE_MAPS if k in want}
    out["hit"] = np.empty(shape, np.uint8)
    o = RmCaptureOutputs(*[out[k].ctypes.data if k in out else None for k in ("geom", "normal", "depth", "color", "evals", "hit")])
    st = RmStats()
    tm = _timing(warmup, repeats)
    check(L.rm_capture(ctypes.byref(desc), ctypes.byref(o), ctypes.byref(st), _ref(tm)))
    out["stats"] = stats_dict(st)
    out["timing"] = timing_dict(tm) if tm is not None else None
    return out


def shade_frames(scene_id: int, cams, hit, t=None, depth=None, warmup=0, repeats=0) -> dict:
    """rm_shade_frames: normal and color (n, H, W, 3) float32 of the n frames `hit` (n, H, W; non-zero = hit) seen by the
    cameras `cams` (n, 14), from their fp64 ray parameters `t` or their fp32 `depth` (exactly one; (n, H, W)).  One frame
    may come without the leading axis; the result then has none either.  With repeats > 0 also `timing`."""
    L = init()
    hit = np.asarray(hit)
    single = hit.ndim == 2
    hit = np.ascontiguousarray((hit[None] if single else hit) != 0, np.uint8)
    if hit.ndim != 3:
        raise ValueError(f"hit has shape {hit.shape}, not (n, H, W)")
    n, H, W = hit.shape
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 14)
    if len(cams) != n:
        raise ValueError(f"{len(cams)} cameras for {n} frames")
    if (t is None) == (depth is None):
        raise ValueError("exactly one of t and depth must be given")
    src = np.ascontiguousarray(t, np.float64) if t is not None else np.ascontiguousarray(depth, np.float32)
    if src.size != hit.size:
        raise ValueError(f"{'t' if t is not None else 'depth'} has shape {src.shape}, hit {hit.shape}")
    normal, color = np.empty((n, H, W, 3), np.float32), np.empty((n, H, W, 3), np.float32)
    tm = _timing(warmup, repeats)
    check(L.rm_shade_frames(int(scene_id), W, H, n, cams.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                            _ptr(src) if t is not None else None, _ptr(src) if t is None else None, _ptr(hit), _ptr(normal),
                            _ptr(color), _ref(tm)))
    out = {"normal": normal[0] if single else normal, "color": color[0] if single else color}
    if tm is not None:
        out["timing"] = timing_dict(tm)
    return out


def intrinsic_features(scene_id: int, pts, eps: float, chords, seglen, ts, details=False, warmup=0, repeats=0):
    """rm_intrinsic_features: pts (nsets, n_lip, 3), chords (nsets, n_chords, 6), seglen (nsets, n_chords), ts (chord_steps)
    -> one dict of RmIntrinsicFeatures' fields per set; with `details` also gmag (n_lip; NaN = left out) and slab_counts
    (n_chords).  With repeats > 0 also the kernels' timing dict."""
    L = init()
    pts = np.ascontiguousarray(pts, np.float64)
    chords = np.ascontiguousarray(chords, np.float64)
    seglen = np.ascontiguousarray(seglen, np.float64)
    ts = np.ascontiguousarray(ts, np.float64).reshape(-1)
    if pts.ndim != 3 or pts.shape[2] != 3 or chords.ndim != 3 or chords.shape[2] != 6 or chords.shape[0] != pts.shape[0]:
        raise ValueError(f"pts {pts.shape} / chords {chords.shape}: want (nsets, n_lip, 3) and (nsets, n_chords, 6)")
    if seglen.shape != chords.shape[:2]:
        raise ValueError(f"seglen has shape {seglen.shape}, not {chords.shape[:2]}")
    nsets, n_lip, n_chords = pts.shape[0], pts.shape[1], chords.shape[1]
    res = (RmIntrinsicFeatures * max(nsets, 1))()
    gmag = np.empty((nsets, n_lip), np.float64) if details else None
    counts = np.empty((nsets, n_chords), np.int32) if details else None
    dp = ctypes.POINTER(ctypes.c_double)
    ptr = lambda a: None if a is None or a.size == 0 else a.ctypes.data_as(dp)      # noqa: E731
    tm = _timing(warmup, repeats)
    check(L.rm_intrinsic_features(int(scene_id), nsets, n_lip, ptr(pts), float(eps), n_chords, ptr(chords), ptr(seglen), len(ts),
                                  ptr(ts), res, ptr(gmag), None if counts is None or counts.size == 0 else _ptr(counts), _ref(tm)))
    out = [{name: getattr(res[i], name) for name, _ in RmIntrinsicFeatures._fields_} for i in range(nsets)]
    if details:
        for i, r in enumerate(out):
            r["gmag"], r["slab_counts"] = gmag[i], counts[i]
    return (out, timing_dict(tm)) if tm is not None else out


def view_maps(capture: dict, width: int, height: int):
    """(RmViewMaps, the arrays it points into) of a capture dict: depth / normal / evals as contiguous float32, hit (non-zero
    = hit) as uint8."""
    shape = (int(height), int(width))
    keep = [np.ascontiguousarray(capture["depth"], np.float32), np.ascontiguousarray(capture["normal"], np.float32),
            np.ascontiguousarray(capture["evals"], np.float32), np.ascontiguousarray(np.asarray(capture["hit"]) != 0, np.uint8)]
    for a, key, tail in zip(keep, ("depth", "normal", "evals", "hit"), ((), (3,), (), ())):
        if a.shape != shape + tail:
            raise ValueError(f"{key} has shape {a.shape}, not {shape + tail}")
    return RmViewMaps(*[a.ctypes.data for a in keep]), keep


def view_features(cams, captures, warmup=0, repeats=0):
    """rm_view_features: one dict of RmViewFeatures' fields (int counts, float features, box_lo / box_hi as (3,) arrays) per
    capture dict of `captures` (one frame size), seen by the cameras `cams` (n, 14).  With repeats > 0 also the timing dict."""
    L = init()
    n = len(captures)
    cams = np.ascontiguousarray(cams, np.float64).reshape(-1, 14)
    if len(cams) != n:
        raise ValueError(f"{len(cams)} cameras for {n} captures")
    if n == 0:
        return []
    height, width = np.asarray(captures[0]["hit"]).shape
    marr = (RmViewMaps * n)()
    keep = []
    for i, c in enumerate(captures):
        marr[i], k = view_maps(c, width, height)
        keep.append(k)
    res = (RmViewFeatures * n)()
    tm = _timing(warmup, repeats)
    check(L.rm_view_features(int(width), int(height), n, cams.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), marr, res, _ref(tm)))
    out = []
    for i in range(n):
        r = {name: getattr(res[i], name) for name, _ in RmViewFeatures._fields_[:9]}
        r["box_lo"], r["box_hi"] = np.array(res[i].box_lo[:]), np.array(res[i].box_hi[:])
        out.append(r)
    return (out, timing_dict(tm)) if tm is not None else out
