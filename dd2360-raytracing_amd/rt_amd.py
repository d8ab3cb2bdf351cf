"""ctypes binding of librt_amd.so (include/rt_amd.h) — the thin Python layer used by tests/, bench.py and
__graft_entry__.py.  The product is the C-ABI library and the C++ host program (host/main.cpp); this module only
marshals arguments.  Device memory, streams and process groups come from PyTorch (plumbing only).

There is no fallback of any kind: if librt_amd.so cannot be loaded, or a call returns non-zero, RtError is raised.
"""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RT_AMD_LIB", os.path.join(_HERE, "librt_amd.so"))   # RT_AMD_LIB: tuning experiments only

FP32, FP16 = 0, 1
MAT_NONE, MAT_LAMBERTIAN, MAT_METAL, MAT_DIELECTRIC = -1, 0, 1, 2
OCTREE_MAX_NODES = 585        # rt_amd.h RT_OCTREE_MAX_NODES
TRAVERSAL_REFERENCE, TRAVERSAL_FAST = 0, 1
BUILD_HOST, BUILD_DEVICE, BUILD_HOST_DECLINED = 0, 1, 2      # rt_amd.h RT_BUILD_*: what Octree.build_path() returns
ARITH_IEEE, ARITH_CONTRACT = 0, 1
IMAGE_P3, IMAGE_P6, IMAGE_PFM = 0, 1, 2

# PODs of include/rt_amd.h
rand_state_dtype = np.dtype([("d", "<u4"), ("v", "<u4", 5), ("boxmuller_flag", "<i4"), ("boxmuller_flag_double", "<i4"),
                             ("boxmuller_extra", "<f4"), ("pad_", "<u4"), ("boxmuller_extra_double", "<f8")])
sphere_dtype = np.dtype([("center", "<f4", 3), ("radius", "<f4"), ("material", "<i4"), ("albedo", "<f4", 3), ("param", "<f4")])
camera_dtype = np.dtype([("origin", "<f4", 3), ("lower_left_corner", "<f4", 3), ("horizontal", "<f4", 3), ("vertical", "<f4", 3),
                         ("u", "<f4", 3), ("v", "<f4", 3), ("w", "<f4", 3), ("lens_radius", "<f4")])
octnode_dtype = np.dtype([("level", "<i4"), ("aabb", "<f4", 6), ("children", "<i4", 8)])
hit_record_dtype = np.dtype([("t", "<f4"), ("p", "<f4", 3), ("normal", "<f4", 3), ("sphere", "<i4")])
assert rand_state_dtype.itemsize == 48 and sphere_dtype.itemsize == 36 and camera_dtype.itemsize == 88
assert octnode_dtype.itemsize == 60 and hit_record_dtype.itemsize == 32


class RtError(RuntimeError):
    pass


class Partition(C.Structure):
    """rt_partition: part `part` of `nparts`; tile_end > tile_begin: the tile range [tile_begin, tile_end) (a band of rt_split_balanced),
    otherwise runs of PART_RUN tiles dealt round-robin"""
    _fields_ = [("part", C.c_int32), ("nparts", C.c_int32), ("tile_begin", C.c_int64), ("tile_end", C.c_int64)]


WHOLE = Partition(0, 1)
PART_RUN = 64          # rt_amd.h RT_PART_RUN: consecutive tiles per run of the tile split (tests restate the split with it)
# rt_amd.h RT_SCHEDULE_WORDS: the words rt_render_ctx_schedule / rt_world_render_schedule copy, in this order
SCHEDULE_FIELDS = ("inflight_thr", "static_thr", "tail_mark", "head", "head_thr", "from_end", "long_raw", "solo_raw")
# rt_amd.h RT_FEEDBACK_WORDS: the words rt_render_ctx_schedule_feedback / rt_world_render_schedule_feedback copy, behind the rebuild count
FEEDBACK_FIELDS = ("has_counts", "rebuilt", "max_count", "solo_cap")

class Adaptive(C.Structure):
    """rt_adaptive: min_spp samples for every pixel, then `batch` more at a time for the pixels whose relative standard error of the
    mean luminance (the mean floored at `floor`) is still above rel_error, up to max_spp (include/rt_amd.h states the exact rule)"""
    _fields_ = [("min_spp", C.c_int32), ("max_spp", C.c_int32), ("batch", C.c_int32), ("rel_error", C.c_float), ("floor", C.c_float)]

ADAPTIVE_STATE_BYTES = 24      # rt_amd.h RT_ADAPTIVE_STATE_BYTES: the refinement state per buffer element (S_rgb, SL, Q, k)


class Budget(C.Structure):
    """rt_budget: `samples` to spend in `rounds` selections; a chosen pixel takes `batch` samples a round and is eligible while
    k + batch <= max_spp; floor as Adaptive.floor (include/rt_amd.h states the priority and the selection rule)"""
    _fields_ = [("samples", C.c_int64), ("rounds", C.c_int32), ("batch", C.c_int32), ("max_spp", C.c_int32), ("floor", C.c_float)]


class DenoiseParams(C.Structure):
    """rt_denoise_params: input mode (DENOISE_INPUT_*), the progressive sample count (SUM), levels (step 2^L at level L), the normal
    exponent's log2 (-1 = off) and the position / colour sigmas (0 = off); include/rt_amd.h states the exact filter"""
    _fields_ = [("input", C.c_int32), ("samples", C.c_int32), ("levels", C.c_int32), ("normal_pow_log2", C.c_int32),
                ("sigma_position", C.c_float), ("sigma_color", C.c_float)]

DENOISE_INPUT_GAMMA, DENOISE_INPUT_SUM = 0, 1      # rt_amd.h RT_DENOISE_INPUT_*
DENOISE_MAX_LEVELS = 8         # rt_amd.h RT_DENOISE_MAX_LEVELS
DENOISE_MAX_PIXELS = 1 << 30   # rt_amd.h RT_DENOISE_MAX_PIXELS: the largest frame of render_guides / denoise
DENOISE_WORK_BYTES = 32        # rt_amd.h RT_DENOISE_WORK_BYTES: the workspace per pixel (two float4 colour buffers)
# rt_amd.h RT_DENOISE_DEFAULT_*: chosen on C3 at 16 spp for the lowest RMSE against 1024 spp (tools/denoise_study.py)
DENOISE_DEFAULTS = dict(levels=2, normal_pow_log2=4, sigma_position=0.01, sigma_color=0.3)


def denoise_params(input=DENOISE_INPUT_GAMMA, samples=1, **kw):
    """a DenoiseParams with the library's defaults for whatever kw does not set"""
    return _params(DenoiseParams, DENOISE_DEFAULTS, kw, input, samples)


class DenoiseVarParams(C.Structure):
    """rt_denoise_var_params: levels, the normal exponent's log2 (-1 = off), prefilter (1 = the centre's variance is its 3x3 blur), the
    position sigma and the variance sigma in standard errors of the centre's mean luminance (0 = off); include/rt_amd.h states the rule"""
    _fields_ = [("levels", C.c_int32), ("normal_pow_log2", C.c_int32), ("prefilter", C.c_int32), ("sigma_position", C.c_float),
                ("sigma_variance", C.c_float)]

DENOISE_VAR_EPS = 1e-8         # rt_amd.h RT_DENOISE_VAR_EPS
# rt_amd.h RT_DENOISE_VAR_DEFAULT_*: one setting for C3 at 16, 64 and 128 spp (tools/denoise_variance_study.py)
DENOISE_VAR_DEFAULTS = dict(levels=1, normal_pow_log2=4, prefilter=1, sigma_position=0.01, sigma_variance=4.0)


def denoise_var_params(**kw):
    """a DenoiseVarParams with the library's defaults for whatever kw does not set"""
    return _params(DenoiseVarParams, DENOISE_VAR_DEFAULTS, kw)


class TemporalParams(C.Structure):
    """rt_temporal_params: the cap on the effective sample count taken over from the history (0 = take nothing), reuse_specular (0 = a
    first hit on metal or glass starts again), the relative position tolerance and the smallest normal dot product of an accepted history
    tap; include/rt_amd.h states the rule"""
    _fields_ = [("max_history", C.c_int32), ("reuse_specular", C.c_int32), ("position_tolerance", C.c_float), ("normal_min_dot", C.c_float)]

TEMPORAL_HISTORY_BYTES = 20    # rt_amd.h RT_TEMPORAL_HISTORY_BYTES: float4 (x.r, x.g, x.b, v) [n], then float neff [n]
# rt_amd.h RT_TEMPORAL_DEFAULT_*: DESIGN.md §5.10 "Temporal accumulation" (tools/temporal_study.py)
TEMPORAL_DEFAULTS = dict(max_history=32, reuse_specular=0, position_tolerance=0.03, normal_min_dot=0.9)


def temporal_params(**kw):
    """a TemporalParams with the library's defaults for whatever kw does not set"""
    return _params(TemporalParams, TEMPORAL_DEFAULTS, kw)


class TemporalRectify(C.Structure):
    """rt_temporal_rectify: the window radius (1..2), the smallest number of accepted window pixels at which the history is tested, and
    gamma, the allowed distance of the history from the window mean in standard deviations of the window (0 = off);
    include/rt_amd.h states the rule"""
    _fields_ = [("radius", C.c_int32), ("min_count", C.c_int32), ("gamma", C.c_float)]

# rt_amd.h RT_TEMPORAL_RECTIFY_DEFAULT_*: DESIGN.md §5.10 "History rectification" (profiles/r19/rectify.txt)
TEMPORAL_RECTIFY_DEFAULTS = dict(radius=1, min_count=4, gamma=1.5)


def temporal_rectify(**kw):
    """a TemporalRectify with the library's defaults for whatever kw does not set"""
    return _params(TemporalRectify, TEMPORAL_RECTIFY_DEFAULTS, kw)


class TemporalInputs(C.Structure):
    """rt_temporal_inputs: what temporal_accumulate takes besides the state and the world — the last frame's history (NULL: the first
    frame), this frame's guides, the last frame's guides and camera (a host pointer); build one with temporal_inputs()"""
    _fields_ = [("d_hist_in", C.c_void_p), ("d_hits", C.c_void_p), ("d_hits_prev", C.c_void_p), ("cam_prev", C.c_void_p)]


def temporal_inputs(d_hits, d_hist_in=None, d_hits_prev=None, cam_prev=None):
    """a TemporalInputs from device tensors (or raw ints) and the last frame's camera (a camera_dtype array); the result keeps the
    tensors and a copy of the camera alive.  d_hist_in None marks the first frame"""
    ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())
    t = TemporalInputs(ptr(d_hist_in), ptr(d_hits), ptr(d_hits_prev), None)
    t._keep = (d_hits, d_hist_in, d_hits_prev)
    if cam_prev is not None:
        t._cam = np.ascontiguousarray(cam_prev, camera_dtype).reshape(1).copy()
        t.cam_prev = t._cam.ctypes.data
    return t


class LevelsParams(C.Structure):
    """rt_levels_params: input mode (DENOISE_INPUT_*), the progressive sample count (SUM), the output format (LEVELS_*) and top_first
    (1 = the PPM's row order, 0 = the framebuffer's); include/rt_amd.h states the quantisation"""
    _fields_ = [("input", C.c_int32), ("samples", C.c_int32), ("format", C.c_int32), ("top_first", C.c_int32)]

LEVELS_RGB8, LEVELS_RGBA8, LEVELS_GRAY8 = 0, 1, 2      # rt_amd.h RT_LEVELS_*


class FrameMetrics(C.Structure):
    """rt_frame_metrics: the 64-byte record frame_compare leaves; psnr and ssim are the notebook's grey metrics (evaluations.ipynb
    :1021-1027), rmse the float error over the finite pixels — each through the library's host function"""
    _fields_ = [("pixels", C.c_int64), ("gray_sse", C.c_int64), ("gray_differ", C.c_int64), ("windows", C.c_int64), ("ssim_sum", C.c_double),
                ("finite_pixels", C.c_int64), ("sq_err", C.c_double), ("reserved", C.c_int64)]

    @property
    def psnr(self):
        return lib().rt_frame_psnr(C.byref(self))

    @property
    def ssim(self):
        return lib().rt_frame_ssim(C.byref(self))

    @property
    def rmse(self):
        return lib().rt_frame_rmse(C.byref(self))

assert C.sizeof(FrameMetrics) == 64 and C.sizeof(LevelsParams) == 16

# every symbol include/rt_amd.h declares: (restype, argtypes)
_vp, _i, _i64, _f, _P = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.POINTER
SYMBOLS = {
    "rt_abi_version": (_i, []),
    "rt_device_check": (_i, [_vp]),
    "rt_error_string": (C.c_char_p, [_i]),
    "rt_rand_init": (_i, [_vp]),
    "rt_create_world": (_i, [_vp, _i, _f, _vp, _i, _i, _vp, _i, _vp]),
    "rt_camera_init": (_i, [_vp, _vp, _vp, _vp, _f, _f, _f, _f, _i]),
    "rt_world_create": (_i, [_vp, _i, _vp, _i, _vp]),
    "rt_world_upload": (_i, [_vp]),
    "rt_world_set_camera": (_i, [_vp, _vp]),
    "rt_world_camera": (_i, [_vp, _vp]),
    "rt_world_set_geometry": (_i, [_vp, _vp, _vp]),
    "rt_world_get_geometry": (_i, [_vp, _vp, _vp]),
    "rt_free_world": (_i, [_vp]),
    "rt_build_octree": (_i, [_vp, _i, _i, _i, _vp]),
    "rt_octree_upload": (_i, [_vp]),
    "rt_build_octree_gpu": (_i, [_vp, _i, _vp, _vp]),
    "rt_octree_build_path": (_i, [_vp]),
    "rt_octree_debug_array": (_i, [_vp, _i, _vp, C.c_size_t, _vp]),
    "rt_free_octree": (_i, [_vp]),
    "rt_octree_info": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_octree_flat_info": (_i, [_vp, _vp, _vp]),
    "rt_octree_set_traversal": (_i, [_vp, _i]),
    "rt_world_set_list_traversal": (_i, [_vp, _i]),
    "rt_world_set_arith": (_i, [_vp, _i]),
    "rt_world_list_accel_info": (_i, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_octree_accel_info": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "rt_octree_nodes": (_i, [_vp, _vp]),
    "rt_octree_leaves": (_i, [_vp, _vp, _vp]),
    "rt_part_pixels": (_i64, [_i, _i, Partition]),
    "rt_render_init": (_i, [_i, _i, _vp, Partition, _vp]),
    "rt_render": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_progressive": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, Partition, _vp]),
    "rt_world_render_times": (_i, [_vp, _vp, _i, _vp]),
    "rt_render_ctx_create": (_i, [_vp]),
    "rt_render_ctx_reserve": (_i, [_vp, _i, _i, Partition]),
    "rt_render_ctx_destroy": (_i, [_vp]),
    "rt_render_on": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_progressive_on": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive": (_i, [_vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_part": (_i, [_vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_part_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_begin": (_i, [_vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_begin_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_refine": (_i, [_vp, _i, _i, _P(Adaptive), _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_refine_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_adaptive_priority": (_f, [_f, _f, _i, _f]),
    "rt_adaptive_budget_check": (_i, [_P(Budget)]),
    "rt_adaptive_budget_picks": (_i, [_P(Budget), _i, _vp]),
    "rt_adaptive_budget_select": (_i, [_vp, _vp, _i, _i, Partition, _P(Budget), _i64, _vp, _vp, _vp]),
    "rt_render_adaptive_spend": (_i, [_vp, _i, _i, _P(Budget), _vp, _vp, _vp, _vp, _vp, Partition, _vp, _vp]),
    "rt_render_adaptive_spend_on": (_i, [_vp, _vp, _i, _i, _P(Budget), _vp, _vp, _vp, _vp, _vp, Partition, _vp, _vp]),
    "rt_render_ctx_times": (_i, [_vp, _vp, _i, _vp]),
    "rt_render_ctx_counters": (_i, [_vp, _vp]),
    "rt_world_render_counters": (_i, [_vp, _vp]),
    "rt_render_ctx_schedule": (_i, [_vp, _vp, _i]),
    "rt_world_render_schedule": (_i, [_vp, _vp, _i]),
    "rt_render_ctx_schedule_reuse": (_i, [_vp, _vp, _vp]),
    "rt_world_render_schedule_reuse": (_i, [_vp, _vp, _vp]),
    "rt_render_ctx_schedule_feedback": (_i, [_vp, _vp, _vp, _i]),
    "rt_world_render_schedule_feedback": (_i, [_vp, _vp, _vp, _i]),
    "rt_render_ctx_schedule_counts": (_i, [_vp, _vp, _i64]),
    "rt_world_render_schedule_counts": (_i, [_vp, _vp, _i64]),
    "rt_render_kernel_name": (_i, [_vp, _vp, _i, _vp, _i]),
    "rt_multi_unique_id": (_i, [_vp]),
    "rt_multi_init": (_i, [_vp, _i, _i, _vp]),
    "rt_multi_probe": (_i, []),
    "rt_multi_init_custom": (_i, [_vp, _i, _i, _vp, _vp]),
    "rt_multi_destroy": (_i, [_vp]),
    "rt_multi_reserve": (_i, [_vp, _i, _i, _i, _i]),
    "rt_multi_render": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _i, _i, _vp]),
    "rt_multi_render_adaptive": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _i, _i, _vp, _vp]),
    "rt_multi_last_render_ms": (_i, [_vp, _vp, _vp]),
    "rt_multi_selftest": (_i, [_vp, _vp, _vp, C.c_size_t, _vp]),
    "rt_assemble": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "rt_assemble_split": (_i, [_vp, _vp, _i, _i, _i, _vp, _i64, _i, _vp]),
    "rt_split_balanced": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "rt_multi_set_split": (_i, [_vp, _i]),
    "rt_multi_last_split": (_i, [_vp, _vp]),
    "rt_trace_rays": (_i, [_vp, _vp, _vp, _i64, _vp, _vp]),
    "rt_render_guides": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "rt_denoise": (_i, [_vp, _vp, _i, _i, _vp, _P(DenoiseParams), _vp, _vp]),
    "rt_denoise_check": (_i, [_i, _i, _P(DenoiseParams)]),
    "rt_denoise_adaptive": (_i, [_vp, _vp, _i, _i, _vp, _vp, _P(DenoiseVarParams), _vp, _vp]),
    "rt_denoise_adaptive_check": (_i, [_i, _i, _P(DenoiseVarParams)]),
    "rt_temporal_check": (_i, [_i, _i, _P(TemporalParams)]),
    "rt_temporal_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(TemporalParams), _vp]),
    "rt_temporal_accumulate_moving": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(TemporalParams), _vp]),
    "rt_temporal_rectify_check": (_i, [_P(TemporalRectify)]),
    "rt_temporal_accumulate_rectified": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _P(TemporalParams), _P(TemporalRectify), _vp]),
    "rt_denoise_history": (_i, [_vp, _vp, _i, _i, _vp, _vp, _P(DenoiseVarParams), _vp, _vp]),
    "rt_adaptive_priority_filtered": (_f, [_f, _f, _f]),
    "rt_adaptive_budget_select_filtered": (_i, [_vp, _vp, _vp, _i, _i, _P(Budget), _P(DenoiseVarParams), _i64, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_spend_filtered": (_i, [_vp, _i, _i, _P(Budget), _P(DenoiseVarParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_spend_filtered_on": (_i, [_vp, _vp, _i, _i, _P(Budget), _P(DenoiseVarParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_adaptive_budget_select_temporal": (_i, [_vp, _vp, _vp, _i, _i, _P(Budget), _P(TemporalInputs), _P(TemporalParams), _i64, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_spend_temporal": (_i, [_vp, _i, _i, _P(Budget), _P(TemporalInputs), _P(TemporalParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_render_adaptive_spend_temporal_on": (_i, [_vp, _vp, _i, _i, _P(Budget), _P(TemporalInputs), _P(TemporalParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "rt_frame_levels": (_i, [_vp, _vp, _i, _i, _i, _P(LevelsParams), _vp]),
    "rt_frame_levels_check": (_i, [_i, _i, _i, _P(LevelsParams)]),
    "rt_frame_levels_bytes": (_i64, [_i, _i, _i]),
    "rt_frame_compare_work_bytes": (_i64, [_i, _i]),
    "rt_frame_compare": (_i, [_vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "rt_frame_psnr": (C.c_double, [_P(FrameMetrics)]),
    "rt_frame_ssim": (C.c_double, [_P(FrameMetrics)]),
    "rt_frame_rmse": (C.c_double, [_P(FrameMetrics)]),
    "rt_write_ppm": (_i, [C.c_char_p, _i, _i, _vp, _i]),
    "rt_format_ppm": (_i64, [_i, _i, _vp, _i, _vp, _i64]),
    "rt_write_image": (_i, [C.c_char_p, _i, _i, _vp, _i, _i]),
}

_LIB = None


# every symbol include/rt_amd_rebuild.h declares (the header rt_amd.h includes at its end): (restype, argtypes)
SYMBOLS_REBUILD = {
    "rt_octree_rebuild_gpu": (_i, [_vp, _vp, _vp]),
    "rt_octree_rebuild_info": (_i, [_vp, _vp, _vp, _vp]),
}

# every symbol include/rt_amd_fused.h declares (the other header rt_amd.h includes at its end): (restype, argtypes)
SYMBOLS_FUSED = {
    "rt_render_adaptive_fused": (_i, [_vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_fused_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_multi_set_adaptive_fused": (_i, [_vp, _i]),
}

# every symbol include/rt_amd_refine_fused.h declares (the header rt_amd.h includes after it): (restype, argtypes)
SYMBOLS_REFINE_FUSED = {
    "rt_render_adaptive_refine_fused": (_i, [_vp, _i, _i, _P(Adaptive), _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_refine_fused_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
}

# every symbol include/rt_amd_h16_adaptive.h declares (adaptive sampling of binary16 worlds; the header rt_amd.h includes last): (restype, argtypes)
SYMBOLS_H16_ADAPTIVE = {
    "rt_render_adaptive_h16": (_i, [_vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
    "rt_render_adaptive_h16_on": (_i, [_vp, _vp, _i, _i, _P(Adaptive), _vp, _vp, _vp, _vp, _vp, Partition, _vp]),
}


def lib():
    """Load librt_amd.so.  Raises RtError when it is missing or does not export the whole ABI (no fallback)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise RtError("librt_amd.so is not built (%s): run __graft_entry__.build() / make -C dd2360-raytracing_amd" % LIB_PATH)
        # One HIP runtime per process: PyTorch bundles its own libamdhip64.so (same soname as /opt/rocm's).  Import it
        # first so that librt_amd.so's NEEDED libamdhip64.so.7 resolves to the copy torch already mapped; two runtimes
        # in one process leave the second one without devices (hipErrorNoDevice).
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise RtError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in list(SYMBOLS.items()) + list(SYMBOLS_REBUILD.items()) + list(SYMBOLS_FUSED.items()) + list(SYMBOLS_REFINE_FUSED.items()) + list(SYMBOLS_H16_ADAPTIVE.items()):
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise RtError("librt_amd.so does not export %s" % name)
            fn.restype, fn.argtypes = res, args
        _LIB = L
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = lib().rt_error_string(int(rc))
        raise RtError("%s failed: %d (%s)" % (what, rc, msg.decode() if msg else "?"))


# ---- marshalling, written once ---------------------------------------------------------------------------------------
def _call(name, *args):
    """the symbol `name` with args; RtError, naming the symbol, unless it returns 0"""
    check(getattr(lib(), name)(*args), name)


def _np(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(t):
    """device pointer of a torch tensor (or a raw int); None stays None (NULL)"""
    return None if t is None else C.c_void_p(t if isinstance(t, int) else t.data_ptr())


def _h(obj):
    """the handle of an optional World / Octree / RenderCtx; None stays None (NULL)"""
    return None if obj is None else obj.h


def _ref(p):
    """byref of an optional parameter structure; None stays None (NULL)"""
    return None if p is None else C.byref(p)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _on(stream):
    """the caller's stream (a raw hipStream_t), or torch's current one"""
    return _stream() if stream is None else C.c_void_p(stream)


def _frame(name, ctx, stream, *args):
    """a frame call: rt_X(args, stream) on the world's own context, or, with a RenderCtx, rt_X_on(ctx, args, stream)"""
    if ctx is None:
        _call(name, *args, _on(stream))
    else:
        _call(name + "_on", ctx.h, *args, _on(stream))


def _params(cls, defaults, kw, *head):
    """cls(*head, then the fields `defaults` names, in its order): the library's defaults for whatever kw does not set"""
    p = dict(defaults, **kw)
    return cls(*head, *(p[k] for k in defaults))


class _Handle:
    """owner of h, the opaque handle a subclass's create call filled: freed once, by the symbol the subclass names in _free"""
    _free = None

    def close(self):
        if getattr(self, "h", None):
            getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Scheduled(_Handle):
    """a handle that reaches a render context's scheduling record — the context itself (_stem rt_render_ctx) or the world that owns one
    (_stem rt_world_render): the six accessors, once"""
    _stem = None

    def _times(self):
        out, n = np.zeros(64, np.float32), C.c_int(0)
        _call(self._stem + "_times", self.h, _np(out), 64, C.byref(n))
        return out[: n.value].tolist()

    def _counters(self):
        out = np.zeros(4, np.uint32)
        _call(self._stem + "_counters", self.h, _np(out))
        return dict(zip(("slots", "thin_waves", "long_chains", "long_handles"), (int(v) for v in out)))

    def _schedule(self):
        out = np.zeros(len(SCHEDULE_FIELDS), np.uint32)
        _call(self._stem + "_schedule", self.h, _np(out), len(out))
        return dict(zip(SCHEDULE_FIELDS, (int(v) for v in out)))

    def schedule_reuse(self):
        """(reused, computed): launches that reused the context's kept schedule / scheduling passes issued, since it was created"""
        a, b = C.c_uint64(0), C.c_uint64(0)
        _call(self._stem + "_schedule_reuse", self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def schedule_feedback(self):
        """the measured pass of the context's record (rt_*_schedule_feedback): passes rebuilt from recorded counts since the context was
        created ("refined"), whether the record holds counts / a rebuilt pass, the frame's largest count and the solo cap"""
        a, out = C.c_uint64(0), np.zeros(len(FEEDBACK_FIELDS), np.uint32)
        _call(self._stem + "_schedule_feedback", self.h, C.byref(a), _np(out), len(out))
        return dict(zip(("refined",) + FEEDBACK_FIELDS, [a.value] + [int(v) for v in out]))

    def schedule_counts(self, n):
        """the iteration counts the record's launch left, one uint16 per buffer element of that launch (n of them: rt_part_pixels)"""
        out = np.zeros(int(n), np.uint16)
        _call(self._stem + "_schedule_counts", self.h, _np(out), int(n))
        return out


# the frame calls, each marshalled once; the free function (current stream, the world's context) and the RenderCtx method forward here
# (`part or WHOLE` serves the methods' part=None; a free function given part=None, once a ctypes ArgumentError, now renders the whole frame)
def _render(fb, max_x, max_y, ns, world, d_rand_state, octree, part, ctx=None, stream=None):
    _frame("rt_render", ctx, stream, _dev(fb), max_x, max_y, ns, world.h, _dev(d_rand_state), _h(octree), part or WHOLE)


def _render_adaptive(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp, ctx=None, stream=None):
    _frame("rt_render_adaptive", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp))


def _render_adaptive_part(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_part", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp),
           part or WHOLE)


def _render_adaptive_begin(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_begin", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp),
           _dev(d_state), part or WHOLE)


def _render_adaptive_fused(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_fused", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp),
           _dev(d_state), part or WHOLE)


def _render_adaptive_refine(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_refine", ctx, stream, _dev(fb), max_x, max_y, C.byref(frm), C.byref(to), world.h, _dev(d_rand_state), _h(octree),
           _dev(d_spp), _dev(d_state), part or WHOLE)


def _render_adaptive_refine_fused(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_refine_fused", ctx, stream, _dev(fb), max_x, max_y, C.byref(frm), C.byref(to), world.h, _dev(d_rand_state),
           _h(octree), _dev(d_spp), _dev(d_state), part or WHOLE)


def _render_adaptive_h16(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, ctx=None, stream=None):
    _frame("rt_render_adaptive_h16", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp),
           _dev(d_state), part or WHOLE)


def _render_adaptive_spend(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, d_picked, ctx=None, stream=None):
    _frame("rt_render_adaptive_spend", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), world.h, _dev(d_rand_state), _h(octree), _dev(d_spp),
           _dev(d_state), part or WHOLE, _dev(d_picked))


def _render_adaptive_spend_filtered(fb, max_x, max_y, params, filter, d_hits, world, d_rand_state, d_state, octree, d_spp, d_picked, ctx=None,
                                    stream=None):
    _frame("rt_render_adaptive_spend_filtered", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), C.byref(filter), _dev(d_hits), world.h,
           _dev(d_rand_state), _h(octree), _dev(d_spp), _dev(d_state), _dev(d_picked))


def _render_adaptive_spend_temporal(fb, max_x, max_y, params, inputs, temporal, world, d_rand_state, d_state, octree, d_spp, d_picked, ctx=None,
                                    stream=None):
    _frame("rt_render_adaptive_spend_temporal", ctx, stream, _dev(fb), max_x, max_y, C.byref(params), C.byref(inputs), C.byref(temporal), world.h,
           _dev(d_rand_state), _h(octree), _dev(d_spp), _dev(d_state), _dev(d_picked))


def render_kernel_name(world, octree=None, mode=0):
    """the kernel rt_render (mode 0) / rt_render_progressive (mode 1) / rt_render_adaptive_fused or, binary16, rt_render_adaptive_h16
    (mode 3) / rt_render_adaptive_refine_fused (mode 4, binary32 only) launches for this world and tree"""
    buf = C.create_string_buffer(64)
    _call("rt_render_kernel_name", world.h, _h(octree), mode, buf, 64)
    return buf.value.decode()


class RenderCtx(_Scheduled):
    """rt_render_ctx: per-launch state for frames rendered concurrently on one GPU (one context per stream)"""
    _free, _stem = "rt_render_ctx_destroy", "rt_render_ctx"

    def __init__(self):
        h = C.c_void_p()
        _call("rt_render_ctx_create", C.byref(h))
        self.h = h

    def reserve(self, max_x, max_y, part=None):
        _call("rt_render_ctx_reserve", self.h, max_x, max_y, part or WHOLE)
        return self

    def render(self, fb, max_x, max_y, ns, world, d_rand_state, octree=None, part=None, stream=None):
        _render(fb, max_x, max_y, ns, world, d_rand_state, octree, part, self, stream)

    def render_adaptive(self, fb, max_x, max_y, params, world, d_rand_state, octree=None, d_spp=None, stream=None):
        """rt_render_adaptive_on: params is an Adaptive; d_spp (optional) an int32 tensor of max_x * max_y"""
        _render_adaptive(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp, self, stream)

    def render_adaptive_part(self, fb, max_x, max_y, params, world, d_rand_state, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_part_on: buffers of rt_part_pixels(part) elements (d_spp: int32), tile-major unless part is the whole frame"""
        _render_adaptive_part(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp, part, self, stream)

    def render_adaptive_begin(self, fb, max_x, max_y, params, world, d_rand_state, d_state, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_begin_on: rt_render_adaptive_part_on that also fills d_state (alloc_adaptive_state) for later refinement"""
        _render_adaptive_begin(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, self, stream)

    def render_adaptive_fused(self, fb, max_x, max_y, params, world, d_rand_state, d_state=None, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_fused_on: render_adaptive_begin's frame and state (d_state None: render_adaptive_part's frame) in one launch"""
        _render_adaptive_fused(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, self, stream)

    def render_adaptive_refine(self, fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_refine_on: continue the frame that d_state holds at target `frm` (an Adaptive) to the target `to`"""
        _render_adaptive_refine(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part, self, stream)

    def render_adaptive_refine_fused(self, fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_refine_fused_on: render_adaptive_refine's result from the seed pass and one render launch"""
        _render_adaptive_refine_fused(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part, self, stream)

    def render_adaptive_h16(self, fb, max_x, max_y, params, world, d_rand_state, d_state=None, octree=None, d_spp=None, part=None, stream=None):
        """rt_render_adaptive_h16_on: the adaptive frame of a binary16 world in one launch (fb: 3 halves per element)"""
        _render_adaptive_h16(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, self, stream)

    def render_adaptive_spend(self, fb, max_x, max_y, params, world, d_rand_state, d_state, octree=None, d_spp=None, part=None, d_picked=None,
                              stream=None):
        """rt_render_adaptive_spend_on: spend the Budget `params` on the frame that d_state holds; d_picked (optional): uint32 per round"""
        _render_adaptive_spend(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, d_picked, self, stream)

    def adaptive_budget_select(self, d_state, max_x, max_y, params, picks, d_list, d_count, part=None, stream=None):
        """rt_adaptive_budget_select: the ids of the `picks` pixels a round would choose into d_list (uint32), their number into d_count"""
        _call("rt_adaptive_budget_select", self.h, _dev(d_state), max_x, max_y, part or WHOLE, C.byref(params), picks, _dev(d_list), _dev(d_count),
              _on(stream))

    def render_adaptive_spend_filtered(self, fb, max_x, max_y, params, filter, d_hits, world, d_rand_state, d_state, octree=None, d_spp=None,
                                       d_picked=None, stream=None):
        """rt_render_adaptive_spend_filtered_on: the spend ranked by the error left after denoise_adaptive's first level (whole frames);
        filter is the DenoiseVarParams the frame will be filtered with, d_hits the guides of render_guides"""
        _render_adaptive_spend_filtered(fb, max_x, max_y, params, filter, d_hits, world, d_rand_state, d_state, octree, d_spp, d_picked, self, stream)

    def adaptive_budget_select_filtered(self, d_state, d_hits, max_x, max_y, params, filter, picks, d_list, d_count, d_keys=None, stream=None):
        """rt_adaptive_budget_select_filtered: adaptive_budget_select with the filter-aware key; d_keys (optional, float32 per pixel)
        receives every pixel's key before the eligibility mask"""
        _call("rt_adaptive_budget_select_filtered", self.h, _dev(d_state), _dev(d_hits), max_x, max_y, C.byref(params), C.byref(filter), picks,
              _dev(d_list), _dev(d_count), _dev(d_keys), _on(stream))

    def render_adaptive_spend_temporal(self, fb, max_x, max_y, params, inputs, temporal, world, d_rand_state, d_state, octree=None, d_spp=None,
                                       d_picked=None, stream=None):
        """rt_render_adaptive_spend_temporal_on: the spend ranked by the error left after temporal_accumulate's merge (whole frames);
        inputs is a TemporalInputs (temporal_inputs()), temporal the TemporalParams the history is kept with"""
        _render_adaptive_spend_temporal(fb, max_x, max_y, params, inputs, temporal, world, d_rand_state, d_state, octree, d_spp, d_picked, self, stream)

    def adaptive_budget_select_temporal(self, d_state, world, max_x, max_y, params, inputs, temporal, picks, d_list, d_count, d_keys=None,
                                        stream=None):
        """rt_adaptive_budget_select_temporal: adaptive_budget_select with the history-aware key; d_keys (optional, float32 per pixel)
        receives every pixel's key before the eligibility mask"""
        _call("rt_adaptive_budget_select_temporal", self.h, _dev(d_state), world.h, max_x, max_y, C.byref(params), C.byref(inputs), C.byref(temporal),
              picks, _dev(d_list), _dev(d_count), _dev(d_keys), _on(stream))

    def times(self):
        """device times (ms) of the render kernel of the launches since the last query (HIP events on the launch stream)"""
        return self._times()

    def counters(self):
        """scheduling counters of the latest launch: slots handed out, thin waves left, long chains pre-classified, handles taken"""
        return self._counters()

    def schedule(self):
        """the words that decided the latest launch's hand-out (rt_render_ctx_schedule): in-flight and pilot thresholds, tail mark
        (first tail slot + 1), head count, head threshold, from-end flag, raw long / solo chain counts (before the use_long gate)"""
        return self._schedule()


SPLIT_RUNS, SPLIT_BALANCED, SPLIT_BALANCED_CACHED = 0, 1, 2      # rt_amd.h RT_SPLIT_*: rt_multi_set_split
GATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
MULTI_ID_BYTES = 128           # rt_amd.h RT_MULTI_ID_BYTES


def multi_unique_id():
    """rank 0: the RCCL unique id (bytes) to hand to the other ranks"""
    buf = C.create_string_buffer(MULTI_ID_BYTES)
    _call("rt_multi_unique_id", buf)
    return buf.raw


def multi_probe():
    """rt_multi_probe: 0 when this rank could enter rt_multi_init's collective part (RCCL bound, context on the current device)"""
    return int(lib().rt_multi_probe())


class Multi(_Handle):
    """rt_multi: tile split over the ranks of a node + the single framebuffer exchange + rt_assemble on the root.
    unique_id (bytes) selects RCCL; gather (a Python callable with the rt_gather_fn arguments) a custom exchange."""
    _free = "rt_multi_destroy"

    def __init__(self, rank, nranks, unique_id=None, gather=None):
        h = C.c_void_p()
        if gather is not None:
            self._cb = GATHER_FN(gather)                          # keep the thunk alive
            _call("rt_multi_init_custom", C.byref(h), rank, nranks, C.cast(self._cb, C.c_void_p), None)
        else:
            assert unique_id is not None and len(unique_id) == MULTI_ID_BYTES
            self._id = C.create_string_buffer(unique_id, MULTI_ID_BYTES)
            _call("rt_multi_init", C.byref(h), rank, nranks, self._id)
        self.h, self.rank, self.nranks = h, rank, nranks
        self.split_mode = SPLIT_RUNS                             # the library's default (rt_multi_set_split)

    def reserve(self, max_x, max_y, precision=FP32, root=0):
        _call("rt_multi_reserve", self.h, max_x, max_y, precision, root)
        return self

    def render(self, fb_full, max_x, max_y, ns, world, octree=None, root=0, precision=None):
        _call("rt_multi_render", self.h, _dev(fb_full), max_x, max_y, ns, world.h, _h(octree), world.precision if precision is None else precision,
              root, _stream())

    def render_adaptive(self, fb_full, max_x, max_y, params, world, octree=None, root=0, d_spp_full=None, precision=None):
        """rt_multi_render_adaptive (RT_SPLIT_RUNS only): the root gets the frame and, d_spp_full given (int32, max_x * max_y), the count map"""
        _call("rt_multi_render_adaptive", self.h, _dev(fb_full), max_x, max_y, C.byref(params), world.h, _h(octree),
              world.precision if precision is None else precision, root, _dev(d_spp_full), _stream())

    def set_split(self, mode):
        _call("rt_multi_set_split", self.h, mode)
        self.split_mode = mode
        return self

    def set_adaptive_fused(self, on):
        """rt_multi_set_adaptive_fused: 1 = render_adaptive renders each rank's part in one launch (the same bits), 0 = in rounds"""
        _call("rt_multi_set_adaptive_fused", self.h, int(on))
        return self

    def last_split(self):
        st = (C.c_int64 * (self.nranks + 1))()
        _call("rt_multi_last_split", self.h, st)
        return list(st)

    def last_render_ms(self):
        a, b = C.c_float(0), C.c_float(0)
        _call("rt_multi_last_render_ms", self.h, C.byref(a), C.byref(b))
        return a.value, b.value

    def selftest(self, d_src, d_dst, nbytes):
        _call("rt_multi_selftest", self.h, _dev(d_src), _dev(d_dst), nbytes, _stream())


def device_check():
    n = C.c_int(0)
    rc = lib().rt_device_check(C.byref(n))
    return rc, n.value


def split_balanced(world, octree, max_x, max_y, nparts, counts=False):
    """rt_split_balanced: starts[nparts + 1] of the bands of equal predicted cost (and, counts=True, the pilot's per-tile bounces, tests and columns)"""
    tiles = ((max_x + 7) // 8) * ((max_y + 7) // 8)
    st = (C.c_int64 * (nparts + 1))()
    btc = [np.zeros(tiles, np.int32) for _ in range(3)] if counts else [None] * 3
    _call("rt_split_balanced", None, world.h, _h(octree), max_x, max_y, nparts, st, *(_np(a) if counts else None for a in btc), _stream())
    return (list(st), *btc) if counts else list(st)


def split_parts(starts):
    """the rt_partition of every band of a split"""
    n = len(starts) - 1
    return [Partition(p, n, starts[p], starts[p + 1]) for p in range(n)]


def assemble_split(fb_full, fb_parts, max_x, max_y, starts, part_stride_px, precision=FP32):
    n = len(starts) - 1
    st = (C.c_int64 * (n + 1))(*starts)
    _call("rt_assemble_split", _dev(fb_full), _dev(fb_parts), max_x, max_y, n, st, part_stride_px, precision, _stream())


def _size(name, *args):
    """a host-only size query: the count, RtError for the negative that marks an invalid argument"""
    n = getattr(lib(), name)(*args)
    if n < 0:
        raise RtError("%s: invalid argument" % name)
    return n


def part_pixels(max_x, max_y, part=WHOLE):
    return _size("rt_part_pixels", max_x, max_y, part)


class World(_Scheduled):
    """rand_init + create_world of main.cu:388-401 (host side), and the device scene they feed."""
    _free, _stem = "rt_free_world", "rt_world_render"

    def __init__(self, num_spheres, nx, ny, sphere_radius=0.1, precision=FP32, spheres=None, camera=None):
        self.num_spheres, self.nx, self.ny, self.precision = num_spheres, nx, ny, precision
        self.rand_state = np.zeros(1, rand_state_dtype)
        if spheres is None:
            self.spheres = np.zeros(num_spheres, sphere_dtype)
            self.camera = np.zeros(1, camera_dtype)
            created = C.c_int(0)
            _call("rt_rand_init", _np(self.rand_state))
            _call("rt_create_world", _np(self.spheres), num_spheres, sphere_radius, _np(self.camera), nx, ny, _np(self.rand_state), precision,
                  C.byref(created))
            self.created = created.value
        else:
            self.spheres = np.ascontiguousarray(spheres, sphere_dtype)
            self.camera = np.ascontiguousarray(camera, camera_dtype).reshape(1)
            self.created = int((self.spheres["material"] != MAT_NONE).sum())
        h = C.c_void_p()
        _call("rt_world_create", _np(self.spheres), num_spheres, _np(self.camera), precision, C.byref(h))
        self.h = h

    def upload(self):
        _call("rt_world_upload", self.h)
        return self

    def set_camera(self, cam):
        """rt_world_set_camera: the camera (a camera_dtype record) of every launch from now on; host only, launches already enqueued keep
        theirs"""
        cam = np.ascontiguousarray(cam, camera_dtype).reshape(1).copy()
        _call("rt_world_set_camera", self.h, _np(cam))
        self.camera = cam
        return self

    def get_camera(self):
        """rt_world_camera: the camera the next launch will use, as a camera_dtype array of one record"""
        cam = np.zeros(1, camera_dtype)
        _call("rt_world_camera", self.h, _np(cam))
        return cam

    def set_geometry(self, d_geom):
        """rt_world_set_geometry on the current stream: d_geom is a float32 device tensor of num_spheres x 4 (cx, cy, cz, radius) in
        world-list order.  Octrees built before the call describe the old geometry: build them again (Octree(world, spl, gpu=True), or
        octree.rebuild() in place)"""
        _call("rt_world_set_geometry", self.h, _dev(d_geom), _stream())
        self._spheres_stale = True
        return self

    def get_geometry(self, d_out=None):
        """rt_world_get_geometry on the current stream: the world's geometry as a float32 device tensor [num_spheres, 4] (d_out, or a new one)"""
        if d_out is None:
            import torch
            d_out = torch.empty((self.num_spheres, 4), dtype=torch.float32, device="cuda")
        _call("rt_world_get_geometry", self.h, _dev(d_out), _stream())
        return d_out

    def host_spheres(self):
        """self.spheres with the geometry the device holds: downloaded (a synchronising copy) after a set_geometry"""
        if getattr(self, "_spheres_stale", False):
            g = self.get_geometry().cpu().numpy()
            self.spheres["center"] = g[:, :3]
            self.spheres["radius"] = g[:, 3]
            self._spheres_stale = False
        return self.spheres

    def set_list_traversal(self, mode):
        """TRAVERSAL_REFERENCE (every sphere in list order) or TRAVERSAL_FAST (default: the candidate grid) for renders without an octree"""
        _call("rt_world_set_list_traversal", self.h, mode)
        return self

    def set_arith(self, mode):
        """ARITH_IEEE (default, the parity contract) or ARITH_CONTRACT (FMA contraction allowed: a tolerance mode)"""
        _call("rt_world_set_arith", self.h, mode)
        return self

    def list_accel_info(self):
        e, g, h, n, l = C.c_int(0), C.c_int(0), C.c_float(0), C.c_int(0), C.c_int(0)
        _call("rt_world_list_accel_info", self.h, C.byref(e), C.byref(g), C.byref(h), C.byref(n), C.byref(l))
        return {"enabled": bool(e.value), "grid_dim": g.value, "cell_size": h.value, "grid_entries": n.value, "large_spheres": l.value}

    def render_times(self):
        """device times (ms) of the render kernel of the calls since the last query (HIP events on the launch stream)"""
        return self._times()

    def render_counters(self):
        """scheduling counters of the latest render() on this world (see RenderCtx.counters)"""
        return self._counters()

    def render_schedule(self):
        """the words that decided the hand-out of the latest render() on this world (see RenderCtx.schedule)"""
        return self._schedule()


class Octree(_Handle):
    """buildOctree (acceleration_structure.h:195) + upload (main.cu:413-417)."""
    _free = "rt_free_octree"

    def __init__(self, world, spheres_per_leaf=30, gpu=False):
        """gpu=True: rt_build_octree_gpu (built on the device from the world's device copy, ready to render)"""
        self.world, self.spl = world, spheres_per_leaf
        h = C.c_void_p()
        if gpu:
            _call("rt_build_octree_gpu", world.h, spheres_per_leaf, C.byref(h), _stream())
        else:
            _call("rt_build_octree", _np(world.host_spheres()), world.num_spheres, spheres_per_leaf, world.precision, C.byref(h))
        self.h = h

    def upload(self):
        _call("rt_octree_upload", self.h)
        return self

    def build_path(self):
        """rt_octree_build_path: BUILD_HOST, BUILD_DEVICE or BUILD_HOST_DECLINED (gpu=True, but the device build declined the input)"""
        return _size("rt_octree_build_path", self.h)

    def rebuild(self, world=None):
        """rt_octree_rebuild_gpu on the current stream: the tree of the world's current device geometry (after set_geometry) in this
        handle, which a gpu=True build made; everything observable equals a fresh Octree(world, spl, gpu=True)"""
        _call("rt_octree_rebuild_gpu", self.h, _h(self.world if world is None else world), _stream())
        return self

    def rebuild_info(self):
        """rt_octree_rebuild_info: rebuilds that succeeded, how many of them had to enlarge the kept memory or run twice, and the
        host-blocking waits of the last one"""
        v = [C.c_uint64(0) for _ in range(3)]
        _call("rt_octree_rebuild_info", self.h, *[C.byref(x) for x in v])
        return dict(zip(("rebuilds", "regrown", "host_syncs_last"), (x.value for x in v)))

    def set_traversal(self, mode):
        """TRAVERSAL_REFERENCE (exact bucket scan) or TRAVERSAL_FAST (default, culling grid + fallback)"""
        _call("rt_octree_set_traversal", self.h, mode)
        return self

    def device_array(self, which):
        """bytes of one device-resident array of the (uploaded) tree, see rt_octree_debug_array"""
        n = C.c_size_t(0)
        _call("rt_octree_debug_array", self.h, which, None, 0, C.byref(n))
        buf = np.zeros(max(1, n.value), np.uint8)
        _call("rt_octree_debug_array", self.h, which, _np(buf), n.value, C.byref(n))
        return buf[: n.value]

    def accel_info(self):
        g, n, l = C.c_int(0), C.c_int(0), C.c_int(0)
        h = C.c_float(0)
        _call("rt_octree_accel_info", self.h, C.byref(g), C.byref(h), C.byref(n), C.byref(l))
        return dict(grid_dim=g.value, cell_size=h.value, grid_entries=n.value, large_spheres=l.value)

    def info(self):
        v = [C.c_int(0) for _ in range(5)]
        _call("rt_octree_info", self.h, *[C.byref(x) for x in v])
        fn, fe = C.c_int(0), C.c_int(0)
        _call("rt_octree_flat_info", self.h, C.byref(fn), C.byref(fe))
        keys = ["node_count", "leaf_count", "spl", "dropped_full", "dropped_outside"]
        d = dict(zip(keys, [x.value for x in v]))
        d.update(flat_nodes=fn.value, flat_entries=fe.value)
        return d

    def nodes(self):
        out = np.zeros(OCTREE_MAX_NODES, octnode_dtype)
        _call("rt_octree_nodes", self.h, _np(out))
        return out

    def leaves(self):
        lc = self.info()["leaf_count"]
        counts = np.zeros(lc, np.int32)
        idx = np.zeros((lc, self.spl), np.int32)
        _call("rt_octree_leaves", self.h, _np(counts), _np(idx))
        return counts, idx


def camera_init(lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, precision=FP32):
    cam = np.zeros(1, camera_dtype)
    a = [np.asarray(x, np.float32) for x in (lookfrom, lookat, vup)]
    _call("rt_camera_init", _np(cam), _np(a[0]), _np(a[1]), _np(a[2]), vfov, aspect, aperture, focus_dist, precision)
    return cam


# ---- device-side calls: buffers are torch CUDA tensors -------------------------------------------------------------
def alloc_rand_state(max_x, max_y, part=WHOLE, device="cuda"):
    import torch
    return torch.zeros(part_pixels(max_x, max_y, part) * 48, dtype=torch.uint8, device=device)


def alloc_fb(max_x, max_y, part=WHOLE, precision=FP32, device="cuda"):
    import torch
    return torch.zeros(part_pixels(max_x, max_y, part) * 3, dtype=torch.float32 if precision == FP32 else torch.float16, device=device)


def render_init(max_x, max_y, d_rand_state, part=WHOLE):
    _call("rt_render_init", max_x, max_y, _dev(d_rand_state), part, _stream())


def render(fb, max_x, max_y, ns, world, d_rand_state, octree=None, part=WHOLE):
    _render(fb, max_x, max_y, ns, world, d_rand_state, octree, part)


def render_progressive(fb, max_x, max_y, current_sample, world, d_rand_state, octree=None, part=WHOLE):
    _call("rt_render_progressive", _dev(fb), max_x, max_y, current_sample, world.h, _dev(d_rand_state), _h(octree), part, _stream())


def render_adaptive(fb, max_x, max_y, params, world, d_rand_state, octree=None, d_spp=None):
    """rt_render_adaptive on the current stream: params is an Adaptive; d_spp (optional) an int32 tensor of max_x * max_y"""
    _render_adaptive(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp)


def render_adaptive_part(fb, max_x, max_y, params, world, d_rand_state, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_part on the current stream: buffers of rt_part_pixels(part) elements (d_spp: int32), tile-major unless part is the whole frame"""
    _render_adaptive_part(fb, max_x, max_y, params, world, d_rand_state, octree, d_spp, part)


def alloc_adaptive_state(max_x, max_y, part=WHOLE, device="cuda"):
    """the refinement state of rt_render_adaptive_begin / _refine: ADAPTIVE_STATE_BYTES per buffer element of the part"""
    import torch
    return torch.zeros(part_pixels(max_x, max_y, part) * ADAPTIVE_STATE_BYTES, dtype=torch.uint8, device=device)


def render_adaptive_begin(fb, max_x, max_y, params, world, d_rand_state, d_state, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_begin on the current stream: rt_render_adaptive_part that also fills d_state (alloc_adaptive_state)"""
    _render_adaptive_begin(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part)


def render_adaptive_fused(fb, max_x, max_y, params, world, d_rand_state, d_state=None, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_fused on the current stream: what render_adaptive_begin leaves (d_state None: what render_adaptive_part
    leaves), from one scheduling pass and one render launch - the stop rule runs inside the kernel"""
    _render_adaptive_fused(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part)


def render_adaptive_refine(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_refine on the current stream: continue the frame that d_state holds at target `frm` to the target `to`;
    afterwards fb, d_spp, d_rand_state and d_state hold what render_adaptive_begin(to) would have left"""
    _render_adaptive_refine(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part)


def render_adaptive_refine_fused(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_refine_fused on the current stream: what render_adaptive_refine leaves, from its seed pass and one render
    launch - every listed pixel resumes from the state and the stop rule runs inside the kernel"""
    _render_adaptive_refine_fused(fb, max_x, max_y, frm, to, world, d_rand_state, d_state, octree, d_spp, part)


def render_adaptive_h16(fb, max_x, max_y, params, world, d_rand_state, d_state=None, octree=None, d_spp=None, part=WHOLE):
    """rt_render_adaptive_h16 on the current stream: the adaptive frame of a binary16 world in one launch — every pixel is
    render(ns = its count)'s pixel; d_state (alloc_adaptive_state, optional) takes every pixel's sums and count"""
    _render_adaptive_h16(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part)


def adaptive_priority(SL, Q, k, floor):
    """rt_adaptive_priority: the key a budget ranks a pixel by (host, binary32)"""
    return np.float32(lib().rt_adaptive_priority(float(np.float32(SL)), float(np.float32(Q)), int(k), float(np.float32(floor))))


def adaptive_budget_check(params):
    """rt_adaptive_budget_check: True when the Budget is accepted (host only)"""
    return lib().rt_adaptive_budget_check(C.byref(params)) == 0


def adaptive_budget_picks(params, round):
    """rt_adaptive_budget_picks: K_r, the picks of round `round`"""
    k = C.c_int64(0)
    _call("rt_adaptive_budget_picks", C.byref(params), round, C.byref(k))
    return k.value


def adaptive_budget_select(ctx, d_state, max_x, max_y, params, picks, d_list, d_count, part=WHOLE):
    """rt_adaptive_budget_select on the current stream, with the workspace of the RenderCtx `ctx`"""
    ctx.adaptive_budget_select(d_state, max_x, max_y, params, picks, d_list, d_count, part)


def render_adaptive_spend(fb, max_x, max_y, params, world, d_rand_state, d_state, octree=None, d_spp=None, part=WHOLE, d_picked=None):
    """rt_render_adaptive_spend on the current stream: spend the Budget `params` on the frame that d_state holds (render_adaptive_begin,
    _refine or an earlier spend left it); d_picked (optional): one uint32 per round, the round's pick count"""
    _render_adaptive_spend(fb, max_x, max_y, params, world, d_rand_state, d_state, octree, d_spp, part, d_picked)


def adaptive_priority_filtered(l, v, floor):
    """rt_adaptive_priority_filtered: the key of a filtered pixel — l the luminance of its filtered mean, v that mean's variance"""
    return np.float32(lib().rt_adaptive_priority_filtered(float(np.float32(l)), float(np.float32(v)), float(np.float32(floor))))


def adaptive_budget_select_filtered(ctx, d_state, d_hits, max_x, max_y, params, filter, picks, d_list, d_count, d_keys=None):
    """rt_adaptive_budget_select_filtered on the current stream, with the workspace of the RenderCtx `ctx`"""
    ctx.adaptive_budget_select_filtered(d_state, d_hits, max_x, max_y, params, filter, picks, d_list, d_count, d_keys)


def render_adaptive_spend_filtered(fb, max_x, max_y, params, filter, d_hits, world, d_rand_state, d_state, octree=None, d_spp=None, d_picked=None):
    """rt_render_adaptive_spend_filtered on the current stream: render_adaptive_spend with the pixels ranked by the error that is left
    after the first level of denoise_adaptive (filter: its DenoiseVarParams, d_hits: the guides); fb stays unfiltered"""
    _render_adaptive_spend_filtered(fb, max_x, max_y, params, filter, d_hits, world, d_rand_state, d_state, octree, d_spp, d_picked)


def adaptive_budget_select_temporal(ctx, d_state, world, max_x, max_y, params, inputs, temporal, picks, d_list, d_count, d_keys=None):
    """rt_adaptive_budget_select_temporal on the current stream, with the workspace of the RenderCtx `ctx`"""
    ctx.adaptive_budget_select_temporal(d_state, world, max_x, max_y, params, inputs, temporal, picks, d_list, d_count, d_keys)


def render_adaptive_spend_temporal(fb, max_x, max_y, params, inputs, temporal, world, d_rand_state, d_state, octree=None, d_spp=None, d_picked=None):
    """rt_render_adaptive_spend_temporal on the current stream: render_adaptive_spend with the pixels ranked by the error that is left
    after temporal_accumulate merged them with the last frame's history (inputs: temporal_inputs(), temporal: its TemporalParams); fb
    stays unfiltered and the history is only read — run temporal_accumulate after the spend"""
    _render_adaptive_spend_temporal(fb, max_x, max_y, params, inputs, temporal, world, d_rand_state, d_state, octree, d_spp, d_picked)


def assemble(fb_full, fb_parts, max_x, max_y, nparts, precision=FP32):
    _call("rt_assemble", _dev(fb_full), _dev(fb_parts), max_x, max_y, nparts, precision, _stream())


def trace_rays(world, octree, d_rays, n, d_out):
    _call("rt_trace_rays", world.h, _h(octree), _dev(d_rays), n, _dev(d_out), _stream())


def alloc_guides(max_x, max_y, device="cuda"):
    """the guide buffer of render_guides: one 32-byte rt_hit_record per pixel (view it on the host with hit_record_dtype)"""
    import torch
    return torch.zeros(max_x * max_y * 32, dtype=torch.uint8, device=device)


def alloc_denoise_work(max_x, max_y, device="cuda"):
    """the workspace of denoise: DENOISE_WORK_BYTES per pixel"""
    import torch
    return torch.empty(max_x * max_y * DENOISE_WORK_BYTES // 4, dtype=torch.float32, device=device)


def render_guides(world, octree, max_x, max_y, d_hits):
    """rt_render_guides on the current stream: the first hit of every pixel's centre ray, row-major, into d_hits (alloc_guides)"""
    _call("rt_render_guides", world.h, _h(octree), max_x, max_y, _dev(d_hits), _stream())


def denoise_check(max_x, max_y, params):
    """rt_denoise_check: True when denoise accepts a frame of this size with these parameters (host only, nothing is launched)"""
    return lib().rt_denoise_check(max_x, max_y, C.byref(params)) == 0


def denoise(fb_out, fb_in, max_x, max_y, d_hits, params, d_work):
    """rt_denoise on the current stream: params is a DenoiseParams (denoise_params()); fb_out may be fb_in"""
    _call("rt_denoise", _dev(fb_out), _dev(fb_in), max_x, max_y, _dev(d_hits), C.byref(params), _dev(d_work), _stream())


def denoise_adaptive_check(max_x, max_y, params):
    """rt_denoise_adaptive_check: True when denoise_adaptive accepts a frame of this size with these parameters (host only)"""
    return lib().rt_denoise_adaptive_check(max_x, max_y, C.byref(params)) == 0


def denoise_adaptive(fb_out, fb_in, max_x, max_y, d_hits, d_state, params, d_work):
    """rt_denoise_adaptive on the current stream: d_state is the whole-frame state render_adaptive_begin / _refine left, fb_in the frame
    of the same call, params a DenoiseVarParams (denoise_var_params()); fb_out may be fb_in"""
    _call("rt_denoise_adaptive", _dev(fb_out), _dev(fb_in), max_x, max_y, _dev(d_hits), _dev(d_state), C.byref(params), _dev(d_work), _stream())


def alloc_temporal_history(max_x, max_y, device="cuda"):
    """a history of temporal_accumulate: TEMPORAL_HISTORY_BYTES per pixel, zeroed (neff = 0: nothing accumulated); view the first
    4 * n floats as (n, 4) for (x.r, x.g, x.b, v) and the last n as neff"""
    import torch
    return torch.zeros(max_x * max_y * TEMPORAL_HISTORY_BYTES // 4, dtype=torch.float32, device=device)


def temporal_check(max_x, max_y, params):
    """rt_temporal_check: True when temporal_accumulate accepts a frame of this size with these parameters (host only)"""
    return lib().rt_temporal_check(max_x, max_y, C.byref(params)) == 0


def _temporal_accumulate(name, d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, geom, d_state, world, max_x, max_y, *params):
    """what the three temporal_accumulate* share: on the first frame (d_hist_in None) the history, the last frame's guides and its camera
    all go as NULL, whatever was passed for them.  `geom` holds the d_geom_prev pointer of the forms that take one, and here the two
    differ, on purpose left as they were: temporal_accumulate_moving also nulls d_geom_prev on the first frame,
    temporal_accumulate_rectified sends it as given."""
    first = d_hist_in is None
    cam = None if first else _np(np.ascontiguousarray(cam_prev, camera_dtype).reshape(1))
    _call(name, _dev(d_hist_out), None if first else _dev(d_hist_in), _dev(d_hits), None if first else _dev(d_hits_prev), cam, *geom, _dev(d_state),
          world.h, max_x, max_y, *params, _stream())


def temporal_accumulate(d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, d_state, world, max_x, max_y, params):
    """rt_temporal_accumulate on the current stream: this frame's history into d_hist_out from its state and guides and, unless
    d_hist_in is None (the first frame), the history, guides and camera (a camera_dtype array) of the last frame; params is a
    TemporalParams (temporal_params())"""
    _temporal_accumulate("rt_temporal_accumulate", d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, (), d_state, world, max_x, max_y,
                         C.byref(params))


def temporal_accumulate_moving(d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, d_geom_prev, d_state, world, max_x, max_y, params):
    """rt_temporal_accumulate_moving on the current stream: temporal_accumulate for a world whose spheres moved (World.set_geometry)
    since the frame that wrote d_hist_in; d_geom_prev is what World.get_geometry returned for that frame (None with d_hist_in None)"""
    _temporal_accumulate("rt_temporal_accumulate_moving", d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev,
                         (None if d_hist_in is None else _dev(d_geom_prev),), d_state, world, max_x, max_y, C.byref(params))


def temporal_rectify_check(rectify):
    """rt_temporal_rectify_check: True when temporal_accumulate_rectified accepts these rectification parameters (host only)"""
    return lib().rt_temporal_rectify_check(_ref(rectify)) == 0


def temporal_accumulate_rectified(d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, d_state, world, max_x, max_y, params, rectify,
                                  d_geom_prev=None):
    """rt_temporal_accumulate_rectified on the current stream: temporal_accumulate (d_geom_prev None) or temporal_accumulate_moving
    (d_geom_prev: what World.get_geometry returned for the frame that wrote d_hist_in) whose history sheds effective samples where this
    frame's neighbourhood contradicts it; rectify is a TemporalRectify (temporal_rectify())"""
    _temporal_accumulate("rt_temporal_accumulate_rectified", d_hist_out, d_hist_in, d_hits, d_hits_prev, cam_prev, (_dev(d_geom_prev),), d_state,
                         world, max_x, max_y, C.byref(params), _ref(rectify))


def denoise_history(fb_out, fb_in, max_x, max_y, d_hits, d_hist, params, d_work):
    """rt_denoise_history on the current stream: denoise_adaptive with the mean and variance of every pixel taken from the history
    d_hist (temporal_accumulate); fb_in supplies the pass-through pixels, fb_out may be fb_in"""
    _call("rt_denoise_history", _dev(fb_out), _dev(fb_in), max_x, max_y, _dev(d_hits), _dev(d_hist), C.byref(params), _dev(d_work), _stream())


def frame_levels_bytes(max_x, max_y, fmt=LEVELS_RGB8):
    """rt_frame_levels_bytes: the size of frame_levels' output"""
    return _size("rt_frame_levels_bytes", max_x, max_y, fmt)


def frame_levels(d_out, fb, max_x, max_y, params, precision=FP32):
    """rt_frame_levels on the current stream: the frame as 8-bit levels into d_out (a uint8 tensor of frame_levels_bytes), params a
    LevelsParams"""
    _call("rt_frame_levels", _dev(d_out), _dev(fb), max_x, max_y, precision, C.byref(params), _stream())


def alloc_compare_work(max_x, max_y, device="cuda"):
    """the workspace of frame_compare: rt_frame_compare_work_bytes bytes (one partial record per block)"""
    import torch
    return torch.empty(_size("rt_frame_compare_work_bytes", max_x, max_y) // 8, dtype=torch.float64, device=device)


def frame_metrics(d_metrics):
    """the FrameMetrics a frame_compare with d_metrics left on the device (synchronises: a 64-byte copy)"""
    return FrameMetrics.from_buffer_copy(d_metrics.cpu().numpy().tobytes())


def frame_compare(fb_a, fb_b, max_x, max_y, d_work, precision_a=FP32, precision_b=FP32, d_ssim_map=None, d_metrics=None):
    """rt_frame_compare on the current stream: two gamma frames, each with its own precision; d_work from alloc_compare_work, d_ssim_map
    (optional) a float64 tensor of (max_y-6) * (max_x-6).  Returns the record as a FrameMetrics (.psnr, .ssim, .rmse) after copying its
    64 bytes back; with d_metrics (a 64-byte device tensor, 8-byte aligned) the call only enqueues, for a capture, and returns None:
    read it with frame_metrics(d_metrics)"""
    import torch
    own = d_metrics is None
    if own:
        d_metrics = torch.empty(8, dtype=torch.int64, device=fb_a.device)
    _call("rt_frame_compare", _dev(fb_a), precision_a, _dev(fb_b), precision_b, max_x, max_y, _dev(d_metrics), _dev(d_ssim_map), _dev(d_work),
          _stream())
    return frame_metrics(d_metrics) if own else None


def write_image(path, fb_host, nx, ny, precision=FP32, fmt=IMAGE_P6):
    fb_host = np.ascontiguousarray(fb_host)
    _call("rt_write_image", str(path).encode(), nx, ny, _np(fb_host), precision, fmt)


def format_ppm(fb_host, nx, ny, precision=FP32):
    fb_host = np.ascontiguousarray(fb_host)
    cap = nx * ny * 36 + 64                                      # three ints of <= 11 characters per pixel: formatted once
    buf = C.create_string_buffer(cap)
    n = lib().rt_format_ppm(nx, ny, _np(fb_host), precision, buf, cap)
    if n < 0 or n > cap:
        raise RtError("rt_format_ppm failed: %d" % n)
    return buf.raw[:n]
