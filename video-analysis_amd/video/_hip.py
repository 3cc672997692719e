"""ctypes binding of libvideoanalysis_hip.so (include/videoanalysis_hip.h).

This is the ONLY compute backend of the package: there is no NumPy/CPU fallback.  If the
shared library is missing, or no MI355X is visible, every filter/analysis call raises
:class:`HipUnavailableError` instead of silently computing something else.
"""
import ctypes as C
import os
import weakref

import numpy as np

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG_DIR, "lib", "libvideoanalysis_hip.so")

VA_U8, VA_F32, VA_F64, VA_I16 = 0, 1, 2, 3
BG_NONE, BG_MEAN, BG_EMA, BG_STATIC = 0, 1, 2, 3
MORPH_ERODE, MORPH_DILATE = 0, 1
SHAPE_RECT, SHAPE_CROSS, SHAPE_ELLIPSE = 0, 1, 2
TAPS_CV4, TAPS_CV3 = 0, 1
TAP_RULES = {None: TAPS_CV4, "cv4": TAPS_CV4, "cv3": TAPS_CV3}
MAX_MORPH_OPS = 4
STATS_STRIDE = 16
STAT_NAMES = ("area", "m10", "m01", "m20", "m11", "m02", "m30", "m21", "m12", "m03",
              "xmin", "ymin", "xmax", "ymax")

BG_MODES = {None: BG_NONE, "none": BG_NONE, "mean": BG_MEAN, "ema": BG_EMA, "static": BG_STATIC}
MORPH_OPS = {"erode": MORPH_ERODE, "dilate": MORPH_DILATE}
SHAPES = {"rect": SHAPE_RECT, "cross": SHAPE_CROSS, "ellipse": SHAPE_ELLIPSE}


class HipError(RuntimeError):
    """a call into libvideoanalysis_hip.so failed"""

    def __init__(self, code, message):
        super().__init__("libvideoanalysis_hip: %s (code %d)" % (message, code))
        self.code = code


class HipUnavailableError(HipError):
    """the HIP extension (or a GPU) is not available -- there is no CPU fallback"""

    def __init__(self, message):
        HipError.__init__(self, -19, message)


class va_config(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
                ("channels", C.c_int32), ("dtype", C.c_int32), ("max_batch", C.c_int32),
                ("bg_mode", C.c_int32), ("bg_rate", C.c_float), ("sigma", C.c_double),
                ("thresh", C.c_int32), ("maxval", C.c_int32), ("morph_count", C.c_int32),
                ("morph_op", C.c_int32 * MAX_MORPH_OPS),
                ("morph_shape", C.c_int32 * MAX_MORPH_OPS),
                ("morph_ksize", C.c_int32 * MAX_MORPH_OPS),
                ("connectivity", C.c_int32), ("max_labels", C.c_int32), ("tap_rule", C.c_int32)]


class va_match_query(C.Structure):
    _fields_ = [(name, C.c_int32) for name in ("frame", "templ", "x0", "y0", "nx", "ny")]


class va_match_best(C.Structure):
    _fields_ = [("score", C.c_double), ("x", C.c_int32), ("y", C.c_int32), ("status", C.c_int32),
                ("reserved", C.c_int32)]


class va_match_args(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("method", C.c_int32), ("frames_dev", C.c_void_p),
                ("n", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("reserved", C.c_int32),
                ("frame_stride", C.c_int64), ("templates_dev", C.c_void_p), ("template_shapes_dev", C.c_void_p),
                ("template_offsets_dev", C.c_void_p), ("n_templates", C.c_int64), ("queries_dev", C.c_void_p),
                ("n_queries", C.c_int64), ("total_positions", C.c_int64), ("best_out_dev", C.c_void_p),
                ("maps_out_dev", C.c_void_p), ("map_offsets_dev", C.c_void_p), ("workspace_dev", C.c_void_p),
                ("workspace_bytes", C.c_size_t), ("stream", C.c_void_p)]


MATCH_METHODS = {"sqdiff": 0, "sqdiff_normed": 1, "ccorr": 2, "ccorr_normed": 3, "ccoeff": 4, "ccoeff_normed": 5}
MATCH_QUERY_DTYPE = np.dtype([(name, np.int32) for name in ("frame", "templ", "x0", "y0", "nx", "ny")])
MATCH_BEST_DTYPE = np.dtype([("score", np.float64), ("x", np.int32), ("y", np.int32), ("status", np.int32),
                             ("reserved", np.int32)])
MATCH_MAX_TEMPLATE_PIXELS = 65536

_vp, _i, _sz, _d, _i64 = C.c_void_p, C.c_int, C.c_size_t, C.c_double, C.c_int64

# name -> (restype, argtypes); mirrors include/videoanalysis_hip.h one to one
SIGNATURES = {
    "va_init": (_i, [_i]),
    "va_device_count": (_i, []),
    "va_version": (C.c_char_p, []),
    "va_last_error": (C.c_char_p, []),
    "va_trim": (_i, [_sz]),
    "va_malloc": (_i, [C.POINTER(_vp), _sz]),
    "va_free": (_i, [_vp]),
    "va_host_alloc": (_i, [C.POINTER(_vp), _sz]),
    "va_host_free": (_i, [_vp]),
    "va_memcpy_h2d": (_i, [_vp, _vp, _sz, _vp]),
    "va_memcpy_d2h": (_i, [_vp, _vp, _sz, _vp]),
    "va_memcpy_d2d": (_i, [_vp, _vp, _sz, _vp]),
    "va_memset": (_i, [_vp, _i, _sz, _vp]),
    "va_stream_sync": (_i, [_vp]),
    "va_stream_create": (_i, [C.POINTER(_vp)]),
    "va_stream_destroy": (_i, [_vp]),
    "va_event_create": (_i, [C.POINTER(_vp)]),
    "va_event_destroy": (_i, [_vp]),
    "va_event_record": (_i, [_vp, _vp]),
    "va_stream_wait_event": (_i, [_vp, _vp]),
    "va_event_sync": (_i, [_vp]),
    "va_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "va_gaussian_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _vp]),
    "va_gaussian_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _vp]),
    "va_gaussian_u8_rule": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _i, _vp]),
    "va_gauss_taps_q8": (_i, [_d, C.POINTER(_i), _vp, _i]),
    "va_gauss_taps_q8_rule": (_i, [_d, _i, C.POINTER(_i), _vp, _i]),
    "va_gauss_taps_f32": (_i, [_d, C.POINTER(_i), _vp, _i]),
    "va_bg_update": (_i, [_i, _i, _vp, _vp, _vp, _i64, _d, _i, _sz, _vp]),
    "va_welford_u8": (_i, [_vp, _vp, _vp, _i64, _i, _sz, _vp]),
    "va_mean_any": (_i, [_vp, _i, _vp, _i64, _i, _sz, _vp]),
    "va_welford_any": (_i, [_vp, _i, _vp, _vp, _i64, _i, _sz, _vp]),
    "va_temporal_ranks_u8": (_i, [_vp, _i, _sz, _sz, _vp, _i, _vp, _vp]),
    "va_sliding_median_state_bytes": (_sz, [_sz, _i]),
    "va_sliding_median_u8": (_i, [_vp, _i, _sz, _sz, _i, _i64, _vp, _vp, _vp, _vp, _vp]),
    "va_sliding_median_current": (_i, [_vp, _sz, _i, _i64, _vp, _vp, _vp]),
    "va_time_difference_u8": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "va_threshold_u8": (_i, [_vp, _vp, _sz, _i, _i, _vp]),
    "va_mono_mean_u8": (_i, [_vp, _vp, _sz, _vp]),
    "va_rot90": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "va_normalize_u8": (_i, [_vp, _vp, _sz, _d, _d, _d, _d, _vp]),
    "va_morph_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "va_label_workspace_bytes": (_sz, [_i, _i, _i]),
    "va_label_i32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _sz, _vp]),
    "va_moments_i64": (_i, [_vp, _i, _i, _i, _i, _vp, _vp]),
    "va_largest_region": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]),
    "va_detect_peaks_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "va_detect_peaks_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "va_image_statistics_f32": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _vp]),
    "va_mask_thinning_u8": (_i, [_vp, _vp, _vp, _i, _i, C.POINTER(_i), _vp]),
    "va_image_statistics_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _d, _i, _vp]),
    "va_contour_workspace_bytes": (_sz, [_i, _i, _i]),
    "va_largest_contour": (_i, [_vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "va_find_contours_workspace_bytes": (_sz, [_i, _i, _i]),
    "va_find_contours": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _sz, _vp]),
    "va_region_links_workspace_bytes": (_sz, [_i, _i, _i, _i64]),
    "va_region_links": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "va_template_match_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "va_template_match_u8": (_i, [C.POINTER(va_match_args)]),
    "va_normalize": (_i, [_vp, _i, _vp, _i, _sz, _d, _d, _d, _d, _vp]),
    "va_prepare_u8": (_i, [_vp, _vp] + [_i] * 10 + [_d, _d, _d, _d, _vp]),
    "va_gaussian_noise": (_i, [_vp, _i, _sz, _d, _d, C.c_uint64, C.c_uint64, _vp]),
    "va_resize_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "va_resize_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "va_contour_moments": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp]),
    "va_contour_moments_ragged": (_i, [_vp, _vp, _i64, _i, _vp, _vp]),
    "va_geodesic_workspace_bytes": (_sz, [_i, _i, _i]),
    "va_distance_map_i32": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "va_distance_map_path": (_i, [_vp, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "va_farthest_points": (_i, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _vp]),
    "va_farneback_poly_consts": (_i, [_i, _d, _vp, _vp, _vp, _vp]),
    "va_farneback_workspace_bytes": (_sz, [_i, _i, _i, _d, _i, _i, _i, _i]),
    "va_optical_flow_farneback": (_i, [_vp, _i, _i, _i, _i, _d, _i, _i, _i, _i, _d, _i, _vp, _vp, _vp, _sz, _vp]),
    "va_sobel5_f64": (_i, [_vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "va_active_contour": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _d, _d, _i, _vp,
                               _vp, _vp, _vp]),
    "va_potential_gradients_ragged": (_i, [_vp, _i, _vp, _vp, _i64, _i, _i, _d, _vp, _vp, _vp, _vp]),
    "va_active_contour_ragged": (_i, [_vp, _vp, _vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _d, _d,
                                      _i, _vp, _vp, _vp, _vp]),
    "va_fill_poly": (_i, [_vp, _vp, _i64, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "va_distance_transform_l2_5": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp]),
    "va_guo_hall_thinning_batch": (_i, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp]),
    "va_guo_hall_thinning_scratch_bytes": (_sz, [_i, _i, _i]),
    "va_guo_hall_thinning_u8": (_i, [_vp, _vp, _sz, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    "va_line_scan_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp]),
    "va_warp_affine_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp, _vp]),
    "va_skeleton_graph_workspace_bytes": (_sz, [_i64, _i]),
    "va_skeleton_graph": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _sz,
                               _vp]),
    "va_ray_hits": (_i, [_vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    "va_points_in_outlines": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _i64, _i, _vp, _vp]),
    "va_curves_equidistant": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "va_simplify_rdp": (_i, [_vp, _vp, _i64, _i, _vp, _vp, _vp, _vp, _vp]),
    "va_simplify_visvalingam_workspace_bytes": (_sz, [_i64]),
    "va_simplify_visvalingam": (_i, [_vp, _vp, _i64, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "va_compose_layers_u8": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    "va_draw_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp, _vp]),
    "va_draw_contours_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i64, _vp, _i64, _vp, _i, C.c_uint32, _vp, _vp]),
    "va_jpeg_encode_u8": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "va_jpeg_encode_sampled_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i64, _vp]),
    "va_jpeg_encode_optimized_u8": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _i64,
                                         _vp]),
    "va_jpeg_optimal_tables": (_i, [_vp, _i, _vp, _vp]),
    "va_jpeg_decode_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "va_jpeg_decode_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i64, _vp]),
    "va_jpeg_decode_sampled_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "va_jpeg_decode_sampled_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i64,
                                       _vp]),
    "va_jpeg_decode_split_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i, _i64]),
    "va_jpeg_decode_split_u8": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i64, _i, _i,
                                     _i64, _vp, _vp]),
    "va_pipeline_create": (_i, [C.POINTER(va_config), C.POINTER(_vp)]),
    "va_pipeline_destroy": (_i, [_vp]),
    "va_pipeline_run": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "va_pipeline_overlap": (_i, [_vp, _i]),
    "va_pipeline_fence": (_i, [_vp, _vp]),
    "va_bg_get_state": (_i, [_vp, _vp, _sz, C.POINTER(_i64)]),
    "va_bg_set_state": (_i, [_vp, _vp, _sz, _i64]),
    "va_bg_state_bytes": (_sz, [_vp]),
    "va_pipeline_describe": (C.c_char_p, [_vp]),
    "va_pipeline_profile": (_i, [_vp, _i]),
    "va_pipeline_stage_times": (_i, [_vp, _i, _vp, _vp, _vp, C.POINTER(_i)]),
    "va_gaussian_u8_generic": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _vp]),
    "va_gaussian_u8_valu": (_i, [_vp, _vp, _i, _i, _i, _i, _d, _vp]),
    "va_test_hook_labelling": (_i, [_i, _i]),
    "va_test_hook_gaussian_u8": (_i, [_i]),
    "va_test_hook_gaussian_f32": (_i, [_i]),
    "va_test_hook_fill": (_i, [_i]),
    "va_morph_bits_u8": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "va_comm_unique_id": (_i, [_vp]),
    "va_comm_init": (_i, [C.POINTER(_vp), _i, _i, _vp]),
    "va_gather_counts": (_i, [_vp, _vp, _vp, _i, _vp]),
    "va_comm_destroy": (_i, [_vp]),
}

_lib = None
_ready_device = None


def load_library():
    """dlopen the shared library and declare the prototypes (no GPU needed for this)"""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipUnavailableError(
                "%s is missing -- build it with `make -C video-analysis_amd/csrc` "
                "(or __graft_entry__.build()); there is no CPU fallback" % LIB_PATH)
        try:
            lib = C.CDLL(LIB_PATH)
        except OSError as e:
            raise HipUnavailableError("cannot load %s: %s" % (LIB_PATH, e))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def check(code):
    if code != 0:
        raise HipError(code, load_library().va_last_error().decode("utf-8", "replace"))


def lib(device=None):
    """library handle with an initialised GPU; raises HipUnavailableError without one.

    One device per process (one process per GPU, as bench.py / torch.distributed launch them): the
    first call selects `device` (default: $VA_DEVICE, else $LOCAL_RANK, else 0); asking for a
    device that is not visible, or for a second device later, raises instead of silently running
    somewhere else."""
    global _ready_device
    L = load_library()
    if _ready_device is None:
        if device is None:
            device = int(os.environ.get("VA_DEVICE", os.environ.get("LOCAL_RANK", "0")))
        count = L.va_device_count()
        if count <= 0:
            raise HipUnavailableError("no HIP device visible: the video filters/analysis ops "
                                      "run on MI355X only (no CPU fallback)")
        if not 0 <= device < count:
            raise HipUnavailableError("device %d requested but only %d GPU(s) are visible to this "
                                      "process (check LOCAL_RANK / VA_DEVICE / HIP_VISIBLE_DEVICES)"
                                      % (device, count))
        check(L.va_init(device))
        _ready_device = device
    elif device is not None and device != _ready_device:
        raise ValueError("this process already runs on GPU %d; device %d requested (the library "
                         "uses one device per process: start one process per GPU)"
                         % (_ready_device, device))
    return L


def gpu_available():
    try:
        return load_library().va_device_count() > 0
    except HipError:
        return False


# ------------------------------------------------------------------------------------------ test fill mode
# Undefined device memory that is not zero, and a guarded tail behind every buffer ("Hostile memory").
# -1 = off; 0..255 = on: every DeviceBuffer is allocated with TAIL_BYTES more than asked for and filled with the
# byte, and the library fills its own scratch and pipeline planes (va_test_hook_fill).  Initial value: $VA_TEST_FILL,
# which the library reads too.
TAIL_BYTES = 256


def _fill_from_env():
    text = os.environ.get("VA_TEST_FILL", "")
    return int(text) if text.isdigit() and int(text) <= 255 else -1


_fill_mode = _fill_from_env()
_fill_watchers = []             # video.ops mirrors the value in a global of its own: called with each new value
_guarded = weakref.WeakSet()    # every live DeviceBuffer made while the mode was on
_violations = []                # what free() found (__del__ swallows exceptions): drained by check_guards()


def fill_mode():
    """the fill byte of the test fill mode, or -1 when it is off"""
    return _fill_mode


def set_fill_mode(byte):
    """switch the test fill mode on (0..255) or off (-1), here and in the library where it has the hook (the
    oracle's twin has no scratch of its own and no hook)"""
    global _fill_mode
    byte = int(byte)
    if not -1 <= byte <= 255:
        raise ValueError("the fill byte is -1 (off) or 0..255, got %d" % byte)
    hook = getattr(load_library(), "va_test_hook_fill", None)
    if hook is not None:
        check(hook(byte))
    _fill_mode = byte
    for watcher in _fill_watchers:
        watcher(byte)


class GuardViolation(HipError):
    """bytes behind the end of a device buffer were overwritten (test fill mode)"""

    def __init__(self, message):
        HipError.__init__(self, -14, message)


def check_guards():
    """the guarded ranges of every live DeviceBuffer, checked now, and what free() has recorded since the last
    call: a list of messages, empty when nothing was written behind a buffer.  Each violation is reported once."""
    found, _violations[:] = list(_violations), []
    for buf in list(_guarded):
        damage = buf.check_guard()
        if damage:
            found.append(damage)
    return found


class DeviceBuffer(object):
    """a hipMalloc'ed buffer with NumPy upload/download helpers"""
    _fill = -1          # the byte this buffer and its tail were filled with; -1: made with the test fill mode off
    _alloc = 0          # (test fill mode) bytes allocated: nbytes + TAIL_BYTES
    _asked = 0          # (test fill mode) where the guarded range starts: nbytes, or what ops._take was asked for

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        self._ptr = C.c_void_p()
        if _fill_mode < 0:
            check(lib().va_malloc(C.byref(self._ptr), max(self.nbytes, 1)))
            return
        self._fill, self._asked, self._alloc = _fill_mode, self.nbytes, self.nbytes + TAIL_BYTES
        check(lib().va_malloc(C.byref(self._ptr), self._alloc))
        self.refill()
        _guarded.add(self)

    @property
    def ptr(self):
        return self._ptr.value

    @classmethod
    def from_array(cls, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        buf = cls(arr.nbytes)
        buf.upload(arr, stream)
        return buf

    def upload(self, arr, stream=None):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes > self.nbytes:
            raise ValueError("array of %d bytes does not fit buffer of %d" % (arr.nbytes, self.nbytes))
        L = lib()
        check(L.va_memcpy_h2d(self.ptr, arr.ctypes.data, arr.nbytes, stream))
        check(L.va_stream_sync(stream))     # pageable source: make the copy complete

    def download(self, shape, dtype, stream=None):
        out = np.empty(shape, dtype)
        if out.nbytes > self.nbytes:
            raise ValueError("download of %d bytes exceeds buffer of %d" % (out.nbytes, self.nbytes))
        L = lib()
        check(L.va_memcpy_d2h(out.ctypes.data, self.ptr, out.nbytes, stream))
        check(L.va_stream_sync(stream))
        return out

    def refill(self, start=0):
        """(test fill mode) set the allocation from byte `start` on, tail included, to the fill byte; synchronises"""
        L = lib()
        check(L.va_memset(self.ptr + start, self._fill, self._alloc - start, None))
        check(L.va_stream_sync(None))

    def check_guard(self):
        """(test fill mode) None when every byte behind the size asked for still holds the fill byte; else a message
        with the sizes, the first damaged offset and the number of damaged bytes, and the range is filled again (a
        violation is reported once).  Synchronises.  A write of the fill byte itself cannot be seen."""
        if _fill_mode < 0 or self._fill != _fill_mode or not self.ptr:      # (made with the mode off, or under another byte)
            return None
        tail = np.empty(self._alloc - self._asked, np.uint8)
        L = lib()
        check(L.va_memcpy_d2h(tail.ctypes.data, self.ptr + self._asked, tail.nbytes, None))
        check(L.va_stream_sync(None))
        bad = np.flatnonzero(tail != self._fill)
        if not bad.size:
            return None
        self.refill(self._asked)
        return ("buffer of %d bytes (%d allocated, fill 0x%02X): first damaged offset %d, %d byte(s) differ"
                % (self._asked, self._alloc, self._fill, self._asked + int(bad[0]), bad.size))

    def free(self):
        if self._ptr is not None and self._ptr.value:
            if _fill_mode >= 0:
                damage = self.check_guard()
                if damage:
                    _violations.append("at free(): " + damage)
            load_library().va_free(self._ptr)
            self._ptr = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def gauss_taps_q8(sigma, tap_rule="cv4"):
    """the unsigned 8.8 fixed-point taps used by FilterBlur on uint8 frames (host only); tap_rule
    'cv4' (OpenCV >= 4: error diffusion, sum 256) or 'cv3' (OpenCV 2.4 / 3.x: tap-by-tap rounding)"""
    buf = np.zeros(256, np.uint16)
    ks = C.c_int()
    check(load_library().va_gauss_taps_q8_rule(float(sigma), TAP_RULES[tap_rule], C.byref(ks), buf.ctypes.data, 256))
    return buf[:ks.value].copy()


def gauss_taps_f32(sigma):
    buf = np.zeros(256, np.float32)
    ks = C.c_int()
    check(load_library().va_gauss_taps_f32(float(sigma), C.byref(ks), buf.ctypes.data, 256))
    return buf[:ks.value].copy()


def farneback_poly_consts(poly_n, poly_sigma):
    """FarnebackPrepareGaussian (host only): g, xg, xxg (float32, offsets -poly_n..poly_n) and
    (ig11, ig03, ig33, ig55)"""
    k = 2 * int(poly_n) + 1 if int(poly_n) in (5, 7) else 15
    g, xg, xxg = (np.zeros(k, np.float32) for _ in range(3))
    ig = np.zeros(4, np.float64)
    check(load_library().va_farneback_poly_consts(int(poly_n), float(poly_sigma), g.ctypes.data, xg.ctypes.data,
                                                  xxg.ctypes.data, ig.ctypes.data))
    return g, xg, xxg, tuple(float(v) for v in ig)
