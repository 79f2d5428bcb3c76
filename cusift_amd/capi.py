"""ctypes binding of the C ABI declared in include/cusift_amd.h (libcusift_amd.so).

There is no CPU fallback: if the HIP extension is missing this module raises at import of the
library handle (`lib()`), and every call that needs a GPU fails with the library's error text.
"""
import collections
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CUSIFT_AMD_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libcusift_amd.so")

CUSIFT_OK = 0
NUM_STAGES = 8
STAGE_NAMES = ("scale_down", "laplace_multi", "find_points_multi", "compute_orientations",
               "extract_descriptors", "total", "detect_multi", "describe_all")
# flags of cusift_describe_batch
DESCRIBE_KEEP_ORIENTATION, DESCRIBE_OCTAVE_FROM_SCALE = 1, 2

# SiftPoint, cuSIFT.h:10-30 (588 B, no padding)
SIFT_POINT_DTYPE = np.dtype(
    [
        ("coords2D", "<f4", (2,)),
        ("scale", "<f4"),
        ("sharpness", "<f4"),
        ("edgeness", "<f4"),
        ("orientation", "<f4"),
        ("score", "<f4"),
        ("ambiguity", "<f4"),
        ("match", "<i4"),
        ("match_xpos", "<f4"),
        ("match_ypos", "<f4"),
        ("match_error", "<f4"),
        ("subsampling", "<f4"),
        ("empty", "<f4", (3,)),
        ("data", "<f4", (128,)),
        ("coords3D", "<f4", (3,)),
    ]
)
SIFT_POINT_BYTES = 588
assert SIFT_POINT_DTYPE.itemsize == SIFT_POINT_BYTES

# cusift_compact_point (include/cusift_amd.h): the optional 160-byte wire record
COMPACT_POINT_DTYPE = np.dtype([("coords2D", "<f4", (2,)), ("scale", "<f4"), ("sharpness", "<f4"), ("edgeness", "<f4"),
                                ("orientation", "<f4"), ("subsampling", "<f4"), ("desc_step", "<f4"), ("q", "u1", (128,))])
COMPACT_POINT_BYTES = 160
assert COMPACT_POINT_DTYPE.itemsize == COMPACT_POINT_BYTES

# cusift_trimmed_point: the 135 floats extraction writes, exact (optional 540-byte wire record)
TRIMMED_POINT_DTYPE = np.dtype([("coords2D", "<f4", (2,)), ("scale", "<f4"), ("sharpness", "<f4"), ("edgeness", "<f4"),
                                ("orientation", "<f4"), ("subsampling", "<f4"), ("data", "<f4", (128,))])
TRIMMED_POINT_BYTES = 540
assert TRIMMED_POINT_DTYPE.itemsize == TRIMMED_POINT_BYTES
# cusift_match_row (cusift_amd_extras.h): one row of cusift_match_batch
MATCH_ROW_DTYPE = np.dtype([("score", "<f4"), ("ambiguity", "<f4"), ("match", "<i4"), ("reserved", "<i4")])
MatchRow = MATCH_ROW_DTYPE
MATCH_ROW_BYTES = 16
assert MATCH_ROW_DTYPE.itemsize == MATCH_ROW_BYTES

WIRE_FORMATS = {"exact": (0, SIFT_POINT_BYTES), "compact": (1, COMPACT_POINT_BYTES), "trimmed": (2, TRIMMED_POINT_BYTES)}


class Params(C.Structure):
    """cusift_params (include/cusift_amd.h); the public parameter fields of SiftData, cuSIFT.h:44-51."""

    _fields_ = [
        ("num_octaves", C.c_int),
        ("init_blur", C.c_double),
        ("peak_thresh", C.c_float),
        ("edge_thresh", C.c_float),
        ("lowest_scale", C.c_float),
        ("subsampling", C.c_float),
        ("max_pts", C.c_int),
        ("tex_frac_bits", C.c_int),
        ("fused_detect", C.c_int),
        ("root_sift", C.c_int),
        ("concurrent_batches", C.c_int),
        ("upsample", C.c_int),
    ]


class Camera(C.Structure):
    """cusift_camera (include/cusift_amd_extras.h): pinhole intrinsics and the encoding of a 16-bit depth image.
    origin 1 = MATLAB 1-based cx / cy; encoding 1 = SUN3D PNG samples (the depth rotated left by 3 bits)."""

    _fields_ = [
        ("fx", C.c_float),
        ("fy", C.c_float),
        ("cx", C.c_float),
        ("cy", C.c_float),
        ("origin", C.c_float),
        ("units_per_metre", C.c_float),
        ("encoding", C.c_int),
    ]

    def __init__(self, fx, fy, cx, cy, origin=0.0, units_per_metre=1000.0, encoding=0):
        super().__init__(fx, fy, cx, cy, origin, units_per_metre, encoding)


class BundleParams(C.Structure):
    """cusift_bundle_params (include/cusift_amd_extras.h): the Levenberg-Marquardt settings of cusift_bundle_adjust.
    Fields left out take cusift_bundle_default_params' values (iterations 10, lambda 1e-3, lambda_min 1e-9, lambda_max
    1e6, huber 0 = squared error, max_error 0 = no entry gate, min_decrease 1e-12)."""

    _fields_ = [
        ("iterations", C.c_int),
        ("lambda_", C.c_double),
        ("lambda_min", C.c_double),
        ("lambda_max", C.c_double),
        ("huber", C.c_double),
        ("max_error", C.c_double),
        ("min_decrease", C.c_double),
    ]

    def __init__(self, **fields):
        super().__init__()
        lib().cusift_bundle_default_params(C.byref(self))
        for k, v in fields.items():
            k = "lambda_" if k in ("lambda", "lam") else k
            if k not in [name for name, _ in self._fields_]:
                raise TypeError("unknown bundle parameter %r" % k)
            setattr(self, k, v)


class CusiftError(RuntimeError):
    pass


# name -> (restype, argtypes); every symbol include/cusift_amd.h declares
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_PP = C.POINTER(Params)
SIGNATURES = {
    "cusift_last_error": (C.c_char_p, []),
    "cusift_version": (C.c_char_p, []),
    "cusift_device_count": (_i, [C.POINTER(_i)]),
    "cusift_init": (_i, [_i]),
    "cusift_default_params": (None, [_PP]),
    "cusift_ctx_create": (_i, [C.POINTER(_vp), _i, _vp]),
    "cusift_ctx_create_borrowed": (_i, [C.POINTER(_vp), _i, _vp]),
    "cusift_ctx_destroy": (_i, [_vp]),
    "cusift_ctx_synchronize": (_i, [_vp]),
    "cusift_ctx_stream": (_vp, [_vp]),
    "cusift_ctx_device": (_i, [_vp]),
    "cusift_ctx_wait": (_i, [_vp, _vp]),
    "cusift_comm_get_unique_id": (_i, [_vp]),
    "cusift_comm_create": (_i, [C.POINTER(_vp), _vp, _vp, _i, _i]),
    "cusift_comm_destroy": (_i, [_vp]),
    "cusift_comm_rank": (_i, [_vp, C.POINTER(_i), C.POINTER(_i)]),
    "cusift_comm_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "cusift_expand_gathered": (_i, [_vp, _vp, _sz, _vp, _vp]),
    "cusift_comm_library": (C.c_char_p, []),
    "cusift_comm_set_self_p2p": (_i, [_vp, _i]),
    "cusift_comm_use_library": (_i, [C.c_char_p]),
    "cusift_comm_ctx": (_vp, [_vp]),
    "cusift_comm_reserve": (_i, [_vp, _i, _i, _sz]),
    "cusift_comm_set_fixed_size": (_i, [_vp, _i]),
    "cusift_comm_set_wire_format": (_i, [_vp, _i]),
    "cusift_comm_host_waits": (C.c_ulonglong, [_vp]),
    "cusift_comm_host_wait_ms": (C.c_double, [_vp]),
    "cusift_comm_hip_syncs": (C.c_ulonglong, [_vp]),
    "cusift_allgatherv_begin": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz]),
    "cusift_allgatherv_finish": (_i, [_vp, _vp, _vp]),
    "cusift_allgatherv": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _sz, _vp, _vp]),
    "cusift_compact_gathered": (_i, [_vp, _vp, _sz, _i, _vp, _vp, _sz]),
    "cusift_tiled_plan": (_i, [_i, _i, _i, _i, _i, _i, _i] + [C.POINTER(_i)] * 9),
    "cusift_tiled_create": (_i, [C.POINTER(_vp), _vp, _vp, _i, _i, _i, _i, _PP, _i]),
    "cusift_tiled_destroy": (_i, [_vp]),
    "cusift_tiled_info": (_i, [_vp] + [C.POINTER(_i)] * 4),
    "cusift_tiled_band": (_i, [_vp, _i, C.POINTER(_vp)] + [C.POINTER(_i)] * 7),
    "cusift_tiled_load": (_i, [_vp, _vp, _i]),
    "cusift_tiled_build_octave": (_i, [_vp, _i]),
    "cusift_tiled_exchange": (_i, [_vp, _i]),
    "cusift_tiled_exchange_virtual": (_i, [C.POINTER(_vp), _i, _i]),
    "cusift_tiled_process": (_i, [_vp, _vp, _vp]),
    "cusift_tiled_extract": (_i, [_vp, _vp, _i, _vp, _vp]),
    "cusift_tiled_check": (_i, [_vp, C.POINTER(C.c_uint)]),
    "cusift_exchange_rows": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "cusift_exchange_halos": (_i, [_vp, _vp, _i, _i, _i, _i, _i]),
    "cusift_ctx_reserve": (_i, [_vp, _i, _i, _i, _PP]),
    "cusift_ctx_reserve_bands": (_i, [_vp, _i, _i]),
    "cusift_event_create": (_i, [_vp, C.POINTER(_vp)]),
    "cusift_event_record": (_i, [_vp, _vp]),
    "cusift_event_wait": (_i, [_vp, _vp]),
    "cusift_event_elapsed_ms": (_i, [_vp, _vp, C.POINTER(C.c_float)]),
    "cusift_event_destroy": (_i, [_vp]),
    "cusift_pipe_create": (_i, [C.POINTER(_vp), _i, _i, _i, _i, _PP, _i, _i, _sz]),
    "cusift_pipe_submit": (_i, [_vp, _vp, _i]),
    "cusift_pipe_collect": (_i, [_vp, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(_sz)]),
    "cusift_pipe_in_flight": (_i, [_vp]),
    "cusift_pipe_destroy": (_i, [_vp]),
    "cusift_ctx_set_policy": (_i, [_vp, _i, _i]),
    "cusift_ctx_set_keep_strongest": (_i, [_vp, _i]),
    "cusift_ctx_set_second_orientation": (_i, [_vp, C.c_float]),
    "cusift_ctx_set_cross_check": (_i, [_vp, _i]),
    "cusift_ctx_set_match_bits": (_i, [_vp, _i]),
    "cusift_ctx_get_policy": (_i, [_vp, _i, C.POINTER(C.c_int)]),
    "cusift_ctx_arena_bytes": (_sz, [_vp]),
    "cusift_ctx_forks": (C.c_ulong, [_vp]),
    "cusift_ctx_timing_enable": (_i, [_vp, _i]),
    "cusift_ctx_timing_read": (_i, [_vp, C.POINTER(_f), C.POINTER(_i)]),
    "cusift_ctx_timing_reset": (_i, [_vp]),
    "cusift_kernel_occupancy": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_i)]),
    "cusift_malloc": (_i, [C.POINTER(_vp), _sz]),
    "cusift_free": (_i, [_vp]),
    "cusift_memset": (_i, [_vp, _vp, _i, _sz]),
    "cusift_memcpy_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "cusift_memcpy_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "cusift_memcpy_d2d": (_i, [_vp, _vp, _vp, _sz]),
    "cusift_image_h2d": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "cusift_image_d2h": (_i, [_vp, _vp, _vp, _i, _i, _i]),
    "cusift_malloc_host": (_i, [C.POINTER(_vp), _sz]),
    "cusift_free_host": (_i, [_vp]),
    "cusift_image_u8_h2d": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "cusift_u8_to_f32": (_i, [_vp, _vp, _i, _sz, _vp, _i, _i, _i, _sz, _i]),
    "cusift_gaussian3x3": (_i, [_vp, _vp, _i, _sz, _vp, _i, _i, _i, _sz, _i, _f]),
    "cusift_scale_down": (_i, [_vp, _vp, _i, _sz, _vp, _i, _i, _i, _sz, _i, _f]),
    "cusift_scale_up": (_i, [_vp, _vp, _i, _sz, _vp, _i, _i, _i, _sz, _i]),
    "cusift_scale_down_levels": (_i, [_vp, _vp, _i, _i, _i, _sz, _vp, _vp, _vp, _i, _i, _f]),
    "cusift_extract_bands": (_i, [_vp, _vp, _i, _f, _f, _vp, _i, _vp, _i, _i, _vp]),
    "cusift_laplace_multi": (_i, [_vp, _vp, _i, _i, _i, _sz, _f, _vp, _sz, _i]),
    "cusift_laplace_taps": (_i, [_f, _vp]),
    "cusift_find_points_multi": (_i, [_vp, _vp, _i, _i, _i, _sz, _f, _f, _f, _vp, _i, _vp, _i]),
    "cusift_detect_multi": (_i, [_vp, _vp, _i, _i, _i, _sz, _f, _f, _f, _f, _vp, _i, _vp, _i]),
    "cusift_detect_multi_down": (_i, [_vp, _vp, _i, _i, _i, _sz, _f, _f, _f, _f, _vp, _i, _vp, _i, _vp, _i, _sz, _f]),
    "cusift_compute_orientations": (_i, [_vp, _vp, _i, _i, _i, _sz, _vp, _i, _vp, _vp, _i, _i]),
    "cusift_extract_descriptors": (_i, [_vp, _vp, _i, _i, _i, _sz, _vp, _i, _vp, _vp, _f, _i, _i]),
    "cusift_rootsift": (_i, [_vp, _vp, _i]),
    "cusift_math_eval": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _sz]),
    "cusift_scale_down_band": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _i, _i, _i, _i, _i, _f]),
    "cusift_detect_band": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _vp, _i, _vp]),
    "cusift_describe_band": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp, _i, _vp, _vp, _f, _i, _i, _vp]),
    "cusift_match": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "cusift_match_mutual": (_i, [_vp, _vp, _i, _vp, _i, _i]),
    "cusift_match_guided": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _f]),
    "cusift_match_projected": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, C.POINTER(Camera), _f]),
    "cusift_memcpy2d_d2h": (_i, [_vp, _vp, _sz, _vp, _sz, _sz, _sz]),
    "cusift_find_homography": (_i, [_vp, _vp, _i, _vp, _i, _f, _vp, C.POINTER(_i), _vp, _vp]),
    "cusift_estimate_homography": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, _vp, _vp, C.POINTER(_i),
                                        C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_register_planar": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, _vp, _vp,
                                    C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_estimate_fundamental": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, _vp, _vp, C.POINTER(_i),
                                         C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_register_epipolar": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, _vp, _vp,
                                      C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_estimate_pose": (_i, [_vp, _vp, _i, _i, _i, _f, _f, _vp, _f, C.POINTER(Camera), C.POINTER(Camera), _vp,
                                  C.POINTER(_i), _vp, _vp]),
    "cusift_register_pose": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, C.POINTER(Camera),
                                  C.POINTER(Camera), _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i),
                                  _vp, _vp, _vp, _vp, _vp, C.POINTER(_i), _vp, _vp]),
    "cusift_estimate_pnp": (_i, [_vp, _vp, _i, _i, _i, _f, _f, C.POINTER(Camera), _i, _f, _i, _f, C.c_uint64, _vp, _vp,
                                 C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_register_pnp": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _f, _f, C.POINTER(Camera), _i, _f, _i, _f, C.c_uint64,
                                 _vp, _vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i), _vp, _vp, _vp, _vp]),
    "cusift_estimate_rigid": (_i, [_vp, _vp, _i, _vp, _i, _f, _i, C.c_uint64, _vp, C.POINTER(_i), C.POINTER(_i), _vp, _vp,
                                   _vp, _vp]),
    "cusift_lift_depth": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _sz, C.POINTER(Camera)]),
    "cusift_select_matches": (_i, [_vp, _vp, _i, _vp, _i, _f, _f, _i, _vp, _vp, _vp]),
    "cusift_select_mutual": (_i, [_vp, _vp, _i, _vp, _i, _f, _f, _i, _vp, _vp, _vp]),
    "cusift_select_strongest": (_i, [_vp, _vp, _i, _i, _i, _vp, _i, _vp]),
    "cusift_register_rgbd": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, C.POINTER(Camera), _i, _f, _f, _i, _f, _i,
                                  C.c_uint64, _vp, C.POINTER(_i), C.POINTER(_i), _vp, _vp]),
    "cusift_match_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "cusift_match_batch_mutual": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "cusift_match_batch_guided": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _f, _vp]),
    "cusift_match_batch_projected": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, C.POINTER(Camera), _f, _vp]),
    "cusift_quantize_descriptors": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cusift_desc8_sums": (_i, [_vp, _vp, _i, _vp]),
    "cusift_match8": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i]),
    "cusift_match8_batch": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "cusift_match8_mutual": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i]),
    "cusift_match8_batch_mutual": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp]),
    "cusift_match8_guided": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _f]),
    "cusift_match8_projected": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, C.POINTER(Camera), _f]),
    "cusift_match8_batch_guided": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _vp, _f, _vp]),
    "cusift_match8_batch_projected": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, C.POINTER(Camera), _f, _vp]),
    "cusift_match8_guided_records": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _f]),
    "cusift_match8_projected_records": (_i, [_vp, _vp, _i, _vp, _i, _i, _vp, C.POINTER(Camera), _f]),
    "cusift_register_rgbd_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _sz, C.POINTER(Camera), _vp, _i, _i, _f,
                                        _f, _i, _f, _i, C.c_uint64, _vp, _vp, _vp, _vp, _vp]),
    "cusift_register_planar_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64, _vp,
                                          _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cusift_register_epipolar_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cusift_register_pose_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, _i, _f, _i, _f, C.c_uint64,
                                        C.POINTER(Camera), C.POINTER(Camera), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                        _vp, _vp, _vp, _vp, _vp]),
    "cusift_register_pnp_batch": (_i, [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _i, _f, _f, C.POINTER(Camera), _i, _f, _i, _f,
                                       C.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cusift_pack_points": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "cusift_pack_points_compact": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "cusift_pack_points_trimmed": (_i, [_vp, _vp, _vp, _i, _i, _vp, _sz, _vp]),
    "cusift_expand_trimmed": (_i, [_vp, _vp, _sz, _vp]),
    "cusift_expand_trimmed_host": (_i, [_vp, _sz, _vp]),
    "cusift_expand_points_host": (_i, [_vp, _sz, _vp]),
    "cusift_sort_points_host": (_i, [_vp, _i]),
    "cusift_extract_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _PP, _vp, _vp]),
    "cusift_describe_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _PP, _vp, _vp, C.c_uint]),
    "cusift_second_orientations_batch": (_i, [_vp, _vp, _i, _i, _i, _i, _sz, _PP, _vp, _vp, C.c_float, C.c_uint]),
    "cusift_build_tracks": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _i, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "cusift_triangulate_tracks": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, C.POINTER(Camera), C.c_double, _vp,
                                       _vp]),
    "cusift_bundle_default_params": (None, [C.POINTER(BundleParams)]),
    "cusift_bundle_adjust": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp, C.POINTER(Camera),
                                  C.POINTER(BundleParams), _vp, _vp, _vp, _vp]),
    "cusift_graph_create": (_i, [_vp, C.POINTER(_vp), _vp, _i, _i, _i, _i, _sz, _PP, _vp, _vp]),
    "cusift_graph_launch": (_i, [_vp]),
    "cusift_graph_nodes": (_i, [_vp]),
    "cusift_graph_destroy": (_i, [_vp]),
    "cusift_extract": (_i, [_vp, _vp, _i, _i, _i, _PP, _vp, _vp, C.POINTER(_i)]),
    "cusift_extract_host": (_i, [_vp, _vp, _i, _i, _PP, _vp, _vp, C.POINTER(_i)]),
}

_lib = None


def _prefer_torch_hip_runtime():
    """A process can hold ONE libamdhip64.so.7.  libcusift_amd.so asks for it by soname and would pull in the system
    ROCm's; a PyTorch-ROCm wheel ships its own copy (plus matching HSA / comgr libraries) and stops seeing the GPU if
    it is imported after a different one was loaded (torch.cuda.is_available() == False).  So when torch is installed
    but not imported yet, its copy is loaded first -- the combination every torch-first program (bench.py,
    cusift_amd.batch) runs with anyway.  Without torch the system runtime is used."""
    import importlib.util
    import sys

    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass  # fall back to the system runtime


def lib():
    """The loaded libcusift_amd.so with typed entry points. Raises if the extension is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CusiftError(
                "HIP extension %s is missing: run `python -m cusift_amd.build` (needs hipcc); "
                "there is no CPU fallback for the extraction path" % LIB_PATH
            )
        _prefer_torch_hip_runtime()
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library does not export the symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != CUSIFT_OK:
        msg = lib().cusift_last_error()
        raise CusiftError("cusift error %d: %s" % (rc, msg.decode() if msg else "?"))


def default_params(**overrides):
    p = Params()
    lib().cusift_default_params(C.byref(p))
    for k, v in overrides.items():
        if not hasattr(p, k):
            raise TypeError("unknown parameter %r" % k)
        setattr(p, k, v)
    return p


def device_count():
    n = C.c_int(0)
    check(lib().cusift_device_count(C.byref(n)))
    return n.value


def ialign_up(a, b):
    """iAlignUp, cutils.h:17"""
    return (a - a % b + b) if (a % b != 0) else a


# cusift_ctx_set_policy keys (include/cusift_amd.h)
POLICY_SIDE_STREAM, POLICY_OCTAVE_LISTS, POLICY_GENERIC_KERNELS, POLICY_LAUNCH_PER_OCTAVE, POLICY_MATCH_SPLITS, \
    POLICY_TILED_PER_OCTAVE, POLICY_PYRAMID_IN_DETECT = range(7)


PLANAR_RULES = {"dot": 0, "l2": 1}  # the candidate rule of cusift_estimate_homography, by the distance it is meant for
# what cusift_estimate_homography / cusift_register_planar return: homography (refined, [9]), ransac (the winner, [9]),
# the counts, the winner's flags bool [num_pts] and, with want_all, drawn [4, L], all_homographies [8, L], all_counts [L]
PlanarResult = collections.namedtuple("PlanarResult", "homography ransac num_candidates num_matches num_fit best_loop "
                                      "inliers drawn all_homographies all_counts")
# what cusift_register_planar_batch returns, one entry per pair: homography float32 [P, 9], ransac [P, 9], int32 [P]
# counts, counts = the records of each pair's first frame (as the device read them), and -- when asked for -- lists of
# P bool [count] inlier flags and P float32 [count] match errors (NaN where a pair has no fit: nothing was evaluated)
PlanarBatchResult = collections.namedtuple("PlanarBatchResult", "homography ransac num_candidates num_matches num_fit "
                                           "best_loop counts inliers match_error")
# what cusift_estimate_fundamental / cusift_register_epipolar return: fundamental (refined, float64 [9], row-major, x2^T F
# x1 = 0), ransac (the winner, [9]), the counts, the winner's flags bool [num_pts] and, with want_all, drawn [8, L],
# all_fundamentals float64 [9, L], all_counts [L]
EpipolarResult = collections.namedtuple("EpipolarResult", "fundamental ransac num_candidates num_matches num_fit best_loop "
                                        "inliers drawn all_fundamentals all_counts")
# what cusift_estimate_pose returns: rt float64 [3, 4] = [R | t] with X1 = R X2 + t and |t| = 1, num_front (the winner's
# vote), votes int32 [4] (the four candidates'), sigma float64 [3] (the singular values of E)
PoseResult = collections.namedtuple("PoseResult", "rt num_front votes sigma")
# what cusift_estimate_pnp / cusift_register_pnp return: rt (refined, float64 [3, 4], X1 = R X2 + t in the unit of
# coords3D), ransac (the winner), the counts, inliers bool [N]; with want_all drawn [6, L], all_rt float64 [12, L],
# all_counts [L]
PnPResult = collections.namedtuple("PnPResult", "rt ransac num_candidates num_matches num_fit best_loop inliers drawn "
                                   "all_rt all_counts")
# what cusift_register_pose returns: the EpipolarResult, then the PoseResult
RegisterPoseResult = collections.namedtuple("RegisterPoseResult", EpipolarResult._fields + PoseResult._fields)
# what the pair-list forms return, one entry per pair, as PlanarBatchResult relates to PlanarResult: the models float64
# [P, 9] (F) or [P, 3, 4] (poses), int32 [P] counts, counts = the records of each pair's first frame (as the device read
# them), lists of P bool [count] inlier flags and P float32 [count] match errors (NaN where a pair has no fit); the pose
# form adds rt [P, 3, 4] with |t| = 1, num_front [P], votes [P, 4], sigma [P, 3] and a list of P float32 [count, 3]
# triangulated points (what register_pose writes into coords3D)
EpipolarBatchResult = collections.namedtuple("EpipolarBatchResult", "fundamental ransac num_candidates num_matches "
                                             "num_fit best_loop counts inliers match_error")
PoseBatchResult = collections.namedtuple("PoseBatchResult", EpipolarBatchResult._fields +
                                         ("rt", "num_front", "votes", "sigma", "points3d"))
PnPBatchResult = collections.namedtuple("PnPBatchResult", "rt ransac num_candidates num_matches num_fit best_loop counts "
                                        "inliers match_error")
RIGID_KINDS = {"2d": 0, "3d": 1}  # RigidTransformType2D / RigidTransformType3D, extras/rigidTransform.h:16-19


def _rule_defaults(distance, rule, lo, hi):
    """(rule, lo, hi) of a fused call: where None, the rule that fits the distance (1 = L2: rule 1 with lo = 999, hi = 0.8
    as score / ambiguity thresholds; 0 = dot product: rule 0 with lo = 0, hi = 0.8)."""
    rule = (1 if distance == 1 else 0) if rule is None else PLANAR_RULES.get(rule, rule)
    return rule, (999.0 if rule == 1 else 0.0) if lo is None else lo, 0.8 if hi is None else hi


def _seed64(seed):
    """Any Python int as the uint64_t seed of the C ABI."""
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def check_rigid_args(coord, indices=None, loops=None, thresh2=0.0025, kind="3d"):
    """What Context.estimate_rigid checks before it calls the library (needs no device): returns (coord float32 [N, 6],
    indices int32 [L, 3] or None, L, type).  ValueError for anything cusift_estimate_rigid would refuse."""
    if kind not in RIGID_KINDS:
        raise ValueError("kind must be '2d' or '3d', not %r" % (kind,))
    coord = np.asarray(coord)
    if coord.dtype != np.float32:
        raise ValueError("coord must be float32, not %s" % coord.dtype)
    if coord.ndim != 2 or coord.shape[1] != 6:
        raise ValueError("coord must be [num_pts, 6] (reference xyz, moving xyz), not %s" % (coord.shape,))
    coord = np.ascontiguousarray(coord)
    num_pts = coord.shape[0]
    if not (float(thresh2) > 0.0):
        raise ValueError("thresh2 must be > 0")
    used = 3 if kind == "3d" else 2
    if indices is None:
        if loops is None or int(loops) < 1:
            raise ValueError("without indices, loops >= 1 says how many hypotheses to draw")
        if num_pts < 3:
            raise ValueError("drawing needs num_pts >= 3, got %d" % num_pts)
        return coord, None, int(loops), RIGID_KINDS[kind]
    indices = np.asarray(indices)
    if indices.dtype != np.int32:
        raise ValueError("indices must be int32, not %s" % indices.dtype)
    if indices.ndim != 2 or indices.shape[1] != 3 or indices.shape[0] < 1:
        raise ValueError("indices must be [num_loops >= 1, 3], not %s" % (indices.shape,))
    if loops is not None and int(loops) != indices.shape[0]:
        raise ValueError("loops = %d but indices has %d rows" % (int(loops), indices.shape[0]))
    if num_pts < used:
        raise ValueError("the %s estimate needs num_pts >= %d, got %d" % (kind, used, num_pts))
    read = indices[:, :used]
    if read.min() < 0 or read.max() >= num_pts:
        raise ValueError("sample index out of range [0, %d)" % num_pts)
    return coord, np.ascontiguousarray(indices), indices.shape[0], RIGID_KINDS[kind]


def check_scale_up_args(d_dst, dst_pitch, d_src, w, h, src_pitch, n_images=1, dst_stride=None, src_stride=None):
    """What Context.scale_up checks before it calls the library (needs no device): returns (dst_stride, src_stride) in
    floats.  ValueError for anything cusift_scale_up would refuse."""
    if not d_dst or not d_src:
        raise ValueError("scale_up: missing data")
    w, h, n_images = int(w), int(h), int(n_images)
    if n_images < 1 or n_images > 65535 or w < 1 or h < 1 or int(src_pitch) < w or w > (1 << 27) or h > 4 * 65535:
        raise ValueError("scale_up: bad geometry n=%d w=%d h=%d pitch=%d" % (n_images, w, h, src_pitch))
    if int(dst_pitch) < 2 * w:
        raise ValueError("scale_up: dst_pitch %d < 2 w = %d" % (dst_pitch, 2 * w))
    dst_stride = 2 * h * int(dst_pitch) if dst_stride is None else int(dst_stride)
    src_stride = h * int(src_pitch) if src_stride is None else int(src_stride)
    if n_images > 1 and (src_stride < h * int(src_pitch) or dst_stride < 2 * h * int(dst_pitch)):
        raise ValueError("scale_up: image stride too small")
    return dst_stride, src_stride


def check_cross_check(on):
    """What Context.set_cross_check checks before it calls the library (needs no device): returns 0 or 1.  ValueError
    for anything but a bool, 0 or 1."""
    if not isinstance(on, (bool, int, np.integer)) or on not in (0, 1):
        raise ValueError("cross_check: False / True (0 / 1), got %r" % (on,))
    return int(on)


def check_match_bits(bits):
    """What Context.set_match_bits checks before it calls the library (needs no device): returns 32 or 8.  ValueError
    for anything but the integers 32 and 8."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or bits not in (32, 8):
        raise ValueError("match_bits: 32 or 8, got %r" % (bits,))
    return int(bits)


def check_keep_strongest(k, max_pts=None):
    """What Context.set_keep_strongest checks before it calls the library (needs no device): returns K as an int.
    ValueError for K < 0, a K that is no integer, or (max_pts given) K > max_pts, which the next extraction would refuse."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
        raise ValueError("keep_strongest: K must be an integer, got %r" % (k,))
    if k < 0 or k > 0x7fffffff:
        raise ValueError("keep_strongest: K must be >= 0 (0 = off), got %d" % k)
    if max_pts is not None and k > max_pts:
        raise ValueError("keep_strongest: K = %d exceeds max_pts = %d" % (k, max_pts))
    return int(k)


def check_second_orientation(ratio, allow_off=True):
    """What Context.set_second_orientation (and, with allow_off=False, Context.second_orientations) checks before it calls
    the library (needs no device): returns the ratio as a float.  ValueError for a ratio that is no real number, is
    negative, above 1 or not a number -- and for 0, which turns the setting off, where the stage call is meant."""
    if isinstance(ratio, bool) or not isinstance(ratio, (int, float, np.integer, np.floating)):
        raise ValueError("second_orientation: the ratio must be a number, got %r" % (ratio,))
    r = float(np.float32(ratio))
    if r == 0.0 and allow_off:
        return 0.0
    if not (0.0 < r <= 1.0):  # a NaN fails both comparisons
        raise ValueError("second_orientation: the ratio must %slie in (0, 1], got %r"
                         % ("be 0 (off) or " if allow_off else "", ratio))
    return r


def check_select_strongest_args(d_heads, n_lists, n_images, capacity, d_counts, keep, d_kept):
    """What Context.select_strongest checks before it calls the library (needs no device).  ValueError for anything
    cusift_select_strongest would refuse."""
    if not d_heads or not d_counts or not d_kept:
        raise ValueError("select_strongest: missing data")
    if not (1 <= n_lists <= 16 and 1 <= n_images <= 65535 and capacity >= 1):
        raise ValueError("select_strongest: bad geometry lists=%d (1..16) images=%d (1..65535) capacity=%d"
                         % (n_lists, n_images, capacity))
    if keep < 1 or keep > 0x7fffffff:
        raise ValueError("select_strongest: keep must be >= 1, got %d" % keep)
    if n_lists * capacity > 0x7fffffff or n_images * n_lists * capacity > 1 << 32:
        raise ValueError("select_strongest: %d lists x %d images x %d heads are too many" % (n_lists, n_images, capacity))


GUIDE_MODELS = {"homography": 0, "epipolar": 1}  # CUSIFT_GUIDE_HOMOGRAPHY / CUSIFT_GUIDE_EPIPOLAR


def guide_models(model, m, n_models=None):
    """(model as the C ABI's int, the matrices as contiguous float64 [n, 9]) of a guided match: `model` is
    "homography" / "epipolar" or 0 / 1 (anything else is handed through for the library to refuse), `m` one 3 x 3 or
    9-vector -- or n_models of them -- of any float type (register_planar's float32 H is widened)."""
    m = np.ascontiguousarray(m, dtype=np.float64).reshape(-1, 9)
    if len(m) != (1 if n_models is None else n_models):
        raise ValueError("guided match: %d models for %d pairs" % (len(m), 1 if n_models is None else n_models))
    return GUIDE_MODELS.get(model, model), m


def pose_models(rt, n_models=None):
    """The poses of a projected match as contiguous float64 [n, 12]: one 3 x 4 or 12-vector [R | t] -- or n_models of
    them -- of any float type."""
    rt = np.ascontiguousarray(rt, dtype=np.float64).reshape(-1, 12)
    if len(rt) != (1 if n_models is None else n_models):
        raise ValueError("projected match: %d poses for %d pairs" % (len(rt), 1 if n_models is None else n_models))
    return rt


def pair_list(pairs):
    """A pair list as the C ABI takes it: contiguous int32 [P, 2] of (frame 1, frame 2)."""
    pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    return pairs


def chain_poses(rts, pairs=None):
    """Poses of the frames of a sequence in frame 0's coordinates, float64 [n_images, 4, 4], from the transforms of
    consecutive pairs: rts[i] = [R | t] with x_i ~ R x_{i+1} + t (what register_rgbd_batch returns for pair (i, i + 1)),
    so pose[0] = I and pose[i + 1] = pose[i] @ [[R, t], [0, 1]].  pairs (optional) must be (0, 1), (1, 2), ...:
    anything else is a ValueError -- composing a graph of loop closures is a pose-graph problem, not this helper's."""
    rts = np.asarray(rts, dtype=np.float64).reshape(-1, 3, 4)
    if pairs is not None:
        pairs = np.asarray(pairs).reshape(-1, 2)
        want = np.stack([np.arange(len(rts)), np.arange(len(rts)) + 1], axis=1)
        if pairs.shape != want.shape or not np.array_equal(pairs, want):
            raise ValueError("chain_poses composes consecutive pairs (i, i + 1) only")
    poses = np.zeros((len(rts) + 1, 4, 4), dtype=np.float64)
    poses[0] = np.eye(4)
    for i, rt in enumerate(rts):
        step = np.eye(4)
        step[:3, :] = rt
        poses[i + 1] = poses[i] @ step
    return poses


def track_poses(poses, n_images):
    """Per-frame poses as cusift_triangulate_tracks takes them: contiguous float64 [n_images, 12], the row-major
    [R | t] of every frame -- from chain_poses' [n, 4, 4] (its top three rows) or from [n, 3, 4]."""
    poses = np.asarray(poses, dtype=np.float64)
    if poses.ndim == 3 and poses.shape[1:] == (4, 4):
        poses = poses[:, :3, :]
    if poses.size != 12 * n_images:
        raise ValueError("triangulate_tracks: %d pose entries for %d frames" % (poses.size, n_images))
    return np.ascontiguousarray(poses).reshape(n_images, 12)


def chain_homographies(h, pairs=None):
    """Homographies of the frames of a sequence into frame 0, float64 [n_images, 3, 3], from those of consecutive pairs:
    h[k] maps frame k onto frame k + 1 (what register_planar_batch returns for pair (k, k + 1)), so G[0] = I and
    G[k + 1] = G[k] @ inv(h[k]), each normalised by its [2, 2].  pairs (optional) must be (0, 1), (1, 2), ...: anything
    else is a ValueError, as for chain_poses."""
    h = np.asarray(h, dtype=np.float64).reshape(-1, 3, 3)
    if pairs is not None:
        pairs = np.asarray(pairs).reshape(-1, 2)
        want = np.stack([np.arange(len(h)), np.arange(len(h)) + 1], axis=1)
        if pairs.shape != want.shape or not np.array_equal(pairs, want):
            raise ValueError("chain_homographies composes consecutive pairs (i, i + 1) only")
    chain = np.zeros((len(h) + 1, 3, 3), dtype=np.float64)
    chain[0] = np.eye(3)
    for k, step in enumerate(h):
        g = chain[k] @ np.linalg.inv(step)
        chain[k + 1] = g / g[2, 2]
    return chain


class Context:
    """cusift_ctx: one device + one HIP stream + the scratch arena."""

    def __init__(self, device=0, stream=None):
        """stream=None: the context creates its own stream.  stream=<int handle>: borrow that hipStream_t;
        0 is the device's null stream (torch.cuda.current_stream().cuda_stream is 0 for the default stream)."""
        self._h = C.c_void_p()
        if stream is None:
            check(lib().cusift_ctx_create(C.byref(self._h), device, None))
        else:
            check(lib().cusift_ctx_create_borrowed(C.byref(self._h), device, C.c_void_p(int(stream))))
        self.device = device
        self.cross_check = False  # what set_cross_check last set: the guided chains refuse to run while it is on
        self.match_bits = 32  # what set_match_bits last set: at 8 the guided chains ask for match8=True

    @property
    def handle(self):
        if not self._h:
            raise CusiftError("context already destroyed")
        return self._h

    def close(self):
        if self._h:
            lib().cusift_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        check(lib().cusift_ctx_synchronize(self.handle))

    def stream_handle(self):
        """The hipStream_t of the context as an integer (0 = the null stream): torch.cuda.ExternalStream(...) of it puts
        torch-side work on the stream the kernels run on."""
        return int(lib().cusift_ctx_stream(self.handle) or 0)

    def wait(self, other):
        """cusift_ctx_wait: work enqueued on this context from now on waits for what `other` has enqueued so far."""
        check(lib().cusift_ctx_wait(self.handle, other.handle))

    def reserve(self, n_images, w, h, params):
        check(lib().cusift_ctx_reserve(self.handle, n_images, w, h, C.byref(params)))

    def arena_bytes(self):
        return lib().cusift_ctx_arena_bytes(self.handle)

    def set_policy(self, key, value):
        check(lib().cusift_ctx_set_policy(self.handle, int(key), int(value)))

    def get_policy(self, key):
        v = C.c_int(0)
        check(lib().cusift_ctx_get_policy(self.handle, int(key), C.byref(v)))
        return v.value

    def forks(self):
        """cusift_ctx_forks: extractions that ran octave 0's detection on the context's second stream."""
        return int(lib().cusift_ctx_forks(self.handle))

    # ---- timing ----
    def timing_enable(self, on=True):
        check(lib().cusift_ctx_timing_enable(self.handle, 1 if on else 0))

    def timing_reset(self):
        check(lib().cusift_ctx_timing_reset(self.handle))

    def timing_read(self):
        ms = (C.c_float * NUM_STAGES)()
        n = (C.c_int * NUM_STAGES)()
        check(lib().cusift_ctx_timing_read(self.handle, ms, n))
        return {STAGE_NAMES[i]: (float(ms[i]), int(n[i])) for i in range(NUM_STAGES)}

    # ---- raw device memory ----
    def malloc(self, nbytes):
        p = C.c_void_p()
        check(lib().cusift_malloc(C.byref(p), nbytes))
        return p.value

    def free(self, ptr):
        check(lib().cusift_free(C.c_void_p(ptr)))

    def memset(self, ptr, value, nbytes):
        check(lib().cusift_memset(self.handle, C.c_void_p(ptr), value, nbytes))

    def h2d(self, d_ptr, arr):
        arr = np.ascontiguousarray(arr)
        check(lib().cusift_memcpy_h2d(self.handle, C.c_void_p(d_ptr), arr.ctypes.data, arr.nbytes))

    def d2h(self, arr, d_ptr):
        assert arr.flags["C_CONTIGUOUS"]
        check(lib().cusift_memcpy_d2h(self.handle, arr.ctypes.data, C.c_void_p(d_ptr), arr.nbytes))

    # ---- front-end ----
    def image_u8_h2d(self, d_dst, dst_pitch, img_u8):
        img_u8 = np.ascontiguousarray(img_u8, dtype=np.uint8)
        h, w = img_u8.shape
        check(lib().cusift_image_u8_h2d(self.handle, d_dst, dst_pitch, img_u8.ctypes.data, w, h))

    def u8_to_f32(self, d_dst, dst_pitch, d_src, w, h, src_pitch_bytes, n_images=1, dst_stride=None, src_stride=None):
        dst_stride = h * dst_pitch if dst_stride is None else dst_stride
        src_stride = h * src_pitch_bytes if src_stride is None else src_stride
        check(lib().cusift_u8_to_f32(self.handle, d_dst, dst_pitch, dst_stride, d_src, w, h, src_pitch_bytes,
                                     src_stride, n_images))

    def gaussian3x3(self, d_dst, dst_pitch, d_src, w, h, src_pitch, sigma, n_images=1, dst_stride=None,
                    src_stride=None):
        dst_stride = h * dst_pitch if dst_stride is None else dst_stride
        src_stride = h * src_pitch if src_stride is None else src_stride
        check(lib().cusift_gaussian3x3(self.handle, d_dst, dst_pitch, dst_stride, d_src, w, h, src_pitch, src_stride,
                                       n_images, sigma))

    # ---- stage entry points (device pointers are plain ints) ----
    def scale_down(self, d_dst, dst_pitch, d_src, w, h, src_pitch, n_images=1, dst_stride=None, src_stride=None,
                   variance=0.5):
        dst_stride = (h // 2) * dst_pitch if dst_stride is None else dst_stride
        src_stride = h * src_pitch if src_stride is None else src_stride
        check(lib().cusift_scale_down(self.handle, d_dst, dst_pitch, dst_stride, d_src, w, h, src_pitch, src_stride,
                                      n_images, variance))

    def scale_up(self, d_dst, dst_pitch, d_src, w, h, src_pitch, n_images=1, dst_stride=None, src_stride=None):
        """cusift_scale_up: the 2x enlargement octave -1 is searched in (dst is 2w x 2h, dst_pitch >= 2w)."""
        dst_stride, src_stride = check_scale_up_args(d_dst, dst_pitch, d_src, w, h, src_pitch, n_images, dst_stride,
                                                     src_stride)
        check(lib().cusift_scale_up(self.handle, d_dst, dst_pitch, dst_stride, d_src, w, h, src_pitch, src_stride,
                                    n_images))

    def scale_down_levels(self, d_src, w, h, src_pitch, d_levels, pitches, n_images=1, src_stride=None, strides=None,
                          variance=0.5):
        """cusift_scale_down_levels: the ScaleDown chain (level k = (w >> k) x (h >> k), k = 1..len(d_levels)) in one launch."""
        n = len(d_levels)
        src_stride = h * src_pitch if src_stride is None else src_stride
        if strides is None:
            strides = [(h >> (k + 1)) * pitches[k] for k in range(n)]
        ptrs = (C.c_void_p * n)(*[int(p) for p in d_levels])
        pit = (C.c_int * n)(*[int(p) for p in pitches])
        strd = (C.c_size_t * n)(*[int(x) for x in strides])
        check(lib().cusift_scale_down_levels(self.handle, d_src, w, h, src_pitch, src_stride, ptrs, pit, strd, n,
                                             n_images, variance))

    def laplace_multi(self, d_img, w, h, pitch, init_blur, d_dog, n_images=1, img_stride=None, dog_stride=None):
        img_stride = h * pitch if img_stride is None else img_stride
        dog_stride = 7 * h * pitch if dog_stride is None else dog_stride
        check(lib().cusift_laplace_multi(self.handle, d_img, w, h, pitch, img_stride, init_blur, d_dog, dog_stride,
                                         n_images))

    def find_points_multi(self, d_dog, w, h, pitch, peak_thresh, edge_thresh, subsampling, d_points, max_pts,
                          d_counters, n_images=1, dog_stride=None):
        dog_stride = 7 * h * pitch if dog_stride is None else dog_stride
        check(lib().cusift_find_points_multi(self.handle, d_dog, w, h, pitch, dog_stride, peak_thresh, edge_thresh,
                                             subsampling, d_points, max_pts, d_counters, n_images))

    def detect_multi(self, d_img, w, h, pitch, init_blur, peak_thresh, edge_thresh, subsampling, d_points, max_pts,
                     d_counters, n_images=1, img_stride=None):
        img_stride = h * pitch if img_stride is None else img_stride
        check(lib().cusift_detect_multi(self.handle, d_img, w, h, pitch, img_stride, init_blur, peak_thresh,
                                        edge_thresh, subsampling, d_points, max_pts, d_counters, n_images))

    def detect_multi_down(self, d_img, w, h, pitch, init_blur, peak_thresh, edge_thresh, subsampling, d_heads, max_pts,
                          d_counters, d_next, next_pitch, n_images=1, img_stride=None, next_stride=None, variance=0.5):
        """cusift_detect_multi_down: the fused detection (keypoint HEADS, 64 bytes each) + the next octave's image."""
        img_stride = h * pitch if img_stride is None else img_stride
        next_stride = (h // 2) * next_pitch if next_stride is None else next_stride
        check(lib().cusift_detect_multi_down(self.handle, d_img, w, h, pitch, img_stride, init_blur, peak_thresh,
                                             edge_thresh, subsampling, d_heads, max_pts, d_counters, n_images, d_next,
                                             next_pitch, next_stride, variance))

    def compute_orientations(self, d_img, w, h, pitch, d_points, max_pts, d_first, d_counters, tex_frac_bits=8,
                             n_images=1, img_stride=None):
        img_stride = h * pitch if img_stride is None else img_stride
        check(lib().cusift_compute_orientations(self.handle, d_img, w, h, pitch, img_stride, d_points, max_pts,
                                                d_first, d_counters, tex_frac_bits, n_images))

    def extract_descriptors(self, d_img, w, h, pitch, d_points, max_pts, d_first, d_counters, subsampling,
                            tex_frac_bits=8, n_images=1, img_stride=None):
        img_stride = h * pitch if img_stride is None else img_stride
        check(lib().cusift_extract_descriptors(self.handle, d_img, w, h, pitch, img_stride, d_points, max_pts,
                                               d_first, d_counters, subsampling, tex_frac_bits, n_images))

    # ---- band forms (strip tiling) ----
    def scale_down_band(self, d_dst, dst_pitch, dst_row0, r_begin, r_end, d_src, w, h_src, src_pitch, src_row0,
                        h_src_global, variance=0.5):
        check(lib().cusift_scale_down_band(self.handle, d_dst, dst_pitch, dst_row0, r_begin, r_end, d_src, w, h_src,
                                           src_pitch, src_row0, h_src_global, variance))

    def detect_band(self, d_img, w, h, pitch, row0, h_global, cy_begin, cy_end, init_blur, peak_thresh, edge_thresh,
                    subsampling, d_points, max_pts, d_counter):
        check(lib().cusift_detect_band(self.handle, d_img, w, h, pitch, row0, h_global, cy_begin, cy_end, init_blur,
                                       peak_thresh, edge_thresh, subsampling, d_points, max_pts, d_counter))

    def describe_band(self, d_img, w, h, pitch, row0, h_global, d_points, max_pts, d_first, d_counter, subsampling,
                      tex_frac_bits=8, d_flags=None, root_sift=0):
        check(lib().cusift_describe_band(self.handle, d_img, w, h, pitch, row0, h_global, d_points, max_pts, d_first,
                                         d_counter, subsampling, tex_frac_bits, root_sift, d_flags))

    def math_eval(self, op, d_a, d_b, d_out, d_out2, n):
        """cusift_math_eval: op 0 expf, 1 exp2f, 2 atan2f(a, b), 3 sincosf -> (out, out2), 4 the descriptor's angle
        coordinate of (dy = a, dx = b), 5 the orientation bin's shortcut of (dy = a, dx = b): out = bin (+ 64 if the sample
        is `near` a bin edge: the kernel then evaluates the reference's formula), out2 = that formula's bin; device
        pointers."""
        check(lib().cusift_math_eval(self.handle, op, d_a, d_b, d_out, d_out2, n))

    def rootsift(self, d_points, num_pts):
        check(lib().cusift_rootsift(self.handle, d_points, num_pts))

    def pack_points(self, d_points, d_counters, n_images, max_pts, d_packed, capacity, d_offsets=None):
        check(lib().cusift_pack_points(self.handle, d_points, d_counters, n_images, max_pts, d_packed, capacity,
                                       d_offsets))

    # ---- matcher ----
    def pack_points_trimmed(self, d_points, d_counters, n_images, max_pts, d_packed, capacity, d_offsets=None):
        check(lib().cusift_pack_points_trimmed(self.handle, d_points, d_counters, n_images, max_pts, d_packed, capacity,
                                               d_offsets))

    def expand_trimmed(self, d_trimmed, n, d_points):
        check(lib().cusift_expand_trimmed(self.handle, d_trimmed, n, d_points))

    def pack_points_compact(self, d_points, d_counters, n_images, max_pts, d_packed, capacity, d_offsets=None):
        check(lib().cusift_pack_points_compact(self.handle, d_points, d_counters, n_images, max_pts, d_packed, capacity,
                                               d_offsets))

    def match(self, d_sift1, n1, d_sift2, n2, distance=1):
        """MatchSiftData on device records: distance 1 = L2 (2 - 2 x.y), 0 = dot product."""
        check(lib().cusift_match(self.handle, d_sift1, n1, d_sift2, n2, distance))

    def match_mutual(self, d_sift1, n1, d_sift2, n2, distance=1):
        """cusift_match_mutual: both directions from one pass -- d_sift1 receives what match() writes, d_sift2 the same
        five fields over the records of d_sift1 (lowest record on exactly tied best scores).  Both record sets are
        written: overlapping ranges are refused.  Asynchronous."""
        check(lib().cusift_match_mutual(self.handle, d_sift1, n1, d_sift2, n2, distance))

    def match_guided(self, d_sift1, n1, d_sift2, n2, model, m, radius, distance=1):
        """cusift_match_guided: match() where a record of d_sift2 whose coords2D fail the geometric test against a row's
        coords2D cannot be that row's best or second best.  model "homography" (0): m = H with x2 ~ H x1, the test is
        |x2 - H x1| < radius; "epipolar" (1): m = F with x2^T F x1 = 0, the test is the distance of x2 from the line
        F x1 < radius.  m: 3 x 3 or 9 values, widened to float64.  A row that nothing passes ends with match = -1.
        Asynchronous; m is read before the call returns."""
        model, m = (GUIDE_MODELS.get(model, model), None) if m is None else guide_models(model, m)
        check(lib().cusift_match_guided(self.handle, d_sift1, n1, d_sift2, n2, distance, model,
                                        None if m is None else m.ctypes.data, radius))

    def match_projected(self, d_sift1, n1, d_sift2, n2, rt, camera2, radius, distance=1):
        """cusift_match_projected: match() where a record of d_sift2 counts for a row only within `radius` pixels of where
        the pose puts the row's coords3D in the image of `camera2` (capi.Camera).  rt: [R | t], 3 x 4 or 12 values, X1 = R
        X2 + t as estimate_pnp / register_pnp return it, widened to float64.  A row without depth (Z == 0), behind camera
        2 or that nothing passes ends with match = -1.  coords3D is read, never written.  Asynchronous; rt and camera2
        are read before the call returns."""
        rt = None if rt is None else pose_models(rt)
        check(lib().cusift_match_projected(self.handle, d_sift1, n1, d_sift2, n2, distance,
                                           None if rt is None else rt.ctypes.data,
                                           C.byref(camera2) if camera2 is not None else None, radius))

    def find_homography(self, d_sift, num_pts, rand_pts, thresh=5.0, want_all=False):
        """cusift_find_homography: rand_pts is an int32 array [4, num_loops] of sample indices into d_sift.
        Returns (H[9], num_matches) or, with want_all, (H, num_matches, all_homographies[8, L], all_counts[L])."""
        rand_pts = np.ascontiguousarray(rand_pts, dtype=np.int32)
        assert rand_pts.ndim == 2 and rand_pts.shape[0] == 4, rand_pts.shape
        loops = rand_pts.shape[1]
        hom = np.zeros(9, dtype=np.float32)
        n = C.c_int(0)
        all_h = np.zeros((8, loops), dtype=np.float32) if want_all else None
        all_c = np.zeros(loops, dtype=np.int32) if want_all else None
        check(lib().cusift_find_homography(self.handle, d_sift, num_pts, rand_pts.ctypes.data, loops, thresh,
                                           hom.ctypes.data, C.byref(n), all_h.ctypes.data if want_all else None,
                                           all_c.ctypes.data if want_all else None))
        return (hom, n.value, all_h, all_c) if want_all else (hom, n.value)

    # (result type, dtype, shape of a reported model, samples and values per hypothesis) of the models that _ransac serves
    _H = (PlanarResult, np.float32, 9, 4, 8)
    _F = (EpipolarResult, np.float64, 9, 8, 9)
    _P = (PnPResult, np.float64, (3, 4), 6, 12)

    @staticmethod
    def _ransac(kind, call, num_pts, loops, want_all):
        """Allocates the outputs of a homography, fundamental-matrix or PnP call, calls it with them, returns the result."""
        result, dtype, shape, samples, values = kind
        model, ransac = np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=dtype)
        n_cand, n_match, n_fit, best = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        flags = np.zeros(max(num_pts, 1), dtype=np.int8)
        drawn = np.zeros((samples, loops), dtype=np.int32) if want_all else None
        all_m = np.zeros((values, loops), dtype=dtype) if want_all else None
        all_c = np.zeros(loops, dtype=np.int32) if want_all else None
        check(call(model.ctypes.data, ransac.ctypes.data, C.byref(n_cand), C.byref(n_match), C.byref(n_fit), C.byref(best),
                   flags.ctypes.data, drawn.ctypes.data if want_all else None, all_m.ctypes.data if want_all else None,
                   all_c.ctypes.data if want_all else None))
        return result(model, ransac, n_cand.value, n_match.value, n_fit.value, best.value,
                      flags[:max(num_pts, 0)].astype(bool), drawn, all_m, all_c)

    def estimate_homography(self, d_sift, num_pts, num_pts2=-1, rule=0, lo=0.0, hi=0.8, loops=10000, thresh=5.0,
                            refine_loops=5, refine_thresh=3.0, seed=0, want_all=False):
        """cusift_estimate_homography: FindHomography + ImproveHomography on device records that carry match fields --
        candidates by `rule` (0: score > lo && ambiguity < hi; 1: score < lo^2 && ambiguity < hi^2), samples drawn on the
        device from `seed`, the first hypothesis with the most inliers, `refine_loops` rounds of the fp64 refit;
        match_error of every device record is written.  One synchronisation.  Returns a PlanarResult; with want_all its
        drawn [4, L] / all_homographies [8, L] / all_counts [L] are filled."""
        loops = int(loops)
        return self._ransac(self._H, lambda *out: lib().cusift_estimate_homography(
            self.handle, d_sift, num_pts, num_pts2, PLANAR_RULES.get(rule, rule), lo, hi, loops, thresh, refine_loops,
            refine_thresh, _seed64(seed), *out), num_pts, max(loops, 0), want_all)

    def register_planar(self, d_sift1, n1, d_sift2, n2, distance=1, rule=None, lo=None, hi=None, loops=10000,
                        thresh=5.0, refine_loops=5, refine_thresh=3.0, seed=0, want_all=False):
        """cusift_register_planar: match(distance), then estimate_homography over d_sift1 with num_pts2 = n2 -- one
        synchronisation, the staged route's bits.  rule defaults to the one that fits the distance (1 = L2: rule 1 with
        lo = 999, hi = 0.8 as score / ambiguity thresholds; 0 = dot product: rule 0 with lo = 0, hi = 0.8)."""
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        loops = int(loops)
        return self._ransac(self._H, lambda *out: lib().cusift_register_planar(
            self.handle, d_sift1, n1, d_sift2, n2, distance, rule, lo, hi, loops, thresh, refine_loops, refine_thresh,
            _seed64(seed), *out), n1, max(loops, 0), want_all)

    def estimate_fundamental(self, d_sift, num_pts, num_pts2=-1, rule=0, lo=0.0, hi=0.8, loops=10000, thresh=1.0,
                             refine_loops=5, refine_thresh=1.0, seed=0, want_all=False):
        """cusift_estimate_fundamental: fundamental-matrix RANSAC + refit, all fp64, on device records that carry match
        fields -- candidates by `rule` as estimate_homography, eight samples per hypothesis drawn on the device from
        `seed`, the normalised 8-point solve, Sampson inlier counts over the candidates, the first hypothesis with the
        most inliers, `refine_loops` rounds of the refit over the current inliers; match_error (the Sampson distance) of
        every device record is written.  thresh / refine_thresh are in pixels.  One synchronisation.  Returns an
        EpipolarResult; with want_all its drawn [8, L] / all_fundamentals [9, L] / all_counts [L] are filled."""
        loops = int(loops)
        return self._ransac(self._F, lambda *out: lib().cusift_estimate_fundamental(
            self.handle, d_sift, num_pts, num_pts2, PLANAR_RULES.get(rule, rule), lo, hi, loops, thresh, refine_loops,
            refine_thresh, _seed64(seed), *out), num_pts, max(loops, 0), want_all)

    def register_epipolar(self, d_sift1, n1, d_sift2, n2, distance=1, rule=None, lo=None, hi=None, loops=10000,
                          thresh=1.0, refine_loops=5, refine_thresh=1.0, seed=0, want_all=False):
        """cusift_register_epipolar: match(distance), then estimate_fundamental over d_sift1 with num_pts2 = n2 -- one
        synchronisation, the staged route's bytes.  rule / lo / hi default as in register_planar; the cross-check setting
        is honoured as there."""
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        loops = int(loops)
        return self._ransac(self._F, lambda *out: lib().cusift_register_epipolar(
            self.handle, d_sift1, n1, d_sift2, n2, distance, rule, lo, hi, loops, thresh, refine_loops, refine_thresh,
            _seed64(seed), *out), n1, max(loops, 0), want_all)

    def _guided_chain(self, register, estimate, guided, thresh, d_sift1, n1, d_sift2, n2, radius, opts):
        """register -> the guided matcher under the refined model -> estimate over the rewritten records, same options.
        guided(d_sift1, n1, d_sift2, n2, refined model, radius, distance, on_bytes) is match_guided under H or F, or
        match_projected under [R | t] -- on_bytes: match8_guided_records / match8_projected_records, which quantise both
        record sets into the context's tables and run the 8-bit guided matcher.  opts["match8"] (default False) chooses
        the second pass on bytes; the first pass follows set_match_bits.  With the match bits at 8 the chain runs only
        with match8=True: it never matches bytes first and floats second without being told to."""
        opts = dict(opts)
        on_bytes = bool(opts.pop("match8", False))
        if self.cross_check:
            raise CusiftError("guided registration: turn the cross-check off first (set_cross_check(False)) -- the "
                              "guided matcher has no column side")
        if self.match_bits == 8 and not on_bytes:
            raise CusiftError("guided registration: the match bits are 8 -- pass match8=True for a second pass on bytes "
                              "too, or set them back to 32 first (set_match_bits(32))")
        first = register(d_sift1, n1, d_sift2, n2, **opts)
        distance = opts.get("distance", 1)
        rule, lo, hi = _rule_defaults(distance, opts.get("rule"), opts.get("lo"), opts.get("hi"))
        guided(d_sift1, n1, d_sift2, n2, first[0], opts.get("thresh", thresh) if radius is None else radius, distance,
               on_bytes)
        again = {k: v for k, v in opts.items() if k != "distance"}
        again.update(rule=rule, lo=lo, hi=hi)
        return first, estimate(d_sift1, n1, n2, **again)

    def register_planar_guided(self, d_sift1, n1, d_sift2, n2, radius=None, **opts):
        """The second matching pass of a planar registration: register_planar(**opts), then match_guided under the refined
        homography it returned (radius None: that call's thresh), then estimate_homography over the rewritten records of
        d_sift1 with num_pts2 = n2 and the same options and seed.  Matches that the ratio test of the first pass threw
        away because a look-alike scored as well come back when the look-alike lies elsewhere.  Returns (first pass,
        guided pass), two PlanarResults.  match8=True: the second pass matches bytes (match8_guided_records) -- with
        set_match_bits(8) both passes do, bit for bit register_planar + quantize_descriptors + match8_guided +
        estimate_homography; at 8 bits the chain runs only with it.  CusiftError while the cross-check is on.  Blocking,
        twice."""
        return self._guided_chain(self.register_planar, self.estimate_homography, self._guided_by("homography"), 5.0,
                                  d_sift1, n1, d_sift2, n2, radius, opts)

    def register_epipolar_guided(self, d_sift1, n1, d_sift2, n2, radius=None, **opts):
        """register_planar_guided for two views of a general scene: register_epipolar(**opts), match_guided under the
        refined fundamental matrix (radius None: that call's thresh, pixels from the epipolar line), estimate_fundamental
        over the rewritten records.  Returns (first pass, guided pass), two EpipolarResults."""
        return self._guided_chain(self.register_epipolar, self.estimate_fundamental, self._guided_by("epipolar"), 1.0,
                                  d_sift1, n1, d_sift2, n2, radius, opts)

    def _guided_by(self, model):
        """match_guided -- on bytes: match8_guided_records -- under one kind of model, in _guided_chain's argument
        order"""
        def guided(d1, n1, d2, n2, m, radius, distance, on_bytes):
            (self.match8_guided_records if on_bytes else self.match_guided)(d1, n1, d2, n2, model, m, radius, distance)
        return guided

    @staticmethod
    def _pose(call):
        rt, votes, sigma = np.zeros((3, 4), dtype=np.float64), np.zeros(4, dtype=np.int32), np.zeros(3, dtype=np.float64)
        front = C.c_int(0)
        out = call(rt.ctypes.data, C.byref(front), votes.ctypes.data, sigma.ctypes.data)
        return out, PoseResult(rt, front.value, votes, sigma)

    def estimate_pose(self, d_sift, num_pts, fundamental, camera, camera2=None, num_pts2=-1, rule=0, lo=0.0, hi=0.8,
                      thresh=1.0):
        """cusift_estimate_pose: from a fundamental matrix (float64 [9], as estimate_fundamental returns it) and the two
        views' intrinsics (capi.Camera; camera2 None: both views use `camera`) to [R | t] -- the essential matrix's four
        candidates, the cheirality vote over the candidates that fit F at `thresh`, all fp64 on the device -- and to a
        triangulated point in coords3D of every record that is in front (zeros elsewhere), at the scale |t| = 1.  One
        synchronisation.  Returns a PoseResult."""
        f = np.ascontiguousarray(fundamental, dtype=np.float64).ravel()
        if f.size != 9:
            raise ValueError("fundamental must hold 9 values, not %d" % f.size)
        _, res = self._pose(lambda *out: check(lib().cusift_estimate_pose(
            self.handle, d_sift, num_pts, num_pts2, PLANAR_RULES.get(rule, rule), lo, hi, f.ctypes.data, thresh,
            C.byref(camera), C.byref(camera2) if camera2 is not None else None, *out)))
        return res

    def register_pose(self, d_sift1, n1, d_sift2, n2, camera, camera2=None, distance=1, rule=None, lo=None, hi=None,
                      loops=10000, thresh=1.0, refine_loops=5, refine_thresh=1.0, seed=0, want_all=False):
        """cusift_register_pose: register_epipolar, then estimate_pose at refine_thresh with the refined F where the
        device left it -- one synchronisation, the staged route's bytes.  Returns a RegisterPoseResult: the
        EpipolarResult's fields, then rt, num_front, votes, sigma."""
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        loops = int(loops)
        epi, pose = self._pose(lambda *pout: self._ransac(self._F, lambda *out: lib().cusift_register_pose(
            self.handle, d_sift1, n1, d_sift2, n2, distance, rule, lo, hi, loops, thresh, refine_loops, refine_thresh,
            _seed64(seed), C.byref(camera), C.byref(camera2) if camera2 is not None else None,
            *(out + pout)), n1, max(loops, 0), want_all))
        return RegisterPoseResult(*(epi + pose))

    def estimate_pnp(self, d_sift, num_pts, camera2, num_pts2=-1, rule=0, lo=0.0, hi=0.8, loops=10000, thresh=2.0,
                     refine_loops=5, refine_thresh=2.0, seed=0, want_all=False):
        """cusift_estimate_pnp: absolute pose from 3-D/2-D matches, all fp64 on the device -- the records' coords3D (frame
        1's camera coordinates, as lift_depth or register_pose wrote them) against their matches' pixels in the image of
        `camera2` (capi.Camera).  Candidates by `rule` as estimate_fundamental plus a finite, non-zero depth; six samples
        per hypothesis, the 11-row DLT and the nearest rotation; reprojection inliers in pixels; the first hypothesis with
        the most inliers; `refine_loops` Gauss-Newton rounds.  match_error (the reprojection error) of every device record
        is written.  One synchronisation.  Returns a PnPResult: X1 = R X2 + t, t in the unit of coords3D."""
        loops = int(loops)
        return self._ransac(self._P, lambda *out: lib().cusift_estimate_pnp(
            self.handle, d_sift, num_pts, num_pts2, PLANAR_RULES.get(rule, rule), lo, hi,
            C.byref(camera2) if camera2 is not None else None, loops, thresh, refine_loops, refine_thresh, _seed64(seed),
            *out), num_pts, max(loops, 0), want_all)

    def register_pnp(self, d_sift1, n1, d_sift2, n2, camera2, distance=1, rule=None, lo=None, hi=None, loops=10000,
                     thresh=2.0, refine_loops=5, refine_thresh=2.0, seed=0, want_all=False):
        """cusift_register_pnp: match(distance), then estimate_pnp over d_sift1 with num_pts2 = n2 -- one
        synchronisation, the staged route's bytes.  rule / lo / hi default as in register_planar; the cross-check setting
        is honoured as there."""
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        loops = int(loops)
        return self._ransac(self._P, lambda *out: lib().cusift_register_pnp(
            self.handle, d_sift1, n1, d_sift2, n2, distance, rule, lo, hi,
            C.byref(camera2) if camera2 is not None else None, loops, thresh, refine_loops, refine_thresh, _seed64(seed),
            *out), n1, max(loops, 0), want_all)

    def register_pnp_guided(self, d_sift1, n1, d_sift2, n2, camera2, radius=None, **opts):
        """register_planar_guided for a pose from 3-D/2-D matches: register_pnp(camera2, **opts), match_projected under
        the refined [R | t] (radius None: that call's thresh, pixels from the projection of coords3D), estimate_pnp over
        the rewritten records with num_pts2 = n2 and the same options and seed.  Returns (first pass, guided pass), two
        PnPResults.  match8=True: the second pass is match8_projected_records, on bytes; while the match bits are 8 the
        chain runs only with it.  CusiftError while the cross-check is on.  Blocking, twice."""
        def projected(d1, m1, d2, m2, rt, r, distance, on_bytes):
            (self.match8_projected_records if on_bytes else self.match_projected)(d1, m1, d2, m2, rt, camera2, r, distance)
        return self._guided_chain(
            lambda d1, m1, d2, m2, **o: self.register_pnp(d1, m1, d2, m2, camera2, **o),
            lambda d1, m1, m2, **o: self.estimate_pnp(d1, m1, camera2, m2, **o),
            projected, 2.0, d_sift1, n1, d_sift2, n2, radius, opts)

    def estimate_rigid(self, coord, indices=None, loops=None, thresh2=0.0025, kind="3d", seed=0, want_all=False):
        """cusift_estimate_rigid: RANSAC rigid transform x ~ R y + t from coord float32 [N, 6] (reference xyz, moving
        xyz).  indices int32 [L, 3]: the samples of every hypothesis; None: `loops` hypotheses drawn on the device from
        `seed`.  kind "3d" (three-point Horn estimate, refitted over the winner's inliers) or "2d" (rotation about y
        from two points, no refit).  Returns (Rt [3, 4], num_inliers, best_loop, inlier flags bool [N]) and, with
        want_all, also (all Rt [L, 3, 4], all counts [L], the samples used [L, 3])."""
        coord, indices, loops, rtype = check_rigid_args(coord, indices, loops, thresh2, kind)
        n_pts = coord.shape[0]
        rt = np.zeros((3, 4), dtype=np.float32)
        n, best = C.c_int(0), C.c_int(-1)
        flags = np.zeros(n_pts, dtype=np.int8)
        all_rt = np.zeros((loops, 3, 4), dtype=np.float32) if want_all else None
        all_c = np.zeros(loops, dtype=np.int32) if want_all else None
        drawn = np.zeros((loops, 3), dtype=np.int32) if want_all else None
        check(lib().cusift_estimate_rigid(self.handle, coord.ctypes.data, n_pts,
                                          indices.ctypes.data if indices is not None else None, loops, float(thresh2),
                                          rtype, _seed64(seed), rt.ctypes.data, C.byref(n),
                                          C.byref(best), flags.ctypes.data, all_rt.ctypes.data if want_all else None,
                                          all_c.ctypes.data if want_all else None,
                                          drawn.ctypes.data if want_all else None))
        out = (rt, n.value, best.value, flags.astype(bool))
        return out + (all_rt, all_c, drawn) if want_all else out

    # ---- RGB-D registration ----
    def lift_depth(self, d_points, max_pts, d_depth, w, h, camera, pitch=None, n_images=1, d_counters=None,
                   image_stride=None):
        """cusift_lift_depth: coords3D of d_points[n_images][max_pts] from coords2D, the 16-bit depth image of each
        frame (device pointer; rows `pitch` samples apart, frames `image_stride` samples apart) and `camera`.
        d_counters None: every frame has max_pts records.  Asynchronous."""
        pitch = w if pitch is None else pitch
        image_stride = h * pitch if image_stride is None else image_stride
        check(lib().cusift_lift_depth(self.handle, d_points, d_counters, n_images, max_pts, d_depth, w, h, pitch,
                                      image_stride, C.byref(camera)))

    def set_keep_strongest(self, k):
        """cusift_ctx_set_keep_strongest: every later extraction on this context (and every graph recorded from now on)
        keeps the K strongest keypoints per image, selected on the device before they are described; 0 turns it off.
        K > max_pts is refused by the extraction."""
        k = check_keep_strongest(k)
        check(lib().cusift_ctx_set_keep_strongest(self.handle, k))

    def set_second_orientation(self, ratio):
        """cusift_ctx_set_second_orientation: every later extraction on this context (and every graph recorded from now
        on) appends, behind each image's records, a duplicate of every keypoint whose orientation histogram has a second
        peak above `ratio` of the first, described at that orientation (second_orientations is the stage).  0 turns it
        off; 0.8 is the reference's constant."""
        ratio = check_second_orientation(ratio)
        check(lib().cusift_ctx_set_second_orientation(self.handle, ratio))

    def set_cross_check(self, on):
        """cusift_ctx_set_cross_check: while on, register_planar, register_epipolar, register_pose, register_rgbd,
        register_planar_batch, register_rgbd_batch, register_epipolar_batch, register_pose_batch and register_pnp_batch
        on this context keep mutual matches only -- record i of frame 1
        takes part only if the column side's best for its match is i (the lowest record on exactly tied best scores).
        The four pair calls then write the match fields of d_sift2 as well and refuse overlapping record ranges.  Nothing
        else changes."""
        check(lib().cusift_ctx_set_cross_check(self.handle, check_cross_check(on)))
        self.cross_check = bool(on)

    def set_match_bits(self, bits):
        """cusift_ctx_set_match_bits: 32 (default) or 8.  While 8, the calls set_cross_check affects quantise their
        records into scratch of the context and match the bytes on the int8 matrix pipe (match8 / match8_mutual and the
        batch forms) -- bit for bit the staged route quantize_descriptors + match8 + estimate_*.  Nothing else reads it;
        while it is 8 the guided chains run with match8=True only (their second pass on bytes too)."""
        check(lib().cusift_ctx_set_match_bits(self.handle, check_match_bits(bits)))
        self.match_bits = int(bits)

    def select_strongest(self, d_heads, n_lists, n_images, capacity, d_counts, keep, d_kept):
        """cusift_select_strongest: the selection alone, on lists of 64-byte record heads.  d_heads [n_lists, n_images,
        capacity, 64 B], d_counts uint32 [n_lists, n_images] (in: held, out: kept) and d_kept uint32 [n_images] are
        device pointers.  Asynchronous."""
        check_select_strongest_args(d_heads, n_lists, n_images, capacity, d_counts, keep, d_kept)
        check(lib().cusift_select_strongest(self.handle, d_heads, n_lists, n_images, capacity, d_counts, keep, d_kept))

    def select_matches(self, d_sift1, n1, d_sift2, n2, d_pairs, d_coord, d_count, score_threshold=999.0,
                       ambiguity_threshold=1.0, kind="3d"):
        """cusift_select_matches: MatchSiftData's threshold filter on the device, after match().  d_pairs int32 [n1, 2],
        d_coord float32 [n1, 6] and d_count int32 [1] are device pointers; rows come in ascending record order.
        kind "3d" also asks for a depth on both sides.  Asynchronous."""
        check(lib().cusift_select_matches(self.handle, d_sift1, n1, d_sift2, n2, score_threshold, ambiguity_threshold,
                                          RIGID_KINDS[kind], d_pairs, d_coord, d_count))

    def select_mutual(self, d_sift1, n1, d_sift2, n2, d_pairs, d_coord, d_count, score_threshold=999.0,
                      ambiguity_threshold=1.0, kind="3d"):
        """cusift_select_mutual: select_matches() plus the cross-check -- record i is kept only if the match of its
        partner in d_sift2 is i (after match_mutual(), or match() in both directions).  The same outputs, in ascending
        record order.  Asynchronous."""
        check(lib().cusift_select_mutual(self.handle, d_sift1, n1, d_sift2, n2, score_threshold, ambiguity_threshold,
                                         RIGID_KINDS[kind], d_pairs, d_coord, d_count))

    def register_rgbd(self, d_sift1, n1, d_depth1, d_sift2, n2, d_depth2, w, h, camera, pitch=None, distance=1,
                      score_threshold=999.0, ambiguity_threshold=1.0, loops=1024, thresh2=0.0025, kind="3d", seed=0):
        """cusift_register_rgbd: lift both frames, match, select (3-D), RANSAC + refit -- one synchronisation, at the
        read-back.  Returns (Rt [3, 4] with x1 ~ R x2 + t, pairs int32 [num_matches, 2], inlier flags bool
        [num_matches], num_inliers)."""
        pitch = w if pitch is None else pitch
        rt = np.zeros((3, 4), dtype=np.float32)
        n_match, n_in = C.c_int(0), C.c_int(0)
        pairs = np.zeros((max(n1, 1), 2), dtype=np.int32)
        flags = np.zeros(max(n1, 1), dtype=np.int8)
        check(lib().cusift_register_rgbd(self.handle, d_sift1, n1, d_depth1, d_sift2, n2, d_depth2, w, h, pitch,
                                         C.byref(camera), distance, score_threshold, ambiguity_threshold, int(loops),
                                         float(thresh2), RIGID_KINDS[kind], _seed64(seed),
                                         rt.ctypes.data, C.byref(n_match), C.byref(n_in), pairs.ctypes.data,
                                         flags.ctypes.data))
        return rt, pairs[:n_match.value].copy(), flags[:n_match.value].astype(bool), n_in.value

    # ---- RGB-D registration of a sequence: a batch of frames and a pair list ----
    def match_batch(self, d_points, d_counters, n_images, max_pts, pairs, d_rows, distance=1):
        """cusift_match_batch: cusift_match for every (frame 1, frame 2) of `pairs` (int32 [P, 2]) over
        d_points[n_images][max_pts] + d_counters[n_images] (None: max_pts each), into d_rows[P][max_pts] of MatchRow
        (device pointer).  The records are not written.  Asynchronous."""
        pairs = pair_list(pairs)
        check(lib().cusift_match_batch(self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data,
                                       len(pairs), distance, d_rows))

    def match_batch_mutual(self, d_points, d_counters, n_images, max_pts, pairs, d_rows, d_rows_back, distance=1):
        """cusift_match_batch_mutual: match_batch() plus, from the same pass, d_rows_back[P][max_pts] of MatchRow (device
        pointer): for every record of frame 2 its best and second best of frame 1, `match` an index into frame 1.  The
        records are not written.  Asynchronous."""
        pairs = pair_list(pairs)
        check(lib().cusift_match_batch_mutual(self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data,
                                              len(pairs), distance, d_rows, d_rows_back))

    def match_batch_guided(self, d_points, d_counters, n_images, max_pts, pairs, model, m, radius, d_rows, distance=1):
        """cusift_match_batch_guided: match_batch() with match_guided()'s rule, pair p under m[p] (float [P, 3, 3] or
        [P, 9], widened to float64; one kind of `model` and one radius for the list).  Asynchronous; m is read before the
        call returns."""
        pairs = pair_list(pairs)
        model, m = (GUIDE_MODELS.get(model, model), None) if m is None else guide_models(model, m, len(pairs))
        check(lib().cusift_match_batch_guided(self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data,
                                              len(pairs), distance, model, None if m is None else m.ctypes.data, radius,
                                              d_rows))

    def match_batch_projected(self, d_points, d_counters, n_images, max_pts, pairs, rts, camera2, radius, d_rows,
                              distance=1):
        """cusift_match_batch_projected: match_batch() with match_projected()'s rule, pair p under rts[p] (float [P, 3, 4]
        or [P, 12], widened to float64; one camera2 and one radius for the list).  Asynchronous; rts and camera2 are read
        before the call returns."""
        pairs = pair_list(pairs)
        rts = None if rts is None else pose_models(rts, len(pairs))
        check(lib().cusift_match_batch_projected(self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data,
                                                 len(pairs), distance, None if rts is None else rts.ctypes.data,
                                                 C.byref(camera2) if camera2 is not None else None, radius, d_rows))

    # ---- 8-bit descriptors ----
    def quantize_descriptors(self, d_points, max_pts, d_q, d_sums, n_images=1, d_counters=None):
        """cusift_quantize_descriptors: d_points[n_images][max_pts] (+ d_counters, None: max_pts each) to the byte table
        d_q uint8 [n_images][max_pts][128] (16-byte aligned: the OpenCV / VLFeat / COLMAP convention, 512 v clipped to
        255) and d_sums int32 [n_images][max_pts][2] = (sum q, sum q^2).  Rows past a count are not written.
        Asynchronous."""
        check(lib().cusift_quantize_descriptors(self.handle, d_points, d_counters, n_images, max_pts, d_q, d_sums))

    def desc8_sums(self, d_q, n, d_sums):
        """cusift_desc8_sums: d_sums int32 [n][2] of n byte descriptors d_q uint8 [n][128] that came from elsewhere."""
        check(lib().cusift_desc8_sums(self.handle, d_q, n, d_sums))

    def match8(self, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance=1):
        """cusift_match8: match() on two byte tables (int8 matrix pipe, exact integer scores scaled by 2^-18): writes the
        same five fields of d_sift1[0 .. n1); d_sift2 is read for coords2D of the match only.  Asynchronous."""
        check(lib().cusift_match8(self.handle, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance))

    def match8_mutual(self, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance=1):
        """cusift_match8_mutual: match8() in both directions from one pass: d_sift1 gets match8(1, 2)'s bytes, d_sift2
        gets match8(2, 1)'s.  Overlapping record ranges are refused.  Asynchronous."""
        check(lib().cusift_match8_mutual(self.handle, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance))

    def match8_batch_mutual(self, d_q, d_sums, d_counters, n_images, max_pts, pairs, d_rows, d_rows_back, distance=1):
        """cusift_match8_batch_mutual: match8_batch() plus d_rows_back[P][max_pts], the column side of every pair (what
        match8_batch would write for the swapped pair).  Asynchronous."""
        pairs = pair_list(pairs)
        check(lib().cusift_match8_batch_mutual(self.handle, d_q, d_sums, d_counters, n_images, max_pts,
                                               pairs.ctypes.data, len(pairs), distance, d_rows, d_rows_back))

    def match8_batch(self, d_q, d_sums, d_counters, n_images, max_pts, pairs, d_rows, distance=1):
        """cusift_match8_batch: match_batch() on the tables quantize_descriptors() wrote for a batch, match8()'s model;
        d_rows[P][max_pts] of MatchRow (device pointer).  Asynchronous."""
        pairs = pair_list(pairs)
        check(lib().cusift_match8_batch(self.handle, d_q, d_sums, d_counters, n_images, max_pts, pairs.ctypes.data,
                                        len(pairs), distance, d_rows))

    def match8_guided(self, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, model, m, radius, distance=1):
        """cusift_match8_guided: match8() where only the records of d_sift2 whose coords2D pass match_guided()'s test
        against a row's coords2D count for it (`model`, m and radius as there; the coordinates come from the records, the
        descriptors from the tables).  A row that nothing passes ends with match = -1 and the initial score.
        Asynchronous; m is read before the call returns."""
        model, m = (GUIDE_MODELS.get(model, model), None) if m is None else guide_models(model, m)
        check(lib().cusift_match8_guided(self.handle, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance,
                                         model, None if m is None else m.ctypes.data, radius))

    def match8_projected(self, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, rt, camera2, radius, distance=1):
        """cusift_match8_projected: match8() under match_projected()'s test -- a record of d_sift2 counts for a row only
        within `radius` pixels of where rt and camera2 put the row's coords3D.  Asynchronous; rt and camera2 are read
        before the call returns."""
        rt = None if rt is None else pose_models(rt)
        check(lib().cusift_match8_projected(self.handle, d_sift1, n1, d_q1, d_sums1, d_sift2, n2, d_q2, d_sums2, distance,
                                            None if rt is None else rt.ctypes.data,
                                            C.byref(camera2) if camera2 is not None else None, radius))

    def match8_batch_guided(self, d_points, d_q, d_sums, d_counters, n_images, max_pts, pairs, model, m, radius, d_rows,
                            distance=1):
        """cusift_match8_batch_guided: match8_batch() with match8_guided()'s rule, pair p under m[p]; d_points are the
        records the tables were quantised from (their coords2D are read, nothing of them is written).  Asynchronous; m is
        read before the call returns."""
        pairs = pair_list(pairs)
        model, m = (GUIDE_MODELS.get(model, model), None) if m is None else guide_models(model, m, len(pairs))
        check(lib().cusift_match8_batch_guided(self.handle, d_points, d_q, d_sums, d_counters, n_images, max_pts,
                                               pairs.ctypes.data, len(pairs), distance, model,
                                               None if m is None else m.ctypes.data, radius, d_rows))

    def match8_batch_projected(self, d_points, d_q, d_sums, d_counters, n_images, max_pts, pairs, rts, camera2, radius,
                               d_rows, distance=1):
        """cusift_match8_batch_projected: match8_batch() with match8_projected()'s rule, pair p under rts[p] and the one
        camera2; d_points are the records the tables were quantised from (coords2D and, of a pair's first frame, coords3D
        are read).  Asynchronous; rts and camera2 are read before the call returns."""
        pairs = pair_list(pairs)
        rts = None if rts is None else pose_models(rts, len(pairs))
        check(lib().cusift_match8_batch_projected(self.handle, d_points, d_q, d_sums, d_counters, n_images, max_pts,
                                                  pairs.ctypes.data, len(pairs), distance,
                                                  None if rts is None else rts.ctypes.data,
                                                  C.byref(camera2) if camera2 is not None else None, radius, d_rows))

    def match8_guided_records(self, d_sift1, n1, d_sift2, n2, model, m, radius, distance=1):
        """cusift_match8_guided_records: quantize_descriptors() of both record sets into tables of the context's, then
        match8_guided() on them -- match_guided()'s arguments, the 8-bit matcher's bytes.  Asynchronous."""
        model, m = (GUIDE_MODELS.get(model, model), None) if m is None else guide_models(model, m)
        check(lib().cusift_match8_guided_records(self.handle, d_sift1, n1, d_sift2, n2, distance, model,
                                                 None if m is None else m.ctypes.data, radius))

    def match8_projected_records(self, d_sift1, n1, d_sift2, n2, rt, camera2, radius, distance=1):
        """cusift_match8_projected_records: quantize_descriptors() of both record sets into tables of the context's, then
        match8_projected() on them -- match_projected()'s arguments, the 8-bit matcher's bytes.  Asynchronous."""
        rt = None if rt is None else pose_models(rt)
        check(lib().cusift_match8_projected_records(self.handle, d_sift1, n1, d_sift2, n2, distance,
                                                    None if rt is None else rt.ctypes.data,
                                                    C.byref(camera2) if camera2 is not None else None, radius))

    def register_rgbd_batch(self, d_points, d_counters, n_images, max_pts, d_depth, w, h, camera, pairs, pitch=None,
                            image_stride=None, distance=1, score_threshold=999.0, ambiguity_threshold=1.0, loops=1024,
                            thresh2=0.0025, kind="3d", seed=0):
        """cusift_register_rgbd_batch: one lift of all frames, then match, 3-D selection and RANSAC + refit of every
        pair of `pairs` (int32 [P, 2]) in a fixed number of launches and one synchronisation.  Pair p = (a, b) maps
        frame b into frame a and draws from seed + p.  Returns (rt float32 [P, 3, 4], num_matches int32 [P],
        num_inliers int32 [P], a list of P int32 [num_matches, 2] arrays of selected (record in a, record in b), a list
        of P bool [num_matches] inlier flags)."""
        pairs = pair_list(pairs)
        n_pairs = len(pairs)
        pitch = w if pitch is None else pitch
        image_stride = h * pitch if image_stride is None else image_stride
        rt = np.zeros((n_pairs, 3, 4), dtype=np.float32)
        n_match, n_in = np.zeros(n_pairs, dtype=np.int32), np.zeros(n_pairs, dtype=np.int32)
        sel = np.zeros((n_pairs, max(max_pts, 1), 2), dtype=np.int32)
        flags = np.zeros((n_pairs, max(max_pts, 1)), dtype=np.int8)
        check(lib().cusift_register_rgbd_batch(self.handle, d_points, d_counters, n_images, max_pts, d_depth, w, h,
                                               pitch, image_stride, C.byref(camera), pairs.ctypes.data, n_pairs,
                                               distance, score_threshold, ambiguity_threshold, int(loops),
                                               float(thresh2), RIGID_KINDS[kind], _seed64(seed),
                                               rt.ctypes.data, n_match.ctypes.data, n_in.ctypes.data, sel.ctypes.data,
                                               flags.ctypes.data))
        return (rt, n_match, n_in, [sel[p, :n_match[p]].copy() for p in range(n_pairs)],
                [flags[p, :n_match[p]].astype(bool) for p in range(n_pairs)])

    def register_planar_batch(self, d_points, d_counters, n_images, max_pts, pairs, distance=1, rule=None, lo=None,
                              hi=None, loops=10000, thresh=5.0, refine_loops=5, refine_thresh=3.0, seed=0,
                              want_inliers=True, want_errors=False):
        """cusift_register_planar_batch: register_planar for every pair of `pairs` (int32 [P, 2]) over
        d_points[n_images][max_pts] + d_counters[n_images] (None: max_pts each) in a fixed number of launches and one
        synchronisation.  Pair p = (a, b) maps frame a onto frame b and draws from seed + p; the records are not written.
        rule / lo / hi default as in register_planar.  Returns a PlanarBatchResult."""
        pairs = pair_list(pairs)
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        return PlanarBatchResult(*self._batch(lambda *out: lib().cusift_register_planar_batch(
            self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data, len(pairs), distance, rule, lo, hi,
            int(loops), thresh, refine_loops, refine_thresh, _seed64(seed), *out), (9,), pairs, max_pts, want_inliers,
            want_errors, np.float32))

    def _batch(self, call, shape, pairs, max_pts, want_inliers, want_errors, dtype=np.float64):
        """The outputs that the pair-list forms share: call(*pointers) makes the library call with the eight shared
        output pointers; dtype: of the model's values.  Returns the nine fields of a PlanarBatchResult /
        EpipolarBatchResult / PnPBatchResult."""
        n_pairs = len(pairs)
        model, ransac = np.zeros((n_pairs,) + shape, dtype=dtype), np.zeros((n_pairs,) + shape, dtype=dtype)
        n_cand, n_match, n_fit, best = (np.zeros(n_pairs, dtype=np.int32) for _ in range(4))
        # the call writes 0 / 1 into the first count entries of a pair's block and nothing behind them
        flags = np.full((n_pairs, max(max_pts, 1)), -1, dtype=np.int8)
        err = np.full((n_pairs, max(max_pts, 1)), np.nan, dtype=np.float32) if want_errors else None
        check(call(model.ctypes.data, ransac.ctypes.data, n_cand.ctypes.data, n_match.ctypes.data, n_fit.ctypes.data,
                   best.ctypes.data, flags.ctypes.data, err.ctypes.data if want_errors else None))
        counts = (flags >= 0).sum(axis=1).astype(np.int32) if max_pts > 0 else np.zeros(n_pairs, dtype=np.int32)
        return (model, ransac, n_cand, n_match, n_fit, best, counts,
                [flags[p, :counts[p]] == 1 for p in range(n_pairs)] if want_inliers else None,
                [err[p, :counts[p]].copy() for p in range(n_pairs)] if want_errors else None)

    def register_epipolar_batch(self, d_points, d_counters, n_images, max_pts, pairs, distance=1, rule=None, lo=None,
                                hi=None, loops=10000, thresh=1.0, refine_loops=5, refine_thresh=1.0, seed=0,
                                want_inliers=True, want_errors=False):
        """cusift_register_epipolar_batch: register_epipolar for every pair of `pairs` (int32 [P, 2]) over
        d_points[n_images][max_pts] + d_counters[n_images] (None: max_pts each) in a fixed number of launches and one
        synchronisation.  Pair p = (a, b) gives x_b^T F x_a = 0 and draws from seed + p; the records are not written.
        rule / lo / hi default as in register_planar.  Returns an EpipolarBatchResult."""
        pairs = pair_list(pairs)
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        return EpipolarBatchResult(*self._batch(lambda *out: lib().cusift_register_epipolar_batch(
            self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data, len(pairs), distance, rule, lo, hi,
            int(loops), thresh, refine_loops, refine_thresh, _seed64(seed), *out), (9,), pairs, max_pts, want_inliers,
            want_errors))

    def register_pose_batch(self, d_points, d_counters, n_images, max_pts, pairs, camera, camera2=None, distance=1,
                            rule=None, lo=None, hi=None, loops=10000, thresh=1.0, refine_loops=5, refine_thresh=1.0,
                            seed=0, want_inliers=True, want_errors=False, want_points=False):
        """cusift_register_pose_batch: register_pose for every pair of `pairs`, as register_epipolar_batch and then the
        pose stage at refine_thresh per pair -- still one synchronisation.  camera: the capi.Camera of every pair's frame
        a, camera2 of its frame b (None: the same).  The triangulated points do not go into coords3D (the records are not
        written): want_points returns them.  Returns a PoseBatchResult: X_a = R X_b + t with |t| = 1 PER PAIR, so
        capi.chain_poses does not apply -- the scale of each pair is its own."""
        pairs = pair_list(pairs)
        n_pairs = len(pairs)
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        rt, sigma = np.zeros((n_pairs, 3, 4), dtype=np.float64), np.zeros((n_pairs, 3), dtype=np.float64)
        front, votes = np.zeros(n_pairs, dtype=np.int32), np.zeros((n_pairs, 4), dtype=np.int32)
        xyz = np.zeros((n_pairs, max(max_pts, 1), 3), dtype=np.float32) if want_points else None
        epi = self._batch(lambda *out: lib().cusift_register_pose_batch(
            self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data, n_pairs, distance, rule, lo, hi,
            int(loops), thresh, refine_loops, refine_thresh, _seed64(seed),
            C.byref(camera) if camera is not None else None, C.byref(camera2) if camera2 is not None else None,
            *(out + (rt.ctypes.data, front.ctypes.data, votes.ctypes.data, sigma.ctypes.data,
                     xyz.ctypes.data if want_points else None))), (9,), pairs, max_pts, want_inliers, want_errors)
        counts = epi[6]
        return PoseBatchResult(*(epi + (rt, front, votes, sigma,
                                        [xyz[p, :counts[p]].copy() for p in range(n_pairs)] if want_points else None)))

    def register_pnp_batch(self, d_points, d_counters, n_images, max_pts, pairs, camera2, distance=1, rule=None, lo=None,
                           hi=None, loops=10000, thresh=2.0, refine_loops=5, refine_thresh=2.0, seed=0,
                           want_inliers=True, want_errors=False):
        """cusift_register_pnp_batch: register_pnp for every pair of `pairs`: coords3D of frame a's records (lift_depth
        over the batch, or the caller's; read, never written) against their matches' pixels in frame b, whose capi.Camera
        is camera2 for every pair.  One synchronisation; pair p draws from seed + p.  Returns a PnPBatchResult: X_a = R X_b
        + t in the unit of coords3D -- metric after a depth lift, so capi.chain_poses composes the default pair list's
        rt."""
        pairs = pair_list(pairs)
        rule, lo, hi = _rule_defaults(distance, rule, lo, hi)
        return PnPBatchResult(*self._batch(lambda *out: lib().cusift_register_pnp_batch(
            self.handle, d_points, d_counters, n_images, max_pts, pairs.ctypes.data, len(pairs), distance, rule, lo, hi,
            C.byref(camera2) if camera2 is not None else None, int(loops), thresh, refine_loops, refine_thresh,
            _seed64(seed), *out), (3, 4), pairs, max_pts, want_inliers, want_errors))

    # ---- drivers ----
    def extract_batch(self, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters):
        check(lib().cusift_extract_batch(self.handle, d_imgs, n_images, w, h, pitch, image_stride, C.byref(params),
                                         d_points, d_counters))

    def describe_batch(self, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters=None, flags=0):
        """cusift_describe_batch: orientation + descriptor of the caller's records, in place (asynchronous).  Image i has
        min(d_counters[i], max_pts) records, max_pts with d_counters=None; flags: DESCRIBE_KEEP_ORIENTATION,
        DESCRIBE_OCTAVE_FROM_SCALE."""
        check(lib().cusift_describe_batch(self.handle, d_imgs, n_images, w, h, pitch, image_stride, C.byref(params),
                                          d_points, d_counters, int(flags)))

    def second_orientations(self, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters, ratio=0.8,
                            flags=0):
        """cusift_second_orientations_batch: behind image i's min(d_counters[i], max_pts) records, a duplicate of every
        record whose orientation histogram has a second peak above `ratio` of the first -- the parent's bytes with that
        peak's orientation and the descriptor at it -- in ascending parent index, cut at max_pts; d_counters (uint32 [n],
        required) is updated.  The records must have been described on this image (extract_batch, describe_batch);
        flags: DESCRIBE_OCTAVE_FROM_SCALE.  Asynchronous."""
        ratio = check_second_orientation(ratio, allow_off=False)
        if not d_counters:
            raise ValueError("second_orientations: the counters are read and written, None given")
        check(lib().cusift_second_orientations_batch(self.handle, d_imgs, n_images, w, h, pitch, image_stride,
                                                     C.byref(params), d_points, d_counters, ratio, int(flags)))

    # ---- feature tracks of a sequence ----
    def build_tracks(self, d_counters, n_images, max_pts, pairs, d_rows, d_track, d_offsets, d_obs, d_stats,
                     d_rows_back=None, d_keep=None, rule=1, lo=None, hi=None, min_views=2):
        """cusift_build_tracks: the connected components of the match graph that `pairs` (int32 [P, 2]) and d_rows[P]
        [max_pts] of MatchRow span over the records of a batch, as tracks.  A row is an edge when it passes `rule`
        (0: score > lo && ambiguity < hi; 1: score < lo^2 && ambiguity < hi^2), d_keep (uint8 [P][max_pts], None: all) and
        the cross-check against d_rows_back (None: off); a component is a track when it has min_views nodes and no two
        in one frame.  Device outputs: d_track int32 [n_images][max_pts], d_offsets int32 [N // 2 + 1], d_obs int32 [N],
        d_stats uint32 [8] with N = n_images * max_pts.  lo / hi default as in register_planar.  Asynchronous, nothing is
        read back."""
        pairs = pair_list(pairs)
        rule, lo, hi = _rule_defaults(1, rule, lo, hi)
        check(lib().cusift_build_tracks(self.handle, d_counters, n_images, max_pts, pairs.ctypes.data, len(pairs), d_rows,
                                        d_rows_back, d_keep, rule, lo, hi, min_views, d_track, d_offsets, d_obs, d_stats))

    def triangulate_tracks(self, d_points, n_images, max_pts, d_offsets, d_obs, d_stats, max_tracks, poses, camera,
                           d_points3d, d_front, min_pivot=1e-12):
        """cusift_triangulate_tracks: the point nearest to all pixel rays of every track (fp64), d_points3d float64
        [max_tracks][4] = (X, Y, Z, largest reprojection error in pixels) and d_front int32 [max_tracks] = members in
        front of their camera; four zeros and 0 for a degenerate track (a pivot not > min_pivot: pass 1 - cos(angle) for a
        two-view parallax limit).  poses: [n_images, 4, 4] (chain_poses) or [n_images, 3, 4], camera to world; camera: one
        Camera for all frames.  Asynchronous; poses is read before the call returns."""
        poses = track_poses(poses, n_images)
        check(lib().cusift_triangulate_tracks(self.handle, d_points, n_images, max_pts, d_offsets, d_obs, d_stats,
                                              max_tracks, poses.ctypes.data, C.byref(camera), min_pivot, d_points3d,
                                              d_front))

    def bundle_adjust(self, d_points, n_images, max_pts, d_offsets, d_obs, d_stats, max_tracks, poses, camera,
                      d_points3d, d_poses, d_history, d_summary, fixed=None, params=None, **fields):
        """cusift_bundle_adjust: Schur-complement Levenberg-Marquardt over the poses and the track points (fp64, on the
        device, decisions included).  poses: [n_images, 4, 4] (chain_poses) or [n_images, 3, 4], camera to world; fixed:
        per-frame flags of the frames that must not move (None: frame 0); params: a BundleParams, or its fields as
        keywords (iterations, lam, lambda_min, lambda_max, huber, max_error, min_decrease).  d_points3d float64
        [max_tracks][4] is read (triangulate_tracks' rows) and written; d_poses float64 [n_images][12], d_history
        float64 [iterations][4] = (cost, trial cost, lambda, 1 accepted / 0 rejected / 2 not run) and d_summary
        float64 [8] = (entry cost, final cost, accepted, run, used tracks, used observations, free frames, lambda) are
        written.  Asynchronous; poses and fixed are read before the call returns.  Returns the BundleParams used."""
        poses = track_poses(poses, n_images)
        if params is None:
            params = BundleParams(**fields)
        elif fields:
            raise TypeError("bundle_adjust: params and keyword fields together")
        h_fixed = None
        if fixed is not None:
            fixed = np.ascontiguousarray(np.asarray(fixed).astype(bool), dtype=np.uint8).reshape(-1)
            if fixed.size != n_images:
                raise ValueError("bundle_adjust: %d fixed flags for %d frames" % (fixed.size, n_images))
            h_fixed = fixed.ctypes.data
        check(lib().cusift_bundle_adjust(self.handle, d_points, n_images, max_pts, d_offsets, d_obs, d_stats, max_tracks,
                                         poses.ctypes.data, h_fixed, C.byref(camera), C.byref(params), d_points3d,
                                         d_poses, d_history, d_summary))
        return params

    def describe(self, image, keypoints, keep_orientation=None, **params):
        """SIFT descriptors at the caller's keypoints (blocking, host arrays): `image` float [h, w], `keypoints` [n, 3]
        (x, y, scale) or [n, 4] (+ orientation in degrees) in image pixels.  Four columns keep the given orientations
        unless keep_orientation=False; the octave of each keypoint comes from its scale.  Returns n records
        (SIFT_POINT_DTYPE) in the caller's order; a keypoint that is not finite, or whose scale is not positive, comes
        back with a zero descriptor and subsampling 0.  **params: default_params' fields (num_octaves, root_sift,
        upsample, ...)."""
        img = np.ascontiguousarray(image, dtype=np.float32)
        kp = np.asarray(keypoints, dtype=np.float32)
        if img.ndim != 2 or kp.ndim != 2 or kp.shape[1] not in (3, 4):
            raise ValueError("describe: image [h, w] and keypoints [n, 3] or [n, 4], got %r and %r" % (img.shape, kp.shape))
        if keep_orientation is None:
            keep_orientation = kp.shape[1] == 4
        if keep_orientation and kp.shape[1] != 4:
            raise ValueError("describe: keep_orientation needs a fourth column of orientations")
        n = len(kp)
        recs = np.zeros(n, dtype=SIFT_POINT_DTYPE)
        recs["coords2D"] = kp[:, :2]
        recs["scale"] = kp[:, 2]
        if kp.shape[1] == 4:
            recs["orientation"] = kp[:, 3]
        if n == 0:
            return recs
        h, w = img.shape
        prm = default_params(**dict(params, max_pts=n))
        d_img, d_pts = DeviceBuffer.from_numpy(self, img), DeviceBuffer.from_numpy(self, recs)
        try:
            self.describe_batch(d_img.ptr, 1, w, h, w, h * w, prm, d_pts.ptr, None,
                                DESCRIBE_KEEP_ORIENTATION if keep_orientation else 0)
            self.synchronize()
            return d_pts.to_numpy(SIFT_POINT_DTYPE, (n,))
        finally:
            d_img.free()
            d_pts.free()

    def record_graph(self, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters):
        """cusift_graph_create: extract_batch for fixed buffers, recorded once as a hipGraph (see ExtractGraph)."""
        return ExtractGraph(self, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters)

    def extract(self, d_img, w, h, pitch, params, d_points, h_points=None):
        n = C.c_int(0)
        hp = h_points.ctypes.data if h_points is not None else None
        check(lib().cusift_extract(self.handle, d_img, w, h, pitch, C.byref(params), d_points, hp, C.byref(n)))
        return n.value

    def extract_host(self, img, params, d_points, h_points=None):
        img = np.ascontiguousarray(img, dtype=np.float32)
        h, w = img.shape
        n = C.c_int(0)
        hp = h_points.ctypes.data if h_points is not None else None
        check(lib().cusift_extract_host(self.handle, img.ctypes.data, w, h, C.byref(params), d_points, hp,
                                        C.byref(n)))
        return n.value


UNIQUE_ID_BYTES = 128


def comm_use_library(path=None):
    """cusift_comm_use_library: the library (RCCL, or anything exporting the same nine nccl* entry points) that
    comm_unique_id() / Comm() bind from now on; None = the default search (next to the process's HIP runtime)."""
    check(lib().cusift_comm_use_library(path.encode() if path else None))


def comm_unique_id():
    """cusift_comm_get_unique_id: 128 opaque bytes; rank 0 makes them, every rank passes them to Comm()."""
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    check(lib().cusift_comm_get_unique_id(buf))
    return buf.raw


class Comm:
    """cusift_comm: an RCCL communicator bound to a Context (its device and stream); one process per GPU.
    The all-gatherv of SiftData and the row / halo exchange of the strip tiling (include/cusift_amd.h)."""

    def __init__(self, ctx, unique_id, rank, world, self_p2p=False):
        assert len(unique_id) == UNIQUE_ID_BYTES
        self._h = C.c_void_p()
        self.ctx = ctx  # keeps the context alive
        self.rank, self.world = rank, world
        self._slots = []  # n_images_max of the exchanges in flight, oldest first
        check(lib().cusift_comm_create(C.byref(self._h), ctx.handle, unique_id, rank, world))
        if self_p2p:
            check(lib().cusift_comm_set_self_p2p(self._h, 1))

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            lib().cusift_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def library():
        p = lib().cusift_comm_library()
        return p.decode() if p else ""

    def info(self):
        """cusift_comm_info: what the bound LIBRARY says about this communicator -- {"lib_ranks": ncclCommCount,
        "lib_rank": ncclCommUserRank, "lib_version": ncclGetVersion}; -1 where the library lacks the call."""
        n, r, v = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        check(lib().cusift_comm_info(self._h, C.byref(n), C.byref(r), C.byref(v)))
        return {"lib_ranks": n.value, "lib_rank": r.value, "lib_version": v.value}

    def expand_gathered(self, d_gathered_trimmed, region_cap, totals, d_points):
        """cusift_expand_gathered: regions of 540-byte trimmed records -> regions of 588-byte SiftPoint records, one
        launch on the communicator's stream behind the exchange (asynchronous)."""
        t = np.ascontiguousarray(np.asarray(totals, dtype=np.uint64))
        assert len(t) == self.world
        check(lib().cusift_expand_gathered(self._h, d_gathered_trimmed, region_cap, t.ctypes.data, d_points))

    def reserve(self, n_images_max, tickets=4, stage_records=0):
        check(lib().cusift_comm_reserve(self._h, n_images_max, tickets, stage_records))

    def set_fixed_size(self, on=True):
        check(lib().cusift_comm_set_fixed_size(self._h, 1 if on else 0))

    def set_wire_format(self, fmt=True):
        """fmt: "exact" / "compact" / "trimmed" (or the number; True / False = compact / exact)."""
        if isinstance(fmt, str):
            fmt = WIRE_FORMATS[fmt][0]
        check(lib().cusift_comm_set_wire_format(self._h, int(fmt)))

    def host_waits(self):
        return int(lib().cusift_comm_host_waits(self._h))

    def host_wait_ms(self):
        return float(lib().cusift_comm_host_wait_ms(self._h))

    def hip_syncs(self):
        return int(lib().cusift_comm_hip_syncs(self._h))

    def allgatherv_begin(self, d_points, d_counters, n_images, max_pts, n_images_max, d_gathered, region_cap,
                         producer=None):
        """`producer`: the Context that extracted d_points (the exchange is ordered after it; None: the caller has)."""
        check(lib().cusift_allgatherv_begin(self._h, producer.handle if producer is not None else None, d_points,
                                            d_counters, n_images, max_pts, n_images_max, d_gathered, region_cap))
        self._slots.append(n_images_max)

    def allgatherv_finish(self):
        """Completes the OLDEST begin.  Returns (counts uint32 [world, n_images_max], totals uint64 [world]) -- host
        arrays; rank r's records are d_gathered[r * region_cap : r * region_cap + totals[r]]."""
        if not self._slots:
            raise CusiftError("allgatherv: finish() without begin()")
        counts = np.zeros((self.world, self._slots[0]), dtype=np.uint32)
        totals = np.zeros(self.world, dtype=np.uint64)
        try:
            check(lib().cusift_allgatherv_finish(self._h, counts.ctypes.data, totals.ctypes.data))
        finally:
            self._slots.pop(0)
        return counts, totals

    def allgatherv(self, d_points, d_counters, n_images, max_pts, n_images_max, d_gathered, region_cap, producer=None):
        self.allgatherv_begin(d_points, d_counters, n_images, max_pts, n_images_max, d_gathered, region_cap, producer)
        return self.allgatherv_finish()

    def exchange_rows(self, d_band, pitch, band_rows, ops):
        """ops: list of (peer, send_row, send_rows, recv_row, recv_rows); d_band holds band_rows rows."""
        a = np.ascontiguousarray(np.array(ops, dtype=np.int32).reshape(-1, 5).T)
        n = a.shape[1]
        check(lib().cusift_exchange_rows(self._h, d_band, pitch, band_rows, n, a[0].ctypes.data, a[1].ctypes.data,
                                         a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data))

    def exchange_halos(self, d_band, pitch, top_halo, own_rows, bottom_halo, send_rows):
        check(lib().cusift_exchange_halos(self._h, d_band, pitch, top_halo, own_rows, bottom_halo, send_rows))


def compact_gathered(ctx, d_gathered, region_cap, totals, d_out, capacity):
    """cusift_compact_gathered: the regions of an all-gatherv back to back in rank order (asynchronous on ctx)."""
    t = np.ascontiguousarray(totals, dtype=np.uint64)
    check(lib().cusift_compact_gathered(ctx.handle, d_gathered, region_cap, len(t), t.ctypes.data, d_out, capacity))


def tiled_plan(W, H, world, num_octaves, halo=0, rank=0, octave=0):
    """cusift_tiled_plan (host only): dict of the strip plan's geometry for (rank, octave)."""
    v = [C.c_int(0) for _ in range(9)]
    check(lib().cusift_tiled_plan(W, H, world, num_octaves, halo, rank, octave, *[C.byref(x) for x in v]))
    keys = ("n_octaves", "collapse", "w", "h", "pitch", "own_begin", "own_end", "band_begin", "band_end")
    return dict(zip(keys, (x.value for x in v)))


class Tiled:
    """cusift_tiled: one rank of the strip-tiled extraction of ONE large image (BASELINE configs[4])."""

    def __init__(self, ctx, comm, rank, world, W, H, params, halo=0):
        self._h = C.c_void_p()
        self.ctx, self.comm = ctx, comm  # kept alive
        self.rank, self.world = rank, world
        check(lib().cusift_tiled_create(C.byref(self._h), ctx.handle, comm.handle if comm is not None else None, rank,
                                        world, W, H, C.byref(params), halo))
        v = [C.c_int(0) for _ in range(4)]
        check(lib().cusift_tiled_info(self._h, *[C.byref(x) for x in v]))
        self.n_oct, self.collapse, self.root, self.halo = (x.value for x in v)

    @property
    def handle(self):
        return self._h

    def band(self, octave):
        """(device pointer or None, dict of geometry) of this rank's band of `octave`."""
        ptr = C.c_void_p()
        v = [C.c_int(0) for _ in range(7)]
        check(lib().cusift_tiled_band(self._h, octave, C.byref(ptr), *[C.byref(x) for x in v]))
        keys = ("w", "h", "pitch", "own_begin", "own_end", "band_begin", "band_end")
        return ptr.value, dict(zip(keys, (x.value for x in v)))

    def load(self, d_strip, strip_pitch):
        check(lib().cusift_tiled_load(self._h, d_strip, strip_pitch))

    def build_octave(self, o):
        check(lib().cusift_tiled_build_octave(self._h, o))

    def exchange(self, o):
        check(lib().cusift_tiled_exchange(self._h, o))

    def process(self, d_points, d_counter):
        check(lib().cusift_tiled_process(self._h, d_points, d_counter))

    def extract(self, d_strip, strip_pitch, d_points, d_counter):
        check(lib().cusift_tiled_extract(self._h, d_strip, strip_pitch, d_points, d_counter))

    def check(self, strict=True):
        """Blocking.  Number of keypoints whose footprint left the halo; raises if non-zero and strict."""
        f = C.c_uint(0)
        rc = lib().cusift_tiled_check(self._h, C.byref(f))
        if rc != CUSIFT_OK and (strict or f.value == 0):
            check(rc)
        return f.value

    def close(self):
        if self._h:
            lib().cusift_tiled_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def tiled_exchange_virtual(tiles, octave):
    """cusift_tiled_exchange_virtual: the exchange of `octave` among all ranks' Tiled objects of ONE process."""
    arr = (C.c_void_p * len(tiles))(*[t.handle for t in tiles])
    check(lib().cusift_tiled_exchange_virtual(arr, len(tiles), octave))


class ExtractGraph:
    """A recorded extract_batch (cusift_graph_*): launch() replays all of its kernels with one host call."""

    def __init__(self, ctx, d_imgs, n_images, w, h, pitch, image_stride, params, d_points, d_counters):
        self._g = C.c_void_p()
        self.ctx = ctx  # keeps the context alive
        check(lib().cusift_graph_create(ctx.handle, C.byref(self._g), d_imgs, n_images, w, h, pitch, image_stride,
                                        C.byref(params), d_points, d_counters))

    @property
    def nodes(self):
        return lib().cusift_graph_nodes(self._g)

    def launch(self):
        check(lib().cusift_graph_launch(self._g))

    def close(self):
        if self._g:
            lib().cusift_graph_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def kernel_occupancy(name):
    """(resident workgroups per CU, threads per workgroup) of a named kernel; needs a GPU."""
    n, t = C.c_int(0), C.c_int(0)
    check(lib().cusift_kernel_occupancy(name.encode(), C.byref(n), C.byref(t)))
    return n.value, t.value


def laplace_taps(init_blur):
    taps = np.zeros(8 * 16, dtype=np.float32)
    check(lib().cusift_laplace_taps(init_blur, taps.ctypes.data))
    return taps


class DeviceBuffer:
    """A raw HBM allocation made through the C ABI (cusift_malloc / cusift_free)."""

    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        self.ptr = ctx.malloc(self.nbytes)

    @classmethod
    def from_numpy(cls, ctx, arr):
        arr = np.ascontiguousarray(arr)
        buf = cls(ctx, arr.nbytes)
        ctx.h2d(buf.ptr, arr)
        return buf

    def to_numpy(self, dtype, shape):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes, (out.nbytes, self.nbytes)
        self.ctx.d2h(out, self.ptr)
        return out

    def zero(self):
        self.ctx.memset(self.ptr, 0, self.nbytes)

    def free(self):
        if self.ptr:
            self.ctx.free(self.ptr)
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class HostBuffer:
    """Pinned host memory made through the C ABI (cusift_malloc_host / cusift_free_host): what include/cuSIFT.h's
    SiftData keeps its host records in -- a read-back into it is one DMA, not a staged copy."""

    def __init__(self, nbytes):
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(lib().cusift_malloc_host(C.byref(p), self.nbytes))
        self.ptr = p.value

    def as_numpy(self, dtype, count):
        dtype = np.dtype(dtype)
        assert count * dtype.itemsize <= self.nbytes
        raw = (C.c_char * (count * dtype.itemsize)).from_address(self.ptr)
        return np.frombuffer(raw, dtype=dtype, count=count)  # a view: valid until free()

    def free(self):
        if self.ptr:
            check(lib().cusift_free_host(C.c_void_p(self.ptr)))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


PIPE_U8, PIPE_F32 = 0, 1


class Pipe:
    """cusift_pipe: host frames in, SiftData in pinned host memory out, `depth` batches in flight (C ABI; no torch)."""

    def __init__(self, device, n_images, w, h, params, input_format=PIPE_U8, depth=3, records_capacity=0):
        self._h = C.c_void_p()
        self.n_images, self.w, self.h, self.format = n_images, w, h, input_format
        check(lib().cusift_pipe_create(C.byref(self._h), device, n_images, w, h, C.byref(params), input_format, depth,
                                       records_capacity))

    def submit(self, frames):
        """frames: C-contiguous [n, h, w] uint8 / float32 array (or anything with ctypes.data and the same layout,
        e.g. a pinned torch tensor's numpy view).  It must stay alive and untouched until collected."""
        a = frames
        want = np.uint8 if self.format == PIPE_U8 else np.float32
        assert a.dtype == want and a.ndim == 3 and a.shape[1:] == (self.h, self.w) and a.flags["C_CONTIGUOUS"], a.shape
        check(lib().cusift_pipe_submit(self._h, a.ctypes.data, int(a.shape[0])))

    def collect(self):
        """-> (records: SIFT_POINT_DTYPE view of the pinned slot, offsets [n + 1]); valid until the next collect()."""
        rec, off = C.c_void_p(), C.c_void_p()
        n, total = C.c_int(0), C.c_size_t(0)
        check(lib().cusift_pipe_collect(self._h, C.byref(rec), C.byref(off), C.byref(n), C.byref(total)))
        offsets = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint32)), shape=(n.value + 1,))
        if total.value == 0:
            return np.zeros(0, dtype=SIFT_POINT_DTYPE), offsets
        raw = np.ctypeslib.as_array(C.cast(rec, C.POINTER(C.c_uint8)), shape=(total.value * SIFT_POINT_BYTES,))
        return raw.view(SIFT_POINT_DTYPE), offsets

    def in_flight(self):
        return int(lib().cusift_pipe_in_flight(self._h))

    def close(self):
        if self._h:
            lib().cusift_pipe_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def expand_trimmed(trimmed):
    """cusift_expand_trimmed_host: 540-byte trimmed records -> SiftPoint records (exact; unwritten fields zero)."""
    trimmed = np.ascontiguousarray(trimmed)
    assert trimmed.dtype == TRIMMED_POINT_DTYPE
    out = np.zeros(len(trimmed), dtype=SIFT_POINT_DTYPE)
    check(lib().cusift_expand_trimmed_host(trimmed.ctypes.data, len(trimmed), out.ctypes.data))
    return out


def expand_points(compact):
    """cusift_expand_points_host: COMPACT_POINT_DTYPE array -> SIFT_POINT_DTYPE array (host)."""
    compact = np.ascontiguousarray(compact)
    assert compact.dtype == COMPACT_POINT_DTYPE
    out = np.zeros(len(compact), dtype=SIFT_POINT_DTYPE)
    check(lib().cusift_expand_points_host(compact.ctypes.data, len(compact), out.ctypes.data))
    return out


def sort_points(points):
    """cusift_sort_points_host: canonical order (octave coarsest first, then y, x, scale) of a host SiftPoint array,
    in place; equal point sets give equal arrays."""
    assert points.dtype == SIFT_POINT_DTYPE and points.flags["C_CONTIGUOUS"]
    check(lib().cusift_sort_points_host(points.ctypes.data, len(points)))
    return points


def match_filter(points, score_threshold=999.0, ambiguity_threshold=1.0):
    """The host-side filter of MatchSiftData (extras/matching.cu:318-349, MatchType2D): indices of the points
    whose score < scoreThreshold^2 and ambiguity < ambiguityThreshold^2."""
    t2 = np.float32(score_threshold) * np.float32(score_threshold)
    a2 = np.float32(ambiguity_threshold) * np.float32(ambiguity_threshold)
    return np.nonzero((points["score"] < t2) & (points["ambiguity"] < a2))[0]
