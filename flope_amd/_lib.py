"""ctypes binding of libflope_amd.so (include/flope_amd.h).  Fails loudly when the
library has not been built -- there is deliberately no fallback path."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FLOPE_AMD_LIB") or os.path.join(_HERE, "lib", "libflope_amd.so")   # override: A/B builds only

DT_BF16, DT_F16, DT_F32 = 0, 1, 2
EINVAL = -1                                                                      # FLOPE_EINVAL of include/flope_amd.h
ESTATE = -3                                                                      # FLOPE_ESTATE
IN_F32_NCHW, IN_BF16_NHWC, IN_F16_NHWC, IN_U8_NHWC = 0, 1, 2, 3
TF_ATTN_GENERIC, TF_ATTN_MFMA64, TF_ATTN_TILED, TF_ATTN_F32M = 0, 1, 2, 3     # flope_tf_attention's return (tf_attn_plan.h)
TF_ATTN_MASKED16 = 5                                                           # ... under option mask_mfma where tf_attn_pick_masked picks tf_attn_tiled_masked
TF_ATTN_MASKED = 4                                                             # flope_tf_attention_masked's return
TF_ATTN_BIASED16 = 7                                                           # ... under a compiled bias and option bias_mfma where tf_attn_pick_biased picks tf_attn_tiled_masked, BIASED
TF_ATTN_BIASED = 6                                                             # ... under a compiled bias (flope_tf_bias_create): tf_attn_masked, BIASED
TF_LIN_GENERIC, TF_LIN_ROWWAVE, TF_LIN_ROWWAVE_VEC, TF_LIN_MFMA, TF_LIN_F32M = 0, 1, 2, 3, 4      # flope_tf_linear's return
TF_LIN_SKINNY = 5                                                              # ... under option skinny where tf_gemm_mfma would run on 1 .. 32 rows
TF_LIN_SKINNY_LN = 6                                                           # flope_tf_linear_ln's return: option skinny_ln, a LayerNorm and the skinny linear behind it in one launch
TF_ACT_NONE, TF_ACT_RELU, TF_ACT_GELU = 0, 1, 2                                # flope_tf_linear_act's act, option "activation" 
TF_FWD_LAUNCHES, TF_FWD_FUSED = 0, 1                                          # flope_tf_forward_plan's return
TF_EXTEND_ROW, TF_EXTEND_SPLIT, TF_EXTEND_MFMA = 0, 1, 2                         # flope_tf_stream_extend_plan's / _attention_extend's return
TF_STEP_ROW, TF_STEP_SPLIT = 0, 1                                              # flope_tf_stream_step_plan's / _attention's return
TF_STEP_BIASED, TF_EXTEND_BIASED = 2, 3                                        # ... on a state with a distance table (flope_tf_stream_open_bias)
TF_FEED_SKIPPED, TF_FEED_OVERFLOW, TF_FEED_RANGE, TF_FEED_DUPLICATE, TF_FEED_FULL = -1, -2, -3, -4, -5   # FLOPE_TF_FEED_*: flope_tf_stream_read_feed's codes
TF_FEED_MEAS, TF_FEED_MEAN = 0, 1                                              # flope_tf_stream_step_tracker's source
TF_LN_SCALAR, TF_LN_VEC = 0, 1                                                 # flope_tf_layernorm's return
STAGE_STEM, STAGE_POOL, STAGE_FEAT, STAGE_HIDDEN = 0, 1, 10, 11
HEAD_FC1 = ("packed", "row-major", "simple")                                   # flope_head_plan's *fc1 (plan.h: HeadFc1)
HEAD_FC2 = ("k4", "wave-vector", "wave-scalar")                                # flope_head_plan's *fc2 (plan.h: HeadFc2)


def STAGE_LAYER(li: int, bi: int) -> int:
    return 2 + (li - 1) * 2 + bi


def STAGE_MID(li: int, bi: int) -> int:
    return 12 + (li - 1) * 2 + bi


def STAGE_DS(li: int) -> int:
    return 20 + (li - 2)


# every symbol include/flope_amd.h declares: name -> (restype, argtypes)
_P, _I, _F, _D = C.c_void_p, C.c_int, C.c_float, C.c_double


class TrackView(C.Structure):
    """flope_track_view of include/flope_amd.h (flope_track_device_view)"""
    _fields_ = [("assoc", _P), ("meas", _P), ("means", _P), ("count", _P), ("event", _P), ("device", _I), ("max_tracks", _I), ("max_meas", _I),
                ("n", _I), ("serial", C.c_ulonglong)]


SIGNATURES = {
    "flope_create": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "flope_destroy": (_I, [_P]),
    "flope_last_error": (C.c_char_p, [_P]),
    "flope_load_weights": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_I), C.POINTER(_P)]),
    "flope_forward": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "flope_forward_poses": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _P, _P]),
    "flope_extract_features": (_I, [_P, _P, _I, _I, _P, _P]),
    "flope_procrustes": (_I, [_P, _P, _I, _P]),
    "flope_profile_timeline": (_I, [_P, _P, _P, _I]),
    "flope_nullify_yaw": (_I, [_P, _P, _I, _P]),
    "flope_compose_pose": (_I, [_P, _P, _I, _I, _P, _P]),
    "flope_crop_resize_mask": (_I, [_P, _P, _I, _I, _P, _I, _I, _I, _P, _P]),
    "flope_lanczos4_table": (_I, [_I, _I, _P, _P, _P]),
    "flope_merge_masks_resize": (_I, [_P, _I, _I, _I, _P, _P, _I, _I, _P]),
    "flope_depth_lift": (_I, [_P, _I, _P, _I, _I, _F, _F, _F, _P, _I, C.POINTER(_F), _P, _P, _P, _P, _P]),
    "flope_read_stage": (_I, [_P, _I, _I, _P, C.POINTER(C.c_int64), _P]),
    "flope_set_option": (_I, [_P, C.c_char_p, _I]),
    "flope_debug_read_ws": (_I, [_P, _P, C.c_size_t, C.c_size_t]),
    "flope_debug_pk16": (_I, [_I, _I, _P, _P, _I, _P]),
    "flope_forward_flops": (_D, [_P, _I]),
    "flope_forward_launches": (_I, [_P]),
    "flope_profile_read": (_I, [_P, C.POINTER(_F), _I]),
    "flope_launch_info": (_I, [_P, _I, _I, C.c_char_p, _I, C.POINTER(_D)]),
    "flope_describe_plan": (_I, [_P, C.c_char_p, _I]),
    "flope_version": (C.c_char_p, []),
    "flope_engine_geometry": (_I, [_P, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "flope_head_plan": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "flope_frame_create": (_I, [_P, _I, _I, _I, _I, C.POINTER(_P)]),
    "flope_frame_destroy": (_I, [_P]),
    "flope_frame_last_error": (C.c_char_p, [_P]),
    "flope_frame_select": (_I, [_P, _I, _P, _P, _I, _P]),
    "flope_frame_enqueue": (_I, [_P, _I, _P, _P, _P, _I, _F, C.POINTER(_F), _F, _F, _P]),
    "flope_frame_finish": (_I, [_P, _I, _P, _I]),
    "flope_frame_to_poses": (_I, [_P, _P, _P, _I, _P, _P, _P, _I, _F, C.POINTER(_F), _F, _F, _P, _I, _P]),
    "flope_frame_read_boxes": (_I, [_P, _I, _P, _P, _I]),
    "flope_guard_create": (_I, [_P, _P, _I, _I, C.POINTER(_P)]),
    "flope_guard_destroy": (_I, [_P]),
    "flope_guard_last_error": (C.c_char_p, [_P]),
    "flope_guard_set_gap_min": (_F, [_P, _F]),
    "flope_guard_forward": (_I, [_P, _I, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "flope_guard_repair": (_I, [_P, _I, _P]),
    "flope_guard_forward_repaired": (_I, [_P, _P, _I, _I, _P, _I, _P, _P, _P, _P, _P]),
    "flope_guard_read_selection": (_I, [_P, _I, _P, _I]),
    "flope_guard_select_rows": (_I, [_P, _I, _F, _P, _P, _P]),
    "flope_frame_create_guarded": (_I, [_P, _I, _I, _I, _I, C.POINTER(_P)]),
    "flope_frame_read_gaps": (_I, [_P, _I, _P, _I]),
    # the multi-frame tracker on the device (csrc/track.hip)
    "flope_track_create": (_I, [_I, _I, _I, _D, _D, _D, _D, C.POINTER(_P)]),
    "flope_track_destroy": (_I, [_P]),
    "flope_track_last_error": (C.c_char_p, [_P]),
    "flope_track_reset": (_I, [_P]),
    "flope_track_update": (_I, [_P, _P, _I, _P, _I, _P, _P]),
    "flope_track_count": (_I, [_P]),
    "flope_track_read": (_I, [_P, _P, _P, _P, _P, _I]),
    "flope_track_read_assoc": (_I, [_P, _P, _I]),
    "flope_track_debug_sentinels": (_I, [_P]),
    "flope_track_debug_read": (_I, [_P, _P, _P, _P, _P, _P, _I]),
    "flope_track_device_view": (_I, [_P, _P]),
    "flope_frame_track": (_I, [_P, _I, _P, _P]),
    "flope_stream_create_cu_mask": (_I, [_I, C.POINTER(C.c_uint32), _I, C.POINTER(_P)]),
    "flope_stream_destroy": (_I, [_I, _P]),
    "flope_yolo_create": (_I, [_I, _I, _I, _I, _I, C.POINTER(_P)]),
    "flope_yolo_destroy": (_I, [_P]),
    "flope_yolo_last_error": (C.c_char_p, [_P]),
    "flope_yolo_input_size": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "flope_yolo_load_weights": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_I), C.POINTER(_P)]),
    "flope_yolo_detect": (_I, [_P, _P, _F, _F, _I, _P, _P, _P, _P]),
    "flope_yolo_forward": (_I, [_P, _P, _P]),
    "flope_yolo_postprocess": (_I, [_P, _P, _P, _F, _F, _I, _P, _P, _P, _P]),
    "flope_yolo_read_tensor": (_I, [_P, C.c_char_p, _P, C.POINTER(C.c_int64), _P]),
    "flope_yolo_set_option": (_I, [_P, C.c_char_p, _I]),
    "flope_yolo_op_count": (_I, [_P]),
    "flope_yolo_op_info": (_I, [_P, _I, C.c_char_p, _I]),
    "flope_yolo_forward_ops": (_I, [_P, _P, _I, _P]),
    "flope_yolo_profile": (_I, [_P, _P, _I, C.c_char_p, _I, _P]),
    "flope_yolo_flops": (_D, [_P]),
    "flope_yolo_launches": (_I, [_P]),
    "flope_yolo_graph_cache_size": (_I, [_P]),
    "flope_tf_create": (_I, [_I, _I, _I, _I, _I, _I, _I, _I, _I, C.POINTER(_P)]),
    "flope_tf_destroy": (_I, [_P]),
    "flope_tf_last_error": (C.c_char_p, [_P]),
    "flope_tf_load_weights": (_I, [_P, _I, C.POINTER(C.c_char_p), C.POINTER(_P), C.POINTER(_I), C.POINTER(_P)]),
    "flope_tf_forward": (_I, [_P, _P, _I, _I, _P, _P]),
    "flope_tf_set_option": (_I, [_P, C.c_char_p, _I]),
    "flope_tf_forward_flops": (_D, [_P, _I, _I]),
    "flope_tf_attention": (_I, [_P, _P, _I, _I, _P, _P]),
    "flope_tf_linear": (_I, [_P, C.c_char_p, _P, _I, _P, _P, _I, _I, _I, _P]),
    "flope_tf_linear_act": (_I, [_P, C.c_char_p, _P, _I, _P, _P, _I, _I, _I, _P]),
    "flope_tf_linear_ln_act": (_I, [_P, C.c_char_p, _P, _P, _P, _P, _P, _I, _I, _P]),
    "flope_tf_linear_plan": (_I, [_P, C.c_char_p, _I]),
    "flope_tf_layernorm": (_I, [_P, _P, _P, _P, _P, _I, _P]),
    "flope_tf_linear_ln": (_I, [_P, C.c_char_p, _P, _P, _P, _P, _P, _I, _I, _P]),
    "flope_tf_linear_ln_plan": (_I, [_P, C.c_char_p, _I]),
    "flope_tf_last_ln": (_I, [_P, C.POINTER(_I), C.POINTER(_I)]),
    "flope_tf_forward_varlen": (_I, [_P, _P, _I, _I, C.POINTER(_I), _P, _P]),
    "flope_tf_attention_varlen": (_I, [_P, _P, _I, C.POINTER(_I), _P, _P]),
    "flope_tf_forward_flops_varlen": (_D, [_P, _I, C.POINTER(_I)]),
    "flope_tf_forward_plan": (_I, [_P, _I, _I, C.POINTER(_I)]),
    "flope_tf_last_forward": (_I, [_P]),
    "flope_tf_stream_open": (_I, [_P, _I, _I, C.POINTER(_P)]),
    "flope_tf_stream_open_window": (_I, [_P, _I, _I, _I, C.POINTER(_P)]),
    # ... with a distance table, a relative attention bias [planes][distances]
    "flope_tf_stream_open_bias": (_I, [_P, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(_P)]),
    "flope_tf_stream_bias_planes": (_I, [_P]),
    "flope_tf_stream_close": (_I, [_P]),
    "flope_tf_stream_reset": (_I, [_P, _I, C.POINTER(_I)]),
    "flope_tf_stream_position": (_I, [_P, _I]),
    "flope_tf_stream_step": (_I, [_P, _P, _I, C.POINTER(_I), _P, _P]),
    "flope_tf_stream_prefill": (_I, [_P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), _P, _P]),
    "flope_tf_stream_extend": (_I, [_P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), _P, _P]),
    "flope_tf_stream_step_plan": (_I, [_P]),
    "flope_tf_stream_attention": (_I, [_P, _P, _I, _I, C.POINTER(_I), _P, _P]),
    "flope_tf_stream_extend_plan": (_I, [_P]),
    "flope_tf_stream_attention_extend": (_I, [_P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), _P, _P]),
    # a device-positioned state, stepped by the device tracker's association
    "flope_tf_stream_open_device": (_I, [_P, _I, _I, _I, _I, _I, _I, C.POINTER(C.c_float), C.POINTER(_P)]),
    "flope_tf_stream_step_assoc": (_I, [_P, _P, _P, _P, _I, _P, _P]),
    "flope_tf_stream_step_tracker": (_I, [_P, _P, _I, _P, _P]),
    "flope_tf_stream_reset_device": (_I, [_P, _P]),
    "flope_tf_stream_read_positions": (_I, [_P, _P, _I]),
    "flope_tf_stream_read_feed": (_I, [_P, _P, _P, _I]),
    "flope_tf_stream_read_tokens": (_I, [_P, _P, _I]),
    # scripts/tf_encoder.py: nn.TransformerEncoder.forward(mask=) for any [L, L] mask, compiled once
    "flope_tf_mask_create": (_I, [_P, _I, C.POINTER(C.c_uint32), C.POINTER(_P)]),
    "flope_tf_mask_destroy": (_I, [_P]),
    "flope_tf_mask_info": (_I, [_P, C.POINTER(_I), C.POINTER(C.c_longlong)]),
    "flope_tf_forward_masked": (_I, [_P, _P, _I, _I, C.POINTER(_I), _P, _P, _P]),
    "flope_tf_attention_masked": (_I, [_P, _P, _I, _I, C.POINTER(_I), _P, _P, _P]),
    "flope_tf_forward_flops_masked": (_D, [_P, _I, C.POINTER(_I), _P]),
    "flope_tf_last_forward_masked": (_I, [_P]),
    "flope_tf_mask_tiles": (_I, [_P, C.POINTER(_I)] + [C.POINTER(C.c_longlong)] * 4),
    # ... with a float mask: an additive bias per allowed pair, one plane or one per head
    "flope_tf_bias_create": (_I, [_P, _I, _I, C.POINTER(C.c_float), C.POINTER(_P)]),
    "flope_tf_mask_bias_planes": (_I, [_P]),
}

_lib = None


def load() -> C.CDLL:
    """dlopen the in-tree library and bind every entry point."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles the HIP runtime, and the process must end up with ONE runtime instance -- loading
    # this library before torch left its hipGetDeviceCount without devices (seen with build() then smoke() in one process)
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"flope_amd: {LIB_PATH} is missing -- build it with `make` (or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if a declared symbol is not exported
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def last_error(handle=None) -> str:
    msg = load().flope_last_error(handle)
    return msg.decode() if msg else ""


def check(rc: int, handle=None) -> None:
    if rc != 0:
        raise RuntimeError(f"flope_amd error {rc}: {last_error(handle)}")
