"""ctypes binding of libgemlite_hip.so (C ABI: include/gemlite_hip.h).

This is the ONLY compute backend of the package: there is no eager-PyTorch or CPU fallback.  If the
shared library is missing or a launch is refused, a Python exception is raised (loudly) — the same
exception classes the reference raises for the same conditions (SURVEY.md §8(b) "Errors").
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libgemlite_hip.so")
ABI_VERSION = 1

# status codes (gemlite_status_t)
OK, ERR_BAD_ARGUMENT, ERR_UNSUPPORTED, ERR_BAD_SHAPE, ERR_WORKSPACE, ERR_LAUNCH, ERR_NO_DEVICE, ERR_NO_FUSED_QUANT = 0, -1, -2, -3, -4, -5, -6, -7


class ForwardArgs(C.Structure):
    """struct gemlite_hip_forward_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("matmul_type", C.c_int32),
        ("x", C.c_void_p),
        ("w_q", C.c_void_p),
        ("scales", C.c_void_p),
        ("zeros", C.c_void_p),
        ("scales_x", C.c_void_p),
        ("out", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("M", C.c_int64),
        ("N", C.c_int64),
        ("K", C.c_int64),
        ("W_nbits", C.c_int32),
        ("group_size", C.c_int32),
        ("unpack_mask", C.c_int32),
        ("elements_per_sample", C.c_int32),
        ("w_pack_bits", C.c_int32),
        ("w_dtype", C.c_int32),
        ("input_dtype", C.c_int32),
        ("output_dtype", C.c_int32),
        ("acc_dtype", C.c_int32),
        ("meta_dtype", C.c_int32),
        ("zeros_dtype", C.c_int32),
        ("channel_scale_mode", C.c_int32),
        ("W_group_mode", C.c_int32),
        ("zero_is_scalar", C.c_int32),
        ("data_contiguous", C.c_int32),
        ("type_id", C.c_int32),
        ("stride_xm", C.c_int64),
        ("stride_xk", C.c_int64),
        ("stride_wk", C.c_int64),
        ("stride_wn", C.c_int64),
        ("stride_om", C.c_int64),
        ("stride_on", C.c_int64),
        ("stride_meta_g", C.c_int64),
        ("stride_meta_n", C.c_int64),
        ("stride_sx_m", C.c_int64),
        ("tuning", C.c_int32 * 4),
    ]


class ForwardExt(C.Structure):
    """struct gemlite_hip_forward_ext: the optional extension of a launch (a bias the kernel may add in its epilogue)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("bias_dtype", C.c_int32),
        ("bias", C.c_void_p),
    ]


class QuantizeArgs(C.Structure):
    """struct gemlite_hip_quantize_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("w_dtype", C.c_int32),
        ("w", C.c_void_p),
        ("N", C.c_int64),
        ("K", C.c_int64),
        ("ld_w", C.c_int64),
        ("W_nbits", C.c_int32),
        ("group_size", C.c_int32),
        ("pack_bits", C.c_int32),
        ("meta_dtype", C.c_int32),
        ("q_out", C.c_void_p),
        ("ld_q", C.c_int64),
        ("scales", C.c_void_p),
        ("zeros", C.c_void_p),
        ("stride_meta_g", C.c_int64),
        ("stride_meta_n", C.c_int64),
        ("fold_zeros", C.c_int32),
        ("reserved", C.c_int32),
    ]


class QuantizeHqqArgs(C.Structure):
    """struct gemlite_hip_quantize_hqq_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("iters", C.c_int32),
        ("q", QuantizeArgs),
        ("lp_norm", C.c_float),
        ("beta", C.c_float),
        ("kappa", C.c_float),
        ("reserved", C.c_int32),
    ]


class QuantizeMxArgs(C.Structure):
    """struct gemlite_hip_quantize_mx_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("w_dtype", C.c_int32),
        ("w", C.c_void_p),
        ("N", C.c_int64),
        ("K", C.c_int64),
        ("ld_w", C.c_int64),
        ("format", C.c_int32),
        ("pack_nibbles", C.c_int32),
        ("q_out", C.c_void_p),
        ("ld_q", C.c_int64),
        ("scales", C.c_void_p),
        ("stride_scale_g", C.c_int64),
        ("stride_scale_n", C.c_int64),
        ("reserved", C.c_int64),
    ]


class QuantizeRowsArgs(C.Structure):
    """struct gemlite_hip_quantize_rows_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("w_dtype", C.c_int32),
        ("w", C.c_void_p),
        ("N", C.c_int64),
        ("K", C.c_int64),
        ("ld_w", C.c_int64),
        ("format", C.c_int32),
        ("scale_rule", C.c_int32),
        ("q_out", C.c_void_p),
        ("ld_q", C.c_int64),
        ("scales", C.c_void_p),
        ("stride_s", C.c_int64),
        ("scale_dtype", C.c_int32),
        ("reserved", C.c_int32),
    ]


# form limits of gemlite_hip_quantize_rows (GEMLITE_QUANT_ROWS_WAVE_MAX_K / _RESIDENT_MAX_K of the header): the longest row, in elements,
# that one wave takes, and the longest that one block reads once
QUANT_ROWS_WAVE_MAX_K = 1024
QUANT_ROWS_RESIDENT_MAX_K = 16384


class DequantizeArgs(C.Structure):
    """struct gemlite_hip_dequantize_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("out_dtype", C.c_int32),
        ("w_q", C.c_void_p),
        ("scales", C.c_void_p),
        ("zeros", C.c_void_p),
        ("out", C.c_void_p),
        ("N", C.c_int64),
        ("K", C.c_int64),
        ("stride_wk", C.c_int64),
        ("stride_wn", C.c_int64),
        ("stride_meta_g", C.c_int64),
        ("stride_meta_n", C.c_int64),
        ("ld_out", C.c_int64),
        ("W_nbits", C.c_int32),
        ("group_size", C.c_int32),
        ("elements_per_sample", C.c_int32),
        ("w_pack_bits", C.c_int32),
        ("w_dtype", C.c_int32),
        ("input_dtype", C.c_int32),
        ("meta_dtype", C.c_int32),
        ("zeros_dtype", C.c_int32),
        ("zero_is_scalar", C.c_int32),
        ("W_group_mode", C.c_int32),
        ("channel_scale_mode", C.c_int32),
        ("post_scale", C.c_float),
        ("reserved", C.c_int64),
    ]


class ExpertsArgs(C.Structure):
    """struct gemlite_hip_experts_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("ids_dtype", C.c_int32),
        ("layer", ForwardArgs),
        ("ids", C.c_void_p),
        ("bias", C.c_void_p),
        ("n_slots", C.c_int64),
        ("n_experts", C.c_int64),
        ("slots_per_x_row", C.c_int64),
        ("stride_expert_w", C.c_int64),
        ("stride_expert_meta", C.c_int64),
        ("stride_expert_bias", C.c_int64),
        ("stride_x_row", C.c_int64),
        ("stride_out_slot", C.c_int64),
        ("reserved", C.c_int64 * 2),
    ]


class ExpertsFusedArgs(C.Structure):
    """struct gemlite_hip_experts_fused_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("epilogue", C.c_int32),
        ("experts", ExpertsArgs),
        ("activation", C.c_int32),
        ("weights_dtype", C.c_int32),
        ("weights", C.c_void_p),
        ("slots_per_token", C.c_int64),
        ("reserved", C.c_int64 * 3),
    ]


class ExpertsRowsArgs(C.Structure):
    """struct gemlite_hip_experts_rows_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("rows_per_block", C.c_int32),
        ("experts", ExpertsArgs),
        ("workspace", C.c_void_p),
        ("workspace_bytes", C.c_uint64),
        ("reserved", C.c_int64 * 2),
    ]


class ExpertsRowsGluArgs(C.Structure):
    """struct gemlite_hip_experts_rows_glu_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("activation", C.c_int32),
        ("rows", ExpertsRowsArgs),
        ("reserved", C.c_int64 * 2),
    ]


class ExpertsCombineArgs(C.Structure):
    """struct gemlite_hip_experts_combine_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("dtype", C.c_int32),
        ("ids_dtype", C.c_int32),
        ("weights_dtype", C.c_int32),
        ("y", C.c_void_p),
        ("ids", C.c_void_p),
        ("weights", C.c_void_p),
        ("out", C.c_void_p),
        ("n_slots", C.c_int64),
        ("n_experts", C.c_int64),
        ("slots_per_token", C.c_int64),
        ("N", C.c_int64),
        ("stride_y_slot", C.c_int64),
        ("stride_out_token", C.c_int64),
        ("reserved", C.c_int64 * 2),
    ]


class ExpertsTopkArgs(C.Structure):
    """struct gemlite_hip_experts_topk_args (field order/types must match the header)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("logits_dtype", C.c_int32),
        ("ids_dtype", C.c_int32),
        ("weights_dtype", C.c_int32),
        ("scoring", C.c_int32),
        ("renormalize", C.c_int32),
        ("scale", C.c_float),
        ("reserved0", C.c_int32),
        ("logits", C.c_void_p),
        ("bias", C.c_void_p),
        ("ids", C.c_void_p),
        ("weights", C.c_void_p),
        ("n_tokens", C.c_int64),
        ("n_experts", C.c_int64),
        ("top_k", C.c_int64),
        ("stride_logits_token", C.c_int64),
        ("reserved", C.c_int64 * 2),
    ]


EXPERTS_TOPK_MAX_EXPERTS = 1024  # GEMLITE_EXPERTS_TOPK_MAX_EXPERTS of the header
EXPERTS_TOPK_SOFTMAX, EXPERTS_TOPK_SIGMOID = 0, 1  # gemlite_hip_experts_topk_args.scoring
EXPERTS_ROWS_MAX_EXPERTS = 4096  # GEMLITE_EXPERTS_ROWS_MAX_EXPERTS of the header
EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN = 64  # GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN of the header
EXPERTS_GLU, EXPERTS_COMBINE, ACT_SILU = 1, 2, 1  # gemlite_hip_experts_fused_args.epilogue / .activation
BIAS_NOT_ADDED = 1  # gemlite_hip_forward_ex: launched without the bias, the caller adds it

_lib = None
_lib_lock = threading.Lock()


class GemliteHipError(RuntimeError):
    pass


def load():
    """Load (once) and return the shared library; raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise GemliteHipError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gemlite_amd/csrc`.  gemlite_amd has no non-HIP fallback."
            )
        lib = C.CDLL(LIB_PATH)
        lib.gemlite_hip_abi_version.restype = C.c_int
        lib.gemlite_hip_build_info.restype = C.c_char_p
        lib.gemlite_hip_status_string.restype = C.c_char_p
        lib.gemlite_hip_status_string.argtypes = [C.c_int]
        lib.gemlite_hip_last_hip_error.restype = C.c_int
        for name in ("gemlite_hip_query", "gemlite_hip_forward"):
            getattr(lib, name).restype = C.c_int
        lib.gemlite_hip_query.argtypes = [C.POINTER(ForwardArgs)]
        lib.gemlite_hip_forward.argtypes = [C.POINTER(ForwardArgs), C.c_void_p]
        lib.gemlite_hip_workspace_bytes.restype = C.c_uint64
        lib.gemlite_hip_workspace_bytes.argtypes = [C.POINTER(ForwardArgs)]
        lib.gemlite_hip_kernel_name.restype = C.c_char_p
        lib.gemlite_hip_kernel_name.argtypes = [C.POINTER(ForwardArgs)]
        lib.gemlite_hip_set_profile_events.restype = None
        lib.gemlite_hip_set_profile_events.argtypes = [C.c_void_p, C.c_void_p]
        lib.gemlite_hip_launch_noop.restype = C.c_int
        lib.gemlite_hip_launch_noop.argtypes = [C.c_int32, C.c_int32, C.c_void_p]
        lib.gemlite_hip_capture_group_max.restype = C.c_int
        lib.gemlite_hip_capture_group_max.argtypes = []
        lib.gemlite_hip_capture_group_stats.restype = None
        lib.gemlite_hip_capture_group_stats.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        lib.gemlite_hip_capture_group_compatible.restype = C.c_int
        lib.gemlite_hip_capture_group_compatible.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardArgs)]
        lib.gemlite_hip_capture_group_grid_y.restype = C.c_int
        lib.gemlite_hip_capture_group_grid_y.argtypes = [C.c_int32, C.c_int32]
        lib.gemlite_hip_capture_group_wave_split.restype = None
        lib.gemlite_hip_capture_group_wave_split.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 3)]
        lib.gemlite_hip_capture_group_last_form.restype = C.c_int
        lib.gemlite_hip_capture_group_last_form.argtypes = []
        lib.gemlite_hip_capture_group_geometry.restype = C.c_int
        lib.gemlite_hip_capture_group_geometry.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32 * 4)]
        lib.gemlite_hip_capture_group_tile_of.restype = C.c_int
        lib.gemlite_hip_capture_group_tile_of.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.gemlite_hip_capture_group_lines.restype = C.c_int
        lib.gemlite_hip_capture_group_lines.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.gemlite_hip_capture_group_last_lines.restype = C.c_int
        lib.gemlite_hip_capture_group_last_lines.argtypes = []
        lib.gemlite_hip_capture_group_policy.restype = C.c_int
        lib.gemlite_hip_capture_group_policy.argtypes = [C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32]
        lib.gemlite_hip_k_order_step.restype = C.c_int
        lib.gemlite_hip_k_order_step.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.gemlite_hip_k_order_mode.restype = C.c_int
        lib.gemlite_hip_k_order_mode.argtypes = [C.POINTER(ForwardArgs)]
        lib.gemlite_hip_capture_group_last_policy.restype = C.c_int
        lib.gemlite_hip_capture_group_last_policy.argtypes = []
        lib.gemlite_hip_capture_group_merge_stats.restype = None
        lib.gemlite_hip_capture_group_merge_stats.argtypes = [C.POINTER(C.c_uint64)]
        lib.gemlite_hip_capture_group_rounds_max.restype = C.c_int
        lib.gemlite_hip_capture_group_rounds_max.argtypes = []
        lib.gemlite_hip_capture_group_last_rounds.restype = C.c_int
        lib.gemlite_hip_capture_group_last_rounds.argtypes = []
        lib.gemlite_hip_capture_group_round_member.restype = C.c_int
        lib.gemlite_hip_capture_group_round_member.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        lib.gemlite_hip_capture_group_form.restype = C.c_int
        lib.gemlite_hip_capture_group_form.argtypes = [C.c_int32, C.c_int32, C.c_int64]
        lib.gemlite_hip_capture_group_shared_x_lds_bytes.restype = C.c_int64
        lib.gemlite_hip_capture_group_shared_x_lds_bytes.argtypes = [C.c_int64]
        lib.gemlite_hip_forward_ex.restype = C.c_int
        lib.gemlite_hip_forward_ex.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.c_void_p]
        lib.gemlite_hip_bias_fused.restype = C.c_int
        lib.gemlite_hip_bias_fused.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt)]
        lib.gemlite_hip_kernel_name_ex.restype = C.c_char_p
        lib.gemlite_hip_kernel_name_ex.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt)]
        lib.gemlite_hip_capture_group_compatible_ex.restype = C.c_int
        lib.gemlite_hip_capture_group_compatible_ex.argtypes = [C.POINTER(ForwardArgs), C.POINTER(ForwardExt), C.POINTER(ForwardArgs),
                                                                 C.POINTER(ForwardExt)]
        lib.gemlite_hip_scale_activations_per_token.restype = C.c_int
        lib.gemlite_hip_scale_activations_per_token.argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
        for name in ("gemlite_hip_scale_activations_mxfp8", "gemlite_hip_scale_activations_mxfp4",
                     "gemlite_hip_scale_activations_nvfp4"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                           C.c_void_p]
        lib.gemlite_hip_pack_over_cols.restype = C.c_int
        lib.gemlite_hip_pack_over_cols.argtypes = [
            C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
        lib.gemlite_hip_unpack_over_cols.restype = C.c_int
        lib.gemlite_hip_unpack_over_cols.argtypes = [
            C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
        lib.gemlite_hip_quantize_groups.restype = C.c_int
        lib.gemlite_hip_quantize_groups.argtypes = [C.POINTER(QuantizeArgs), C.c_void_p]
        lib.gemlite_hip_quantize_groups_hqq.restype = C.c_int
        lib.gemlite_hip_quantize_groups_hqq.argtypes = [C.POINTER(QuantizeHqqArgs), C.c_void_p]
        lib.gemlite_hip_quantize_mx.restype = C.c_int
        lib.gemlite_hip_quantize_mx.argtypes = [C.POINTER(QuantizeMxArgs), C.c_void_p]
        lib.gemlite_hip_quantize_rows.restype = C.c_int
        lib.gemlite_hip_quantize_rows.argtypes = [C.POINTER(QuantizeRowsArgs), C.c_void_p]
        lib.gemlite_hip_dequantize.restype = C.c_int
        lib.gemlite_hip_dequantize.argtypes = [C.POINTER(DequantizeArgs), C.c_void_p]
        lib.gemlite_hip_forward_experts.restype = C.c_int
        lib.gemlite_hip_forward_experts.argtypes = [C.POINTER(ExpertsArgs), C.c_void_p]
        lib.gemlite_hip_experts_query.restype = C.c_int
        lib.gemlite_hip_experts_query.argtypes = [C.POINTER(ExpertsArgs)]
        lib.gemlite_hip_forward_experts_fused.restype = C.c_int
        lib.gemlite_hip_forward_experts_fused.argtypes = [C.POINTER(ExpertsFusedArgs), C.c_void_p]
        lib.gemlite_hip_experts_fused_query.restype = C.c_int
        lib.gemlite_hip_experts_fused_query.argtypes = [C.POINTER(ExpertsFusedArgs)]
        lib.gemlite_hip_experts_rows_workspace_bytes.restype = C.c_uint64
        lib.gemlite_hip_experts_rows_workspace_bytes.argtypes = [C.c_int64, C.c_int64, C.c_int32]
        for name in ("gemlite_hip_experts_rows_per_block", "gemlite_hip_experts_rows_query"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [C.POINTER(ExpertsRowsArgs)]
        for name in ("gemlite_hip_experts_route", "gemlite_hip_forward_experts_rows"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [C.POINTER(ExpertsRowsArgs), C.c_void_p]
        for name in ("gemlite_hip_experts_rows_glu_per_block", "gemlite_hip_experts_rows_glu_query"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [C.POINTER(ExpertsRowsGluArgs)]
        lib.gemlite_hip_forward_experts_rows_glu.restype = C.c_int
        lib.gemlite_hip_forward_experts_rows_glu.argtypes = [C.POINTER(ExpertsRowsGluArgs), C.c_void_p]
        lib.gemlite_hip_experts_combine.restype = C.c_int
        lib.gemlite_hip_experts_combine.argtypes = [C.POINTER(ExpertsCombineArgs), C.c_void_p]
        lib.gemlite_hip_experts_combine_query.restype = C.c_int
        lib.gemlite_hip_experts_combine_query.argtypes = [C.POINTER(ExpertsCombineArgs)]
        lib.gemlite_hip_experts_topk.restype = C.c_int
        lib.gemlite_hip_experts_topk.argtypes = [C.POINTER(ExpertsTopkArgs), C.c_void_p]
        lib.gemlite_hip_experts_topk_query.restype = C.c_int
        lib.gemlite_hip_experts_topk_query.argtypes = [C.POINTER(ExpertsTopkArgs)]
        if lib.gemlite_hip_abi_version() != ABI_VERSION:
            raise GemliteHipError("libgemlite_hip.so ABI version mismatch; rebuild it")
        _lib = lib
    return _lib


EXPORTED_SYMBOLS = (
    "gemlite_hip_abi_version", "gemlite_hip_build_info", "gemlite_hip_status_string", "gemlite_hip_last_hip_error",
    "gemlite_hip_query", "gemlite_hip_workspace_bytes", "gemlite_hip_forward", "gemlite_hip_kernel_name",
    "gemlite_hip_set_profile_events", "gemlite_hip_launch_noop", "gemlite_hip_scale_activations_per_token",
    "gemlite_hip_scale_activations_mxfp8", "gemlite_hip_scale_activations_mxfp4", "gemlite_hip_scale_activations_nvfp4",
    "gemlite_hip_pack_over_cols",
    "gemlite_hip_unpack_over_cols",
    "gemlite_hip_capture_group_max", "gemlite_hip_capture_group_stats", "gemlite_hip_capture_group_compatible",
    "gemlite_hip_capture_group_grid_y", "gemlite_hip_capture_group_wave_split",
    "gemlite_hip_capture_group_last_form", "gemlite_hip_capture_group_form", "gemlite_hip_capture_group_shared_x_lds_bytes",
    "gemlite_hip_capture_group_geometry", "gemlite_hip_capture_group_tile_of",
    "gemlite_hip_capture_group_lines", "gemlite_hip_capture_group_last_lines",
    "gemlite_hip_capture_group_policy", "gemlite_hip_capture_group_last_policy",
    "gemlite_hip_capture_group_merge_stats", "gemlite_hip_capture_group_rounds_max", "gemlite_hip_capture_group_last_rounds",
    "gemlite_hip_capture_group_round_member",
    "gemlite_hip_k_order_step", "gemlite_hip_k_order_mode",
    "gemlite_hip_forward_ex", "gemlite_hip_bias_fused", "gemlite_hip_kernel_name_ex", "gemlite_hip_capture_group_compatible_ex",
    "gemlite_hip_quantize_groups", "gemlite_hip_quantize_mx", "gemlite_hip_dequantize", "gemlite_hip_quantize_groups_hqq",
    "gemlite_hip_quantize_rows",
    "gemlite_hip_forward_experts", "gemlite_hip_experts_query",
    "gemlite_hip_forward_experts_fused", "gemlite_hip_experts_fused_query",
    "gemlite_hip_experts_rows_workspace_bytes", "gemlite_hip_experts_rows_per_block", "gemlite_hip_experts_route",
    "gemlite_hip_forward_experts_rows", "gemlite_hip_experts_rows_query",
    "gemlite_hip_forward_experts_rows_glu", "gemlite_hip_experts_rows_glu_query", "gemlite_hip_experts_rows_glu_per_block",
    "gemlite_hip_experts_combine", "gemlite_hip_experts_combine_query",
    "gemlite_hip_experts_topk", "gemlite_hip_experts_topk_query",
)


def forward_ext(bias_ptr: int, bias_dtype: int) -> ForwardExt:
    e = ForwardExt()
    e.struct_size = C.sizeof(ForwardExt)
    e.bias_dtype = int(bias_dtype)
    e.bias = bias_ptr
    return e


def status_string(code: int) -> str:
    return load().gemlite_hip_status_string(int(code)).decode()


def raise_for_status(code: int, what: str):
    """Map a C status to the exception class the reference raises in the same situation."""
    if code == OK:
        return
    msg = f"{what}: {status_string(code)}"
    if code == ERR_UNSUPPORTED or code == ERR_BAD_SHAPE:
        raise NotImplementedError(msg)
    if code == ERR_LAUNCH:
        msg += f" (hipError_t={load().gemlite_hip_last_hip_error()})"
    err = GemliteHipError(msg)
    err.status = code
    raise err


def require_gpu_tensor(t: torch.Tensor, name: str):
    if not t.is_cuda:
        raise GemliteHipError(
            f"gemlite_amd: `{name}` lives on {t.device}; the HIP backend only runs on an MI355X device "
            "(there is deliberately no CPU fallback)")


# ------------------------------------------------------------------------------------------------------
# split-K workspace: one zero-initialised buffer per (device, stream); the kernels leave it zeroed again
# ------------------------------------------------------------------------------------------------------
_workspaces: dict = {}
_ws_lock = threading.Lock()


def workspace(device: torch.device, stream_handle: int, nbytes: int) -> torch.Tensor:
    key = (device.index if device.index is not None else torch.cuda.current_device(), int(stream_handle))
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        with _ws_lock:
            ws = _workspaces.get(key)
            if ws is None or ws.numel() < nbytes:
                size = max(int(nbytes), 1 << 20)
                size = 1 << (size - 1).bit_length()  # grow geometrically
                ws = torch.zeros(size, dtype=torch.uint8, device=device)
                _workspaces[key] = ws
    return ws


class on_device:
    """Context for every ctypes launch: the library launches on the thread's CURRENT device, the tensors may live on another one
    (device_map / model-parallel set-ups move tensors without torch.cuda.set_device).  No-op when they agree."""
    __slots__ = ("_guard",)

    def __init__(self, device: torch.device):
        idx = device.index
        self._guard = torch.cuda.device(idx) if (idx is not None and idx != torch.cuda.current_device()) else None

    def __enter__(self):
        if self._guard is not None:
            self._guard.__enter__()
        return self

    def __exit__(self, *exc):
        if self._guard is not None:
            self._guard.__exit__(*exc)
        return False


def current_stream_handle(device: torch.device) -> int:
    """hipStream_t of torch's current stream on `device`, as an int."""
    return torch.cuda.current_stream(device).cuda_stream  # public API only (the raw private getter saved ~1 us)
