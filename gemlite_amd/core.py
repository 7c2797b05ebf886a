"""GemLiteLinear for MI355X: the reference's module / functional API over the HIP C ABI.

Drop-in surface (reference: gemlite/core.py): ``GemLiteLinear(W_nbits, group_size, in_features,
out_features, input_dtype, output_dtype, acc_dtype, scaled_activations)`` (:231-299), ``.pack(W_q, scales,
zeros, bias, fma_mode, contiguous, packing_bitwidth)`` (:336-519), ``.forward`` / ``.forward_manual`` (:541-557),
``.get_tensor_args`` / ``.get_meta_args`` (:522-538), the ``state_dict`` keys (:503-517, :301-333) and the
functional ``forward_functional(x, bias, tensor_args, meta_args, matmul_type)`` (:128-195).

What is different by design: there is no Triton and no autotuner.  ``forward`` builds one C struct
(`gemlite_hip_forward_args`) and calls ``gemlite_hip_forward`` on the current torch stream; the five
reference kernel families map onto hand-written CDNA4 kernels inside libgemlite_hip.so.  Tensors must live on
the GPU — there is no CPU / eager fallback and a missing library raises.
"""
import bisect
import json
import logging
import os
import threading
from typing import List, Optional, Union

import torch
from torch import Tensor

from . import _hip
from .bitpack import pack_weights_over_cols
from .config import AUTOTUNE, KERNEL, MATMUL_DTYPES, set_autotune, set_kernel_caching  # noqa: F401 (re-exported)
from .dtypes import (DTYPE_TO_TORCH, FP8_INT8_DTYPES, TORCH_TO_DTYPE, DType, is_mx_dtype)
from .quant_utils import (NVFP4_META_SCALE, scale_activations_mxfp4, scale_activations_mxfp8, scale_activations_nvfp4,
                          scale_activations_per_token)

# the name the reference's own test file imports from gemlite.core (tests/test_gemlitelineartriton.py:6; the reference itself no
# longer defines it — SURVEY App. B.7): per-token dynamic quantisation, (x_q, scales_x)
scale_activations = scale_activations_per_token

logger = logging.getLogger(__name__)

# kernel families, in the reference's order: the index is the wire value of `matmul_type`
GEMLITE_MATMUL_TYPES = list(MATMUL_DTYPES)
GEMLITE_MATMUL_TYPES_MAPPING = {name: i for i, name in enumerate(GEMLITE_MATMUL_TYPES)}

# Accumulation dtype recorded in meta_args[7].  The reference picks fp16 accumulation only on a list of
# GeForce parts (core.py:39-54, utils.py:115-122); on an MI355X that resolves to fp32 / int32, which is
# also what the HIP kernels do.
GEMLITE_ACC_DTYPE = {
    DType.FP16: DType.FP32, DType.BF16: DType.FP32, DType.FP32: DType.FP32,
    DType.FP8: DType.FP32, DType.FP8e5: DType.FP32, DType.FP8e4nuz: DType.FP32, DType.FP8e5nuz: DType.FP32,
    DType.INT8: DType.INT32,
    DType.MXFP16: DType.FP32, DType.MXBF16: DType.FP32, DType.MXFP8: DType.FP32, DType.MXFP4: DType.FP32,
    DType.NVFP4: DType.FP32,
}

_CACHE_EPOCH = [0]  # bumped by every mutation of the tuning table: the C++ fast path caches tuning[] per (layer, M) for one epoch


class _EpochDict(dict):
    """A dict that counts its mutations (and those of the family dicts stored in it) in _CACHE_EPOCH — the tuning table is a plain
    module-level dict that load_config(), the autoloader, helper.autotune_layer() and user code all write to directly."""

    def _wrap(self, v):
        return _EpochDict(v) if type(v) is dict else v

    def __setitem__(self, k, v):
        _CACHE_EPOCH[0] += 1
        super().__setitem__(k, self._wrap(v))

    def __delitem__(self, k):
        _CACHE_EPOCH[0] += 1
        super().__delitem__(k)

    def setdefault(self, k, default=None):
        if k not in self:
            self[k] = default
        return self[k]

    def update(self, *a, **kw):
        for k, v in dict(*a, **kw).items():
            self[k] = v

    def clear(self):
        _CACHE_EPOCH[0] += 1
        super().clear()

    def pop(self, *a):
        _CACHE_EPOCH[0] += 1
        return super().pop(*a)

    def popitem(self):
        _CACHE_EPOCH[0] += 1
        return super().popitem()


GEMLITE_HIP_CONFIG_CACHE: dict = _EpochDict()  # tuning hints keyed like the reference's autotune cache
GEMLITE_TRITON_CONFIG_CACHE = GEMLITE_HIP_CONFIG_CACHE  # reference name

# ---- the C++ eager host path (gemlite_amd/csrc_torch/fast_forward.cpp -> gemlite_amd/_fast.so): optional, the ctypes path below is
#      complete without it.  GEMLITE_HIP_NO_FAST_PATH=1 disables it.
try:
    if os.environ.get("GEMLITE_HIP_NO_FAST_PATH"):
        raise ImportError("disabled")
    from . import _fast as _FAST  # noqa: E402
except Exception:  # not built (build() makes it), or a torch it was not built against
    _FAST = None
_FILE_LOCK = threading.Lock()


# ------------------------------------------------------------------------------------------------------
# small setters with the reference's names (core.py:86-97)
# ------------------------------------------------------------------------------------------------------
def _m_buckets():
    vals, i = set(), 0
    while (1 << i) <= 4096:
        v, nxt = 1 << i, 1 << (i + 1)
        vals.add(v)
        if v >= 32 and nxt <= 4096:
            vals.update(((v + nxt) // 2, (v + nxt) // 4))
        i += 1
    return sorted(vals)


_M_BUCKETS = _m_buckets()


def _closest_m_default(M: int) -> int:
    """Round M up to the reference's tuning buckets: powers of two plus the 1/2 and 1/4 interpolations for
    2^i >= 32, capped at 4096 (triton_kernels/utils.py:140-174).  (Table built once: this sits on the per-launch host path.)"""
    if M <= 0:
        return 1  # the reference's table maps 0 to its smallest bucket
    if M >= 4096:
        return 4096
    return _M_BUCKETS[bisect.bisect_left(_M_BUCKETS, M)]


_closest_m = _closest_m_default


def get_closest_m(M: int) -> int:
    return _closest_m(M)


def set_autotune_setting(fct):
    global _closest_m
    _closest_m = fct


def set_packing_bitwidth(packing_bitwidth: int):
    GemLiteLinearHIP.PACKING_BITWIDTH = packing_bitwidth


def set_acc_dtype(dtype):
    assert dtype in [DType.FP16, DType.FP32], "Invalid dtype (should be DType.FP16 or DType.FP32)."
    GEMLITE_ACC_DTYPE[DType.FP16] = dtype  # recorded in meta_args; HIP kernels always accumulate in fp32


def get_default_gemv(W_nbits: int, mx_dtype: bool = False) -> str:
    if mx_dtype:
        return "GEMM_SPLITK"
    return "GEMV_REVSPLITK" if W_nbits < 8 else "GEMV_SPLITK"


def get_matmul_type(batch_size: int, W_nbits: int, mx_dtype: bool = False) -> str:
    """Kernel family by batch size, thresholds as in the reference (core.py:100-114)."""
    if batch_size > 64:
        return "GEMM"
    if batch_size > 1:
        return "GEMM_SPLITK"
    return get_default_gemv(W_nbits, mx_dtype)


# ------------------------------------------------------------------------------------------------------
# launch: tensors + 12 meta ints  ->  gemlite_hip_forward_args  ->  one kernel on the current stream
# ------------------------------------------------------------------------------------------------------
_META_FIELDS = ("scaled_activations", "W_nbits", "group_size", "unpack_mask", "elements_per_sample", "input_dtype",
                "output_dtype", "acc_dtype", "meta_dtype", "channel_scale_mode", "W_group_mode", "data_contiguous")
FUSE_ACT_QUANT_M1 = True  # decode of dynamically quantised layers: activation quantisation fused into the matmul kernel
# 2 <= M <= 64: ONE launch whose first blocks quantise the rows of x while the others stream their weights (csrc/gl_coopquant.h).
# Built, bit-identical to quantiser + matmul, and OFF: an in-launch hand-off on this part is a chain of ~5 dependent device-scope
# memory round trips (row load, write-through drain, flag, poll, first read of the quantised rows: 1-2 us each), a launch boundary
# plus the 2.3-us quantiser is ~4 us — layer(x) measured 3.3-7 us SLOWER fused (profiles/r04/probe_fused_quant_v*.log).
FUSE_ACT_QUANT_ROWS = False
# A bias of the output's 16-bit type is added INSIDE the launch where the library's planner picked a kernel with a biased form (the M = 1
# decode kernel, the 2 .. 64-row kernels): one launch instead of two, bit-identical, and independent biased layers of a stream capture join
# one grouped launch.  False keeps `out += bias` behind every matmul and never asks the library (A/B runs, tests).
FUSE_BIAS = True
TUNING_OVERRIDE = None  # development hook: 4 ints forwarded as gemlite_hip_forward_args.tuning (0 = library default)

# Per-layer launch templates.  A template is the IMMUTABLE byte image of a gemlite_hip_forward_args whose static
# fields (weights, metadata, strides, dtypes, modes) are filled in; every call copies it into a fresh struct and
# adds the per-call fields (x, out, M, strides, scales_x, workspace, tuning) — no shared mutable state, so two
# threads / streams may launch the same layer concurrently.  The key holds EVERY value the template is derived
# from (addresses, shapes, strides, dtypes, numel, device, meta ints): an address reused by the allocator either
# misses, or hits an entry that is correct by construction.
_TEMPLATES: dict = {}
_TEMPLATES_LOCK = threading.Lock()
_SIZEOF_ARGS = _hip.C.sizeof(_hip.ForwardArgs)


def _template_key(W_q: Tensor, scales: Tensor, zeros: Tensor, meta_args) -> tuple:
    return (W_q.data_ptr(), tuple(W_q.shape), W_q.stride(), W_q.dtype, W_q.device.index,
            scales.data_ptr(), tuple(scales.shape), scales.stride(), scales.dtype,
            zeros.data_ptr(), tuple(zeros.shape), zeros.stride(), zeros.dtype, tuple(meta_args))


def _build_template(W_q: Tensor, scales: Tensor, zeros: Tensor, meta_args) -> bytes:
    (_sa, W_nbits, group_size, unpack_mask, e, in_dt, out_dt, acc_dt, meta_dt, c_mode, w_mode, contiguous) = meta_args
    a = _hip.ForwardArgs()
    a.struct_size = _SIZEOF_ARGS
    a.matmul_type = -1
    a.w_q = W_q.data_ptr()
    a.scales = scales.data_ptr() if scales.numel() > 0 else None
    a.zeros = zeros.data_ptr() if zeros.numel() > 0 else None
    a.N = W_q.shape[1]
    a.K = W_q.shape[0] * e
    a.W_nbits, a.group_size, a.unpack_mask, a.elements_per_sample = W_nbits, group_size, unpack_mask, e
    a.w_pack_bits = W_q.element_size() * 8 if e > 1 else 0
    a.w_dtype = TORCH_TO_DTYPE[W_q.dtype].value
    # the output's storage type: MXFP16 / MXBF16 in the output slot (weight-only MX layers) mean fp16 / bf16
    a.input_dtype, a.output_dtype, a.acc_dtype = in_dt, TORCH_TO_DTYPE[DTYPE_TO_TORCH[out_dt]].value, acc_dt
    a.meta_dtype = TORCH_TO_DTYPE[scales.dtype].value if scales.numel() > 0 else meta_dt
    a.zeros_dtype = TORCH_TO_DTYPE[zeros.dtype].value if zeros.numel() > 0 else meta_dt
    a.channel_scale_mode, a.W_group_mode = c_mode, w_mode
    a.zero_is_scalar = int(zeros.numel() == 1)
    a.data_contiguous = int(contiguous)
    base_in = DType.FP16.value if in_dt == DType.BF16.value else (DType.MXFP16.value if in_dt == DType.MXBF16.value else in_dt)
    a.type_id = base_in * 100 + W_nbits
    a.stride_wk, a.stride_wn = W_q.stride(0), W_q.stride(1)
    if is_mx_dtype(in_dt):  # block scales travel as the [N, K/g] transpose of the [K/g, N] buffer (core.py:489-497)
        a.stride_meta_n, a.stride_meta_g = scales.stride(0), scales.stride(1)
    elif scales.dim() == 2 and scales.numel() > 0:
        a.stride_meta_g, a.stride_meta_n = scales.stride(0), scales.stride(1)
    elif zeros.dim() == 2 and zeros.numel() > 1:
        a.stride_meta_g, a.stride_meta_n = zeros.stride(0), zeros.stride(1)
    else:
        a.stride_meta_g, a.stride_meta_n = 0, 1
    return bytes(a)


def _static_args(W_q: Tensor, scales: Tensor, zeros: Tensor, meta_args) -> _hip.ForwardArgs:
    """A FRESH gemlite_hip_forward_args with the layer's static fields filled in (the caller owns it)."""
    key = _template_key(W_q, scales, zeros, meta_args)
    t = _TEMPLATES.get(key)
    if t is None:
        t = _build_template(W_q, scales, zeros, meta_args)
        with _TEMPLATES_LOCK:  # (two threads evicting at once: "dictionary changed size during iteration")
            while len(_TEMPLATES) >= 8192:  # oldest entry out (dicts keep insertion order), not the whole table
                _TEMPLATES.pop(next(iter(_TEMPLATES)), None)
            _TEMPLATES[key] = t
    return _hip.ForwardArgs.from_buffer_copy(t)


def config_key(M: int, N: int, K: int, group_size: int, elements_per_sample: int, type_id: int) -> str:
    """Key of the tuning table, the reference's autotune key (core.py:141-145, triton_kernels `key=[...]`):
    (M bucket, N, K, group_size, elements_per_sample, type_id)."""
    return str((get_closest_m(int(M)), int(N), int(K), int(group_size), int(elements_per_sample), int(type_id)))


def config_family(matmul_type: int, M: int, W_nbits: int, mx: bool = False) -> str:
    """Family name a table entry is filed under: the forced family, or what the reference would pick for M."""
    return GEMLITE_MATMUL_TYPES[matmul_type] if matmul_type >= 0 else get_matmul_type(M, W_nbits, mx)


_TUNING_MASK = (0xFF, 0xFF, 0xFF, 0x3)  # tuning[3]: only the documented x-path bits; development bits are not loadable


def lookup_tuning(matmul_type: int, M: int, a) -> Optional[tuple]:
    """tuning[4] for this launch from GEMLITE_HIP_CONFIG_CACHE (filled by load_config(), the shipped per-GPU table or
    helper.autotune_layer()), or None: the library's own planner decides.  Entries look like
    {"tuning": [t0, t1, t2, t3], "us": 4.5}."""
    if not GEMLITE_HIP_CONFIG_CACHE:
        return None
    fam = GEMLITE_HIP_CONFIG_CACHE.get(config_family(matmul_type, M, a.W_nbits, bool(is_mx_dtype(int(a.input_dtype)))))
    if not fam:
        return None
    entry = fam.get(config_key(M, a.N, a.K, a.group_size, a.elements_per_sample, a.type_id))
    if not entry or "tuning" not in entry:
        return None
    t = (tuple(int(v) for v in entry["tuning"]) + (0, 0, 0, 0))[:4]
    return tuple(v & m for v, m in zip(t, _TUNING_MASK))


def _call_args(x: Tensor, W_q: Tensor, scales: Tensor, zeros: Tensor, scales_x: Optional[Tensor], meta_args, matmul_type: int,
               tuning, raw_x: bool, out_ptr: int, out_strides) -> "_hip.ForwardArgs":
    """The gemlite_hip_forward_args of ONE call: the layer's template + the per-call fields.  Shared by the launch (_hip_matmul) and by
    the planning query in front of it (_library_quantises_inside): both see exactly the same request."""
    a = _static_args(W_q, scales, zeros, meta_args)
    M, K = x.shape
    mx = is_mx_dtype(meta_args[5])
    if mx and x.dtype == torch.uint8:
        K *= 2  # e2m1 codes, two per byte
    if K != a.K:
        raise ValueError(f"x has {K} input features, the packed weight expects {a.K}")
    a.matmul_type = matmul_type
    a.x, a.out, a.M = x.data_ptr(), out_ptr, M
    raw_mx = (mx and raw_x and scales_x is None and x.dtype in (torch.float16, torch.bfloat16) and
              meta_args[5] in (DType.MXFP8.value, DType.MXFP4.value, DType.NVFP4.value))
    if raw_mx:  # one unquantised row of a block-scaled dynamic layer: the kernel quantises it (the layer's format rides in type_id)
        a.input_dtype = TORCH_TO_DTYPE[x.dtype].value
    elif mx:  # the layer's format pair names what x holds (include/gemlite_hip.h "Block-scaled formats")
        if x.dtype != DTYPE_TO_TORCH[meta_args[5]]:
            raise _hip.GemliteHipError(f"{DType(meta_args[5]).name} layer called with {x.dtype} activations")
        a.input_dtype = meta_args[5]
    else:
        a.input_dtype = TORCH_TO_DTYPE[x.dtype].value
    a.stride_xm, a.stride_xk = x.stride(0), x.stride(1)
    a.stride_om, a.stride_on = out_strides
    if scales_x is not None:
        a.scales_x, a.stride_sx_m = scales_x.data_ptr(), scales_x.stride(0)
    if tuning is None:
        tuning = TUNING_OVERRIDE
    if tuning is None:
        tuning = lookup_tuning(matmul_type, M, a)
    if tuning is not None:
        for i in range(4):
            a.tuning[i] = int(tuning[i])
    return a


def _hip_matmul(x: Tensor, W_q: Tensor, scales: Tensor, zeros: Tensor, scales_x: Optional[Tensor], meta_args,
                matmul_type: int, tuning=None, raw_x: bool = False, bias: Optional[Tensor] = None) -> Tensor:
    """out[M, N] = epilogue(x[M, K] @ dequant(W_q)) — the seam the reference fills with
    GEMLITE_TRITON_MAPPING[...].forward (core.py:184-190).  ONE C call per launch: the library plans, carves the
    caller's per-stream workspace and launches; only if that workspace turns out too small is it regrown.
    raw_x: x holds the UNQUANTISED 16-bit rows of a dynamically quantised layer and the kernel quantises them itself (the caller
    asked _library_quantises_inside first).
    bias: added to the result, by the launch itself where the library does that (the caller asked _library_adds_bias first)."""
    lib = _hip.load()
    _hip.require_gpu_tensor(x, "x")
    _hip.require_gpu_tensor(W_q, "W_q")
    if not _AUTOLOAD_DONE:
        autoload_default_config(x.device.index or 0)
    if x.device != W_q.device:
        raise _hip.GemliteHipError(f"x is on {x.device}, the packed weight on {W_q.device}")
    M = x.shape[0]
    out = torch.empty((M, W_q.shape[1]), dtype=DTYPE_TO_TORCH[TORCH_TO_DTYPE[DTYPE_TO_TORCH[meta_args[6]]].value], device=x.device)
    a = _call_args(x, W_q, scales, zeros, scales_x, meta_args, matmul_type, tuning, raw_x, out.data_ptr(), (out.stride(0), out.stride(1)))
    with _hip.on_device(x.device):  # launches go to the tensor's device, not the thread's current one
        stream = _hip.current_stream_handle(x.device)
        ws = _hip.workspace(x.device, stream, 0)
        a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
        if bias is None:
            launch = lambda: lib.gemlite_hip_forward(_hip.C.byref(a), stream)  # noqa: E731
        else:
            ext = _hip.forward_ext(bias.data_ptr(), TORCH_TO_DTYPE[bias.dtype].value)
            launch = lambda: lib.gemlite_hip_forward_ex(_hip.C.byref(a), _hip.C.byref(ext), stream)  # noqa: E731
        rc = launch()
        if rc == _hip.ERR_WORKSPACE:
            need = lib.gemlite_hip_workspace_bytes(_hip.C.byref(a))
            ws = _hip.workspace(x.device, stream, need)
            a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
            rc = launch()
    if rc == _hip.BIAS_NOT_ADDED:  # the launch ran without the bias (the cached answer missed a dependency): add it here, ask again next time
        _FUSED_BIAS_ANSWERS.clear()
        out += bias
        rc = 0
    if rc != 0:
        _hip.raise_for_status(rc, "gemlite_hip_forward")
    # a shape that only the coverage kernel takes is correct but orders of magnitude slower: say so, once per shape
    wkey = (a.N, a.K, a.W_nbits, a.group_size, a.w_pack_bits, a.input_dtype, a.output_dtype, get_closest_m(M), matmul_type)
    if wkey not in _COVERAGE_CHECKED:
        _COVERAGE_CHECKED.add(wkey)
        name = lib.gemlite_hip_kernel_name(_hip.C.byref(a))
        if name and name.startswith((b"generic_matmul_kernel", b"mx_generic_kernel")):
            logger.warning(f"gemlite_amd: no specialised MI355X kernel for N={a.N} K={a.K} W_nbits={a.W_nbits} "
                           f"group_size={a.group_size} packing_bitwidth={a.w_pack_bits} input_dtype={DType(a.input_dtype).name} M={M}: running on the coverage "
                           "kernel (correct, slow).  Group sizes that are a multiple of 32 (K % 256 == 0 for odd multiples) and N % 64 == 0 avoid it; block-scaled "
                           "layers need a K-contiguous W_q (as pack() lays it out), N % 128 == 0 and K % 128 == 0.  8- and 16-bit packing needs 16-bit "
                           "activations, a 4-byte aligned W_q and a power-of-two group size of at least 64 at M >= 2; 32-bit packing "
                           "(set_packing_bitwidth(32)) has the most kernels.")
    return out


# ---- in-launch activation quantisation: ONE source of truth ------------------------------------------------------------
# Whether a kernel takes the UNQUANTISED 16-bit rows of a dynamically quantised layer (per-token int8 / fp8, or block-scaled MXFP8 /
# MXFP4 / NVFP4) is decided in ONE place — resolve() in csrc/plan_forward.hip — and asked through gemlite_hip_query, which plans and never
# launches, on exactly the arguments the launch would carry (_call_args).  Rounds 3-4 kept three hand-written copies of the library's
# preconditions here (alignment, K % 16, K <= 65536, packed / unpacked, one row / several) plus a memo of refusals under a key that
# left out what a refusal depends on.  The answer is cached per everything it depends on: the layer (meta ints, shapes,
# strides, 16-byte alignment of its tensors), M, the activation type and alignment, the device, and the tuning-table epoch (a table
# entry for the shape rides in the query's tuning[] like in the launch's).
_FUSED_QUANT_ANSWERS: dict = {}
_NO_FUSED_QUANT = _FUSED_QUANT_ANSWERS  # (name kept for the tests / scripts that clear it)


def _library_quantises_inside(x2: Tensor, W_q: Tensor, scales: Tensor, zeros: Tensor, meta_args, matmul_type: int) -> bool:
    if matmul_type >= 0 or TUNING_OVERRIDE is not None or x2.dtype not in (torch.float16, torch.bfloat16) or not x2.is_cuda:
        return False  # a forced family / a development override keeps the two-launch form
    M = x2.shape[0]
    if not (FUSE_ACT_QUANT_M1 if M == 1 else FUSE_ACT_QUANT_ROWS):
        return False
    key = (tuple(meta_args), tuple(W_q.shape), W_q.stride(), W_q.dtype, W_q.data_ptr() & 15, scales.data_ptr() & 15, zeros.data_ptr() & 15,
           tuple(scales.shape), scales.stride(), tuple(zeros.shape), zeros.stride(), M, x2.dtype, x2.stride(), x2.data_ptr() & 15,
           x2.device.index, _CACHE_EPOCH[0])
    ans = _FUSED_QUANT_ANSWERS.get(key)
    if ans is None:
        if not _AUTOLOAD_DONE:
            autoload_default_config(x2.device.index or 0)
            key = key[:-1] + (_CACHE_EPOCH[0],)
        a = _call_args(x2, W_q, scales, zeros, None, meta_args, matmul_type, None, True, 0x1000, (W_q.shape[1], 1))
        ans = _hip.load().gemlite_hip_query(_hip.C.byref(a)) == 0
        if len(_FUSED_QUANT_ANSWERS) >= 4096:
            _FUSED_QUANT_ANSWERS.clear()
        _FUSED_QUANT_ANSWERS[key] = ans
    return ans


# ---- bias inside the launch: the same scheme.  resolve() + apply_bias() in csrc/plan_forward.hip decide, gemlite_hip_bias_fused asks them on the
# arguments the launch would carry; the answer is cached per layer / shape / alignment / bias type / tuning epoch.
_FUSED_BIAS_ANSWERS: dict = {}


def _library_adds_bias(x2: Tensor, W_q: Tensor, scales: Tensor, zeros: Tensor, bias: Tensor, meta_args, matmul_type: int) -> bool:
    if not FUSE_BIAS or bias.dtype not in (torch.float16, torch.bfloat16) or bias.dim() != 1 or bias.shape[0] != W_q.shape[1] \
            or not bias.is_contiguous() or bias.device != x2.device or x2.dtype != bias.dtype:
        return False
    M = x2.shape[0]
    key = (tuple(meta_args), tuple(W_q.shape), W_q.stride(), W_q.dtype, W_q.data_ptr() & 15, scales.data_ptr() & 15, zeros.data_ptr() & 15,
           tuple(scales.shape), scales.stride(), tuple(zeros.shape), zeros.stride(), M, x2.dtype, x2.stride(), x2.data_ptr() & 15,
           x2.device.index, bias.dtype, bias.data_ptr() & 15, matmul_type, None if TUNING_OVERRIDE is None else tuple(TUNING_OVERRIDE),
           _CACHE_EPOCH[0])
    ans = _FUSED_BIAS_ANSWERS.get(key)
    if ans is None:
        if not _AUTOLOAD_DONE:
            autoload_default_config(x2.device.index or 0)
            key = key[:-1] + (_CACHE_EPOCH[0],)
        a = _call_args(x2, W_q, scales, zeros, None, meta_args, matmul_type, None, False, 0x1000, (W_q.shape[1], 1))
        ext = _hip.forward_ext(bias.data_ptr(), TORCH_TO_DTYPE[bias.dtype].value)
        ans = _hip.load().gemlite_hip_bias_fused(_hip.C.byref(a), _hip.C.byref(ext)) == 1
        if len(_FUSED_BIAS_ANSWERS) >= 4096:
            _FUSED_BIAS_ANSWERS.clear()
        _FUSED_BIAS_ANSWERS[key] = ans
    return ans


_COVERAGE_CHECKED = set()


def _forward_impl(x: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int],
                  matmul_type: int = -1) -> Tensor:
    W_q, scales, zeros = tensor_args
    W_nbits = meta_args[1]
    out_features = W_q.shape[1]
    if not x.is_contiguous():
        x = x.contiguous()
    out_shape = x.shape[:-1] + (out_features,)
    in_code = meta_args[5]
    scales_x = None
    if bool(meta_args[0]) and (is_mx_dtype(in_code) or DType(in_code) in FP8_INT8_DTYPES):
        # Dynamic activation quantisation (core.py:155-175): per token (int8 / fp8) or per block (MXFP8 / MXFP4 / NVFP4).  Where the library
        # has a kernel that quantises the rows itself — one row: inside the decode kernels, bit-identical to quantiser + matmul; several
        # rows: opt-in, see FUSE_ACT_QUANT_ROWS — the unquantised x goes straight in (ONE launch); the library is the one that knows.
        x2f = x if x.dim() == 2 else x.reshape(-1, x.shape[-1])  # (x is contiguous here: a view)
        if _library_quantises_inside(x2f, W_q, scales, zeros, meta_args, matmul_type):
            # (defensive, ADVICE r5: should a launch still refuse what the query accepted — the answer cache misses a dependency — the
            #  refusal is not an error of the layer: fall through to quantiser + matmul and forget the cached answers)
            try:
                out = _hip_matmul(x2f, W_q, scales, zeros, None, meta_args, matmul_type, raw_x=True)
            except _hip.GemliteHipError as e:
                if getattr(e, "status", None) != _hip.ERR_NO_FUSED_QUANT:
                    raise
                _FUSED_QUANT_ANSWERS.clear()
                out = None
            if out is not None:
                if len(out_shape) != 2:
                    out = out.view(out_shape)
                if bias is not None:
                    out += bias
                return out
        if is_mx_dtype(in_code):
            c_mode = meta_args[9]  # microscales (channel_scale_mode 4) or one fp32 scale per token (2)
            if in_code == DType.MXFP8.value and c_mode == 4:
                x, scales_x = scale_activations_mxfp8(x, w_dtype=torch.float8_e4m3fn)
            elif in_code == DType.MXFP8.value and c_mode == 2:
                x, scales_x = scale_activations_per_token(x, w_dtype=torch.float8_e4m3fn)
            elif in_code == DType.MXFP4.value and c_mode == 4:
                x, scales_x = scale_activations_mxfp4(x)
            elif in_code == DType.NVFP4.value and c_mode == 4:
                x, scales_x = scale_activations_nvfp4(x)
            else:
                raise NotImplementedError(f"no activation quantiser for {DType(in_code).name} with channel_scale_mode {c_mode}")
        else:
            x, scales_x = scale_activations_per_token(x, w_dtype=DTYPE_TO_TORCH[in_code])
    x2 = x if x.dim() == 2 else x.view(-1, x.shape[-1])
    # matmul_type < 0 (auto) is resolved inside the library: the HIP kernel families have their own M
    # thresholds (GEMV <= 4 rows, streaming MFMA above), unlike the Triton ones of get_matmul_type()
    # a bias the planned kernel adds itself rides in the launch (weight-only 16-bit layers; FUSE_BIAS); every other one is added here
    fused = bias is not None and FUSE_BIAS and scales_x is None and _library_adds_bias(x2, W_q, scales, zeros, bias, meta_args, matmul_type)
    out = _hip_matmul(x2, W_q, scales, zeros, scales_x, meta_args, matmul_type, bias=bias if fused else None)
    if len(out_shape) != 2:
        out = out.view(out_shape)
    if bias is not None and not fused:
        out += bias
    return out


@torch.library.custom_op("gemlite::forward_functional", mutates_args=())
def forward_functional(x: Tensor, bias: Optional[Tensor], tensor_args: List[Tensor], meta_args: List[int],
                       matmul_type: int = -1) -> Tensor:
    return _forward_impl(x, bias, tensor_args, meta_args, matmul_type)


@torch.library.register_fake("gemlite::forward_functional")
def _forward_functional_fake(x, bias, tensor_args, meta_args, matmul_type=-1):
    return torch.empty(x.shape[:-1] + (tensor_args[0].shape[1],), device=x.device, dtype=x.dtype)


# ------------------------------------------------------------------------------------------------------
# pack(): which dequant / epilogue modes a given (scales, zeros, activation-scaling) combination selects
# ------------------------------------------------------------------------------------------------------
def select_modes(*, has_scales: bool, channelwise: bool, zeros_kind: str, scaled_activations: bool, fma_mode: bool):
    """-> (W_group_mode, channel_scale_mode, fold_zeros).  Semantics of core.py:408-464, as a decision table.

    W_group_mode:        0 none | 1 q - z | 2 q*s | 3 (q - z)*s | 4 fma(q, s, z')   with z' = -z*s folded at pack time
    channel_scale_mode:  0 none | 1 weight | 2 activation | 3 both (applied after the K reduction)
    """
    assert zeros_kind in ("none", "tensor", "int")
    fold = False
    if channelwise:
        # per-output-channel scales move to the epilogue; inside the K loop only the shift remains
        w_mode = 0 if zeros_kind == "none" else 1
        c_mode = 3 if scaled_activations else 1
        return w_mode, c_mode, fold
    if zeros_kind == "none":
        w_mode = 2 if has_scales else 0
    elif zeros_kind == "tensor":
        if not has_scales:
            w_mode = 1  # shift only (the reference would fail folding zeros without scales)
        elif fma_mode:
            w_mode, fold = 4, True
        else:
            w_mode = 3
    else:
        w_mode = 3 if has_scales else 1
    c_mode = 2 if scaled_activations else 0
    return w_mode, c_mode, fold


class GemLiteLinearHIP(torch.nn.Module):
    SUPPORTED_BITS_TRITON = [1, 2, 4, 8, 16]
    SUPPORTED_DTYPES = [DType.FP16, DType.BF16, DType.FP32, DType.FP8, DType.FP8e4, DType.FP8e5, DType.INT8,
                        DType.MXFP16, DType.MXBF16, DType.MXFP8, DType.MXFP4, DType.NVFP4]
    # accepted by the constructor for API parity, rejected at forward time (MI300X formats, not gfx950's)
    _DEFERRED_DTYPES = [DType.FP8e4nuz, DType.FP8e5nuz]
    MIN_SIZE = 32
    PACKING_BITWIDTH = 32

    def __init__(self, W_nbits=4, group_size=64, in_features=None, out_features=None, input_dtype=DType.FP16,
                 output_dtype=DType.FP16, acc_dtype=None, scaled_activations=False):
        super().__init__()
        if W_nbits not in self.SUPPORTED_BITS_TRITON:
            raise NotImplementedError("Only " + str(self.SUPPORTED_BITS_TRITON) + " W_nbits are supported.")
        if in_features is not None and out_features is not None:
            bad = in_features % self.MIN_SIZE != 0
            if group_size is not None and in_features % group_size != 0:
                bad = True
            if bad:
                raise NotImplementedError(f"Invalid input shapes: {in_features} , {out_features}. "
                                          "in_features should be divisible by 32 or the group_size")
        if input_dtype not in self.SUPPORTED_DTYPES + self._DEFERRED_DTYPES:
            raise NotImplementedError("Unsupport input dtype: " + str(input_dtype))
        if group_size is not None and group_size < 16:
            raise NotImplementedError("Only group_size >= 16 is supported.")

        self.in_features, self.out_features = in_features, out_features
        self.orig_shape = (out_features, in_features)
        self.W_nbits = W_nbits
        self.group_size = 1 if group_size is None else group_size
        self.unpack_mask = 2 ** W_nbits - 1
        self.elements_per_sample = None
        self.signature = (in_features, out_features, W_nbits, self.group_size)
        self.input_dtype, self.output_dtype = input_dtype, output_dtype
        self.compute_dtype = DTYPE_TO_TORCH[input_dtype.value]
        self.meta_dtype = input_dtype
        self.acc_dtype = GEMLITE_ACC_DTYPE[input_dtype] if acc_dtype is None else acc_dtype
        # 16/32-bit float activations are never dynamically quantised (core.py:293-296)
        float_in = self.compute_dtype in (torch.float16, torch.bfloat16, torch.float32)
        self.scaled_activations = False if float_in else bool(scaled_activations)
        self.forward = self.forward_auto_no_warmup

    # ------------------------------------------------------------------------------------------ pack
    def pack(self, W_q: Tensor, scales: Optional[Tensor], zeros: Union[Tensor, int, None], bias: Optional[Tensor] = None,
             fma_mode: bool = True, contiguous: Optional[bool] = None, packing_bitwidth: Optional[int] = None):
        if zeros is not None and self.input_dtype == DType.INT8:
            fractional = isinstance(zeros, float) or (isinstance(zeros, Tensor) and bool((zeros != zeros.round()).any()))
            if fractional:
                raise Exception("INT8 inputs is not compatible with floating-point zeros.")
        if packing_bitwidth is None:
            packing_bitwidth = GemLiteLinearHIP.PACKING_BITWIDTH
        mx = bool(is_mx_dtype(self.input_dtype))
        if mx:
            packing_bitwidth = 8  # microscaling: e2m1 codes two per byte, fp8 unpacked (core.py:363-365)
            if scales is None or zeros is not None:
                raise NotImplementedError("block-scaled formats take (W_q, scales) and no zeros")

        packed = W_q.dtype == torch.uint8
        if packed:
            if mx:  # [N, K/2] bytes, handed on as the [K/2, N] view: K-contiguous per output column
                pk, self.elements_per_sample = pack_weights_over_cols(
                    W_q.view(self.orig_shape), W_nbits=self.W_nbits, packing_bitwidth=packing_bitwidth, transpose=False)
                self.W_q = pk.t()
            else:
                self.W_q, self.elements_per_sample = pack_weights_over_cols(
                    W_q.view(self.orig_shape), W_nbits=self.W_nbits, packing_bitwidth=packing_bitwidth, transpose=True)
            want_contiguous = (not mx) if contiguous is None else bool(contiguous)  # MX: K-contiguous per column (core.py:395-396)
        elif W_q.dtype == torch.int8 or W_q.is_floating_point():
            expect = {torch.float32: 32, torch.float16: 16, torch.bfloat16: 16}.get(W_q.dtype, 8)
            assert self.W_nbits == expect, f"Invalid {expect}-bit weights."
            self.W_q = W_q.t()  # [K, N] view with strides (1, K): K-contiguous per output column
            self.elements_per_sample = 1
            want_contiguous = False if contiguous is None else bool(contiguous)
        else:
            raise Exception("Weights were not packed, please check your W_q.dtype")
        return self._finish_pack(scales, zeros, bias, fma_mode, want_contiguous, mx)

    def _finish_pack(self, scales: Optional[Tensor], zeros: Union[Tensor, int, None], bias: Optional[Tensor], fma_mode: bool,
                     want_contiguous: bool, mx: bool = False, meta_by_group: bool = False):
        """The half of pack() behind the packing: self.W_q / self.elements_per_sample are set; selects the modes, lays the metadata out
        and registers the parameters.  `meta_by_group`: scales / zeros already are [K/g, N] with the zeros folded where the selected
        mode folds them (what the fused quantisers write: WeightQuantizerINT.quantize_packed, and — with `mx`, as block-scale bytes —
        WeightQuantizerMXFP.quantize_packed)."""
        self.device = self.W_q.device
        self.bias = None if bias is None else bias.to(device=self.device)

        N = self.out_features
        zeros_kind = "none" if zeros is None else ("tensor" if isinstance(zeros, Tensor) else "int")
        channelwise = scales is not None and scales.numel() == N
        self.meta_is_channelwise = channelwise
        self.W_group_mode, self.channel_scale_mode, fold = select_modes(
            has_scales=scales is not None, channelwise=channelwise, zeros_kind=zeros_kind,
            scaled_activations=self.scaled_activations, fma_mode=fma_mode)

        def rows_by_group(t: Tensor) -> Tensor:  # [N * K/g (,1)] -> [K/g, N], N fastest
            if meta_by_group:  # (one group: the strides the view below gives a [1, N] tensor)
                return t.view((N, 1)).t() if t.shape[0] == 1 else t
            return t.view((N, -1)).t()

        self.scales = None if scales is None else rows_by_group(scales)
        if zeros_kind == "tensor":
            if fold and not meta_by_group:  # z' = -z * s, computed in fp32 and rounded to the zeros dtype (core.py:433-436)
                zeros = (-zeros.float() * scales.float()).to(zeros.dtype)
            self.zeros = rows_by_group(zeros)
        elif zeros_kind == "int":
            self.zeros = torch.tensor(int(zeros), dtype=torch.int32, device=self.device)
        else:
            self.zeros = None
        if self.channel_scale_mode in (1, 3):
            assert self.W_group_mode not in (3, 4), "Can't use channel_scale_mode with W_group_mode == 3 or 4."

        # absent metadata travels as empty int32 tensors so the functional signature stays List[Tensor]
        if self.zeros is None:
            self.zeros = torch.tensor([[]], dtype=torch.int32, device=self.device)
        if self.scales is None:
            self.scales = torch.tensor([[]], dtype=torch.int32, device=self.device)

        self.data_contiguous = want_contiguous
        if want_contiguous:
            self.W_q = self.W_q.contiguous()
        self.scales = self.scales.contiguous()
        self.zeros = self.zeros.contiguous()
        if mx:
            # one byte per block: e8m0 exponents (NVFP4: e4m3), stored [K/g, N] and handed on as its [N, K/g] transpose;
            # the block scales are part of the contraction, not a group / channel mode (core.py:489-497)
            if self.input_dtype == DType.NVFP4:
                self.scales = self.scales.to(torch.float8_e4m3fn)
            elif self.scales.dtype != torch.uint8:  # uint8 = e8m0 bytes already
                self.scales = self.scales.to(torch.float8_e8m0fnu).view(torch.uint8)
            self.scales = self.scales.T
            self.W_group_mode, self.channel_scale_mode = 2, 0
        self.meta_dtype = TORCH_TO_DTYPE[self.scales.dtype]

        as_param = lambda t: torch.nn.Parameter(t, requires_grad=False)  # noqa: E731
        # registration order = key order of state_dict(): W_q, bias, scales, zeros, metadata, orig_shape (core.py:503-517)
        self.W_q = as_param(self.W_q)
        self.bias = as_param(self.bias) if self.bias is not None else None
        self.scales, self.zeros = as_param(self.scales), as_param(self.zeros)
        self.metadata = as_param(torch.tensor(self.get_meta_args(), device=self.device, dtype=torch.int32))
        self.orig_shape = as_param(torch.tensor([self.out_features, self.in_features], device=self.device,
                                                dtype=torch.int32))
        return self

    # ---------------------------------------------------------------------------------- (de)serialise
    def load_state_dict(self, state_dict, strict=True, assign=False):
        self.W_q = state_dict.pop("W_q", None)
        self.bias = state_dict.pop("bias", None)
        self.scales = state_dict.pop("scales", None)
        self.zeros = state_dict.pop("zeros", None)
        self.metadata = [int(v) for v in state_dict.pop("metadata")]
        self.orig_shape = tuple(int(v) for v in state_dict.pop("orig_shape"))
        for name, val in zip(_META_FIELDS, self.metadata):
            setattr(self, name, val)
        for name in ("input_dtype", "output_dtype", "acc_dtype", "meta_dtype"):
            setattr(self, name, DType(getattr(self, name)))
        self.scaled_activations, self.data_contiguous = bool(self.scaled_activations), bool(self.data_contiguous)
        self.out_features, self.in_features = self.orig_shape
        self.compute_dtype = DTYPE_TO_TORCH[self.input_dtype.value]
        self.signature = (self.in_features, self.out_features, self.W_nbits, self.group_size)
        self.device = self.W_q.device

    # ------------------------------------------------------------------------------------- arguments
    def get_tensor_args(self):
        return [self.W_q, self.scales, self.zeros]

    def get_meta_args(self):
        return [int(self.scaled_activations), self.W_nbits, self.group_size, self.unpack_mask,
                self.elements_per_sample, self.input_dtype.value, self.output_dtype.value, self.acc_dtype.value,
                self.meta_dtype.value, self.channel_scale_mode, self.W_group_mode, int(self.data_contiguous)]

    # ------------------------------------------------------------------------------------ dequantize
    def dequantize(self, dtype: Optional[torch.dtype] = None, out: Optional[Tensor] = None) -> Tensor:
        """The weights this layer multiplies by, as [out_features, in_features] of `dtype` (fp16 / bf16 / fp32; default: the layer's
        16-bit compute type): one `gemlite_hip_dequantize` launch on the current stream, from the stored tensors and metadata only
        (contract: DESIGN §2.3).  For a dynamically quantised layer this is the weight side alone.  `out`: a [out_features, in_features]
        tensor or row-strided view of `dtype` to write into.  GPU layers only, like forward."""
        W_q, scales, zeros = self.get_tensor_args()
        _hip.require_gpu_tensor(W_q, "W_q")
        meta = self.get_meta_args()
        if dtype is None and out is not None:
            dtype = out.dtype
        elif dtype is None:  # the layer's 16-bit compute type: of its activations, or (dynamically quantised layers) of its output
            dtype = DTYPE_TO_TORCH[meta[5]]
            if dtype not in (torch.float16, torch.bfloat16):
                dtype = DTYPE_TO_TORCH[meta[6]]
        if dtype not in (torch.float16, torch.bfloat16, torch.float32):
            raise NotImplementedError(f"dequantize to {dtype}: the result is float16, bfloat16 or float32")
        s = _static_args(W_q, scales, zeros, meta)
        N, K = int(s.N), int(s.K)
        if out is None:
            out = torch.empty((N, K), dtype=dtype, device=W_q.device)
        elif tuple(out.shape) != (N, K) or out.dtype != dtype or out.device != W_q.device or (K > 1 and out.stride(1) != 1):
            raise ValueError(f"out should be a [{N}, {K}] {dtype} tensor on {W_q.device} with unit stride along in_features")
        a = _hip.DequantizeArgs()
        a.struct_size = _hip.C.sizeof(_hip.DequantizeArgs)
        for f in ("w_q", "scales", "zeros", "N", "K", "stride_wk", "stride_wn", "stride_meta_g", "stride_meta_n", "W_nbits", "group_size",
                  "elements_per_sample", "w_pack_bits", "w_dtype", "input_dtype", "meta_dtype", "zeros_dtype", "zero_is_scalar",
                  "W_group_mode", "channel_scale_mode"):
            setattr(a, f, getattr(s, f))
        a.out, a.out_dtype, a.ld_out = out.data_ptr(), TORCH_TO_DTYPE[dtype].value, (out.stride(0) if N > 1 else max(K, out.stride(0)))
        a.post_scale = NVFP4_META_SCALE if meta[5] == DType.NVFP4.value else 1.0  # the fixed second-level scale of an NVFP4 layer
        with _hip.on_device(W_q.device):
            rc = _hip.load().gemlite_hip_dequantize(_hip.C.byref(a), _hip.current_stream_handle(W_q.device))
        _hip.raise_for_status(rc, "gemlite_hip_dequantize")
        return out

    # --------------------------------------------------------------------------------------- forward
    def _call(self, x: Tensor, matmul_type: int) -> Tensor:
        if torch.compiler.is_compiling():
            return forward_functional(x, self.bias, self.get_tensor_args(), self.get_meta_args(), matmul_type)
        return _forward_impl(x, self.bias, self.get_tensor_args(), self.get_meta_args(), matmul_type)

    def forward_manual(self, x: Tensor, matmul_type: str = "GEMM") -> Tensor:
        return self._call(x, GEMLITE_MATMUL_TYPES_MAPPING[matmul_type])

    # The attributes a launch template is derived from: assigning any of them drops the layer's C++ handle (tensors whose storage is
    # replaced in place — module.to(), param.data = ... — are caught inside the C++ call by their data pointers).
    _FAST_FIELDS = frozenset(("W_q", "scales", "zeros", "bias") + _META_FIELDS)

    def __setattr__(self, name, value):
        if name in GemLiteLinearHIP._FAST_FIELDS:
            self.__dict__["_fast"] = None
            self.__dict__["_fast_tried"] = None
        super().__setattr__(name, value)

    def _install_fast(self):
        """Per-layer C++ launch handle for `layer(x)` (weight-only layers with 16-bit activations): (capsule, W_q, scales, zeros, bias)."""
        d = self.__dict__
        d["_fast"] = None
        d["_fast_tried"] = _CACHE_EPOCH[0]
        if _FAST is None or self.W_q is None or not self.W_q.is_cuda or self.elements_per_sample is None:
            return
        meta = self.get_meta_args()
        if meta[0] or meta[5] not in (DType.FP16.value, DType.BF16.value):
            return
        W_q, scales, zeros = self.get_tensor_args()
        cap = _FAST.make(_build_template(W_q, scales, zeros, meta), W_q, scales, zeros, _CACHE_EPOCH[0], not GEMLITE_HIP_CONFIG_CACHE)
        if cap is not None:
            d["_fast"] = (cap, W_q, scales, zeros, self.bias)

    def forward_auto_no_warmup(self, x: Tensor) -> Tensor:
        d = self.__dict__
        f = d.get("_fast")
        if f is not None and TUNING_OVERRIDE is None and not torch.compiler.is_compiling():
            y = _FAST.forward(f[0], f[1], f[2], f[3], x, f[4], -1, _CACHE_EPOCH[0], FUSE_BIAS)
            if y is NotImplemented:  # a tuning table is loaded and this M has not been looked up at this epoch yet
                a = _static_args(f[1], f[2], f[3], self.get_meta_args())
                M = x.numel() // max(1, x.shape[-1])
                a.input_dtype = TORCH_TO_DTYPE[x.dtype].value
                _FAST.set_tuning(f[0], M, lookup_tuning(-1, M, a))
                y = _FAST.forward(f[0], f[1], f[2], f[3], x, f[4], -1, _CACHE_EPOCH[0], FUSE_BIAS)
            if y is False:  # the handle is stale (tensors moved, tuning table changed): rebuilt behind the slow call below
                d["_fast"] = None
                d["_fast_tried"] = None
            elif y is not None and y is not NotImplemented:
                return y
        y = self._call(x, -1)
        # (after a SUCCESSFUL slow call: errors and the once-per-shape coverage-kernel warning come from that path)
        if _FAST is not None and d.get("_fast") is None and d.get("_fast_tried") != _CACHE_EPOCH[0] and TUNING_OVERRIDE is None \
                and x.is_cuda and not torch.compiler.is_compiling():
            self._install_fast()
        return y

    # ----------------------------------------------------------------------- tuning-hint JSON cache
    @staticmethod
    def cache_config(filename: str):
        """Merge the in-memory hint table into `filename` (JSON: family -> "(M,N,K,g,e,type_id)" -> dict)."""
        try:
            with _FILE_LOCK, open(filename, "r") as f:
                config = json.load(f)
        except Exception:
            config = {}
        for name in GEMLITE_MATMUL_TYPES:
            config.setdefault(name, {}).update(GEMLITE_HIP_CONFIG_CACHE.get(name, {}))
        with _FILE_LOCK, open(filename, "w") as f:
            json.dump(config, f)

    @staticmethod
    def load_config(filename: str, print_error: bool = True, overwrite: bool = False):
        if filename is None:
            return False
        try:
            with _FILE_LOCK, open(filename, "r") as f:
                config = json.load(f)
            if overwrite:
                GEMLITE_HIP_CONFIG_CACHE.clear()
            for name, entries in config.items():
                GEMLITE_HIP_CONFIG_CACHE.setdefault(name, {}).update(entries)
        except Exception as e:  # same contract as the reference: log and report failure
            if print_error:
                logger.error(f"Failed to load the cache file '{filename}': {e}")
            return False
        return True

    @staticmethod
    def reset_config():
        GEMLITE_HIP_CONFIG_CACHE.clear()


GemLiteLinear = GemLiteLinearHIP
GemLiteLinearTriton = GemLiteLinearHIP  # the reference's class name; there is no Triton here


# ------------------------------------------------------------------------------------------------------
# shipped per-GPU tuning table, picked by device name like the reference's configs/*.json (core.py:634-654)
# ------------------------------------------------------------------------------------------------------
_ARCH_TAGS = {"gfx950": "mi355x"}  # boxes report "AMD Radeon Graphics" / "AMD Instinct MI355X": the ISA name is reliable
_AUTOLOAD_DONE = False


def get_default_cache_config(device_index: int = 0) -> Optional[str]:
    """Path of the shipped table whose tag occurs in the device name (longest tag first), or in its ISA name."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "configs")
    if not os.path.isdir(root) or not torch.cuda.is_available():
        return None
    props = torch.cuda.get_device_properties(device_index)
    name = props.name.lower().replace(" ", "_")
    arch = getattr(props, "gcnArchName", "").split(":")[0].lower()
    tags = sorted((f[:-5] for f in os.listdir(root) if f.endswith(".json")), key=len, reverse=True)
    for tag in tags:
        if tag in name or _ARCH_TAGS.get(arch) == tag:
            return os.path.join(root, tag + ".json")
    return None


def autoload_default_config(device_index: int = 0) -> Optional[str]:
    """Load the shipped table once (first GPU launch, or explicitly).  Entries already in the cache win."""
    global _AUTOLOAD_DONE
    if _AUTOLOAD_DONE:
        return None
    _AUTOLOAD_DONE = True
    if os.environ.get("GEMLITE_HIP_NO_DEFAULT_CONFIG"):
        return None
    path = get_default_cache_config(device_index)
    if path is None:
        return None
    try:
        with _FILE_LOCK, open(path, "r") as f:
            config = json.load(f)
        for fam, entries in config.items():
            if isinstance(entries, dict):
                tgt = GEMLITE_HIP_CONFIG_CACHE.setdefault(fam, {})
                for k, v in entries.items():
                    tgt.setdefault(k, v)
        logger.warning("Loaded " + path + " config.")
        return path
    except Exception as e:  # a broken table must never break the forward path
        logger.error(f"Failed to load the default config '{path}': {e}")
        return None
