"""Dynamic per-token activation quantisation (reference: gemlite/quant_utils.py:231-347).

``scale_activations_per_token(x, w_dtype)`` returns ``(x_q, scales)`` with ``x_q`` of dtype ``w_dtype``
(int8 / fp8) and ``scales`` fp32 ``[M, 1]``:  s = max(amax|x_row| / qmax, 1e-6), x_q = clamp(x / s),
int8 rounded with floor(v + 0.5) — the rounding the reference's kernel uses on AMD (quant_utils.py:259-266).
Runs as one HIP kernel (`gemlite_hip_scale_activations_per_token`).

``WeightQuantizerINT``: float weights -> grouped asymmetric INT codes + (scale, zero) per group, one HIP kernel
(`gemlite_hip_quantize_groups`; the reference leaves this step to the third-party ``hqq`` package); ``WeightQuantizerHQQ``: the same
with HQQ's zero-point optimiser inside the launch (`gemlite_hip_quantize_groups_hqq`); and back (``dequantize``:
`gemlite_hip_dequantize`, DESIGN §2.3, which ``WeightQuantizerMXFP.dequantize`` takes too for GPU tensors).

``WeightQuantizerRows``: float weights -> channel-wise symmetric INT8 / FP8 codes + one scale per output channel, the tensors of the
``A16W8*`` / ``A8W8*_dynamic`` processors (GPU weights: one HIP kernel, `gemlite_hip_quantize_rows`; CPU tensors: the
reference's torch sequence, ``_quantize_rows_torch``).

Block-scaled formats (reference: gemlite/quant_utils.py:21-225 weight quantiser, :502-954 activation quantisers):
``WeightQuantizerMXFP`` (GPU float weights: one HIP kernel, `gemlite_hip_quantize_mx`; CPU tensors, the scale-search
window and ``index=False``: the reference's torch code) and
``scale_activations_mxfp8 / _mxfp4 / _nvfp4`` (one HIP kernel each, `gemlite_hip_scale_activations_*`).
"""
from __future__ import annotations

from typing import Tuple

import torch

from . import _hip
from .dtypes import TORCH_TO_DTYPE, DType


def get_dtype_range(dtype: torch.dtype) -> Tuple[float, float]:
    if dtype.is_floating_point:
        info = torch.finfo(dtype)
    else:
        info = torch.iinfo(dtype)
    return float(info.min), float(info.max)


def scale_activations_per_token(tensor: torch.Tensor, w_dtype: torch.dtype, fp32_scale: bool = True):
    _hip.require_gpu_tensor(tensor, "tensor")
    if w_dtype not in (torch.int8, torch.float8_e4m3fn, torch.float8_e5m2):
        raise NotImplementedError(f"activation quantisation to {w_dtype} is not supported on gfx950 "
                                  "(use torch.float8_e4m3fn, not the MI300X fnuz flavour)")
    shape = tensor.shape
    x2 = tensor.reshape(-1, shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    M, K = x2.shape
    y = torch.empty((M, K), dtype=w_dtype, device=tensor.device)
    scales = torch.empty((M, 1), dtype=torch.float32, device=tensor.device)
    with _hip.on_device(tensor.device):
        rc = _hip.load().gemlite_hip_scale_activations_per_token(
            x2.data_ptr(), y.data_ptr(), scales.data_ptr(), M, K, x2.stride(0), TORCH_TO_DTYPE[x2.dtype].value,
            TORCH_TO_DTYPE[w_dtype].value, _hip.current_stream_handle(tensor.device))
    _hip.raise_for_status(rc, "scale_activations_per_token")
    if not fp32_scale:
        scales = scales.to(tensor.dtype)
    return y.view(shape), scales


scale_activations_per_token_triton = scale_activations_per_token  # reference export name


# ------------------------------------------------------------------------------------------------------
# grouped asymmetric INT weights: round to nearest on the group's min / max (one HIP launch)
# ------------------------------------------------------------------------------------------------------
def check_group_size(in_features: int, group_size: int, what: str = "weight"):
    if group_size <= 0 or group_size % 32 != 0 or in_features % group_size != 0:
        raise ValueError(f"{what}: group_size {group_size} must be a multiple of 32 that divides in_features = {in_features}")


def _quantize_groups(W: torch.Tensor, W_nbits: int, group_size: int, meta_dtype: torch.dtype, packed: bool, fold_zeros: bool = False,
                     hqq=None):
    """One `gemlite_hip_quantize_groups` launch on W's device and current stream.  packed: (int32 words [K/e, N], scales [K/g, N],
    zeros [K/g, N], folded if asked) — what a packed layer holds; else (uint8 codes [N, K], scales [N * K/g, 1], zeros [N * K/g, 1]).
    hqq = (iters, lp_norm, beta, kappa): the same launch with the zero-point optimiser, `gemlite_hip_quantize_groups_hqq`."""
    _hip.require_gpu_tensor(W, "W")
    assert W.dim() == 2, "W should be [out_features, in_features]"
    if W.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        W = W.float()
    if W.stride(1) != 1:
        W = W.contiguous()
    N, K = W.shape
    check_group_size(K, group_size)
    n_groups = K // group_size
    dev = W.device
    if hqq is None:
        a = _hip.QuantizeArgs()
    else:
        h = _hip.QuantizeHqqArgs()
        h.struct_size = _hip.C.sizeof(_hip.QuantizeHqqArgs)
        h.iters, h.lp_norm, h.beta, h.kappa = hqq
        a = h.q
    if packed:
        q = torch.empty((K // (32 // W_nbits), N), dtype=torch.int32, device=dev)
        scales = torch.empty((n_groups, N), dtype=meta_dtype, device=dev)
        a.pack_bits, a.ld_q, a.stride_meta_g, a.stride_meta_n = 32, 0, N, 1
    else:
        q = torch.empty((N, K), dtype=torch.uint8, device=dev)
        scales = torch.empty((N * n_groups, 1), dtype=meta_dtype, device=dev)
        a.pack_bits, a.ld_q, a.stride_meta_g, a.stride_meta_n = 0, K, 1, n_groups
    zeros = torch.empty_like(scales)
    a.struct_size = _hip.C.sizeof(_hip.QuantizeArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, N, K, W.stride(0)
    a.W_nbits, a.group_size, a.meta_dtype = W_nbits, group_size, TORCH_TO_DTYPE[meta_dtype].value
    a.q_out, a.scales, a.zeros, a.fold_zeros = q.data_ptr(), scales.data_ptr(), zeros.data_ptr(), int(fold_zeros)
    with _hip.on_device(dev):
        if hqq is None:
            rc = _hip.load().gemlite_hip_quantize_groups(_hip.C.byref(a), _hip.current_stream_handle(dev))
        else:
            rc = _hip.load().gemlite_hip_quantize_groups_hqq(_hip.C.byref(h), _hip.current_stream_handle(dev))
    _hip.raise_for_status(rc, "quantize_groups" if hqq is None else "quantize_groups_hqq")
    return q, scales, zeros


class WeightQuantizerINT:
    """Float weights -> (W_q uint8 [N, K], scales [N * K/g, 1], zeros [N * K/g, 1]): the tensors ``from_weights`` of the ``*_HQQ_INT``
    processors and HQQ's ``meta`` hold.  Asymmetric round to nearest on each group's min / max (HQQ's starting point, without its
    optimiser: ``WeightQuantizerHQQ`` below adds it); the codes are taken against the ROUNDED (scale, zero), which is what the layer
    dequantises with.  ``dtype`` is the metadata type: None = W.dtype if that is fp16 / bf16, else fp16.  GPU tensors only."""

    def __init__(self, W_nbits: int, group_size: int, dtype=None, device="cuda:0"):
        assert W_nbits in (8, 4, 2, 1), "W_nbits should be 8, 4, 2 or 1"
        self.W_nbits, self.group_size, self.dtype, self.device = W_nbits, group_size, dtype, device

    def meta_dtype(self, W: torch.Tensor) -> torch.dtype:
        if self.dtype is not None:
            return self.dtype
        return W.dtype if W.dtype in (torch.float16, torch.bfloat16) else torch.float16

    def quantize(self, W: torch.Tensor):
        return _quantize_groups(W, self.W_nbits, self.group_size, self.meta_dtype(W), packed=False)

    def quantize_packed(self, W: torch.Tensor, fold_zeros: bool):
        """The layer's own tensors in one launch: 32-bit words [K/e, N], scales and (folded) zeros [K/g, N]."""
        return _quantize_groups(W, self.W_nbits, self.group_size, self.meta_dtype(W), packed=True, fold_zeros=fold_zeros)

    def dequantize(self, W_q: torch.Tensor, scales: torch.Tensor, zeros: torch.Tensor, shape=None, dtype=None, fold_zeros: bool = False):
        """The float weights [N, K] the tensors of ``quantize()`` (uint8 codes [N, K], metadata [N * K/g, 1]: (q - z) * s) or of
        ``quantize_packed()`` (int32 words [K/e, N], metadata [K/g, N]; ``fold_zeros`` as it was given there: fma(q, s, z')) stand for,
        in one `gemlite_hip_dequantize` launch.  ``dtype``: float16 / bfloat16 / float32, default the metadata's type;
        ``shape``: (N, K) of flat uint8 codes, and the shape of the result."""
        _hip.require_gpu_tensor(W_q, "W_q")
        dev = W_q.device
        dtype = scales.dtype if dtype is None else dtype
        a = _hip.DequantizeArgs()
        if W_q.dtype == torch.int32:
            assert W_q.dim() == 2, "packed W_q should be [K / elements_per_sample, N]"
            e = 32 // self.W_nbits
            N, K = W_q.shape[1], W_q.shape[0] * e
            g = K // (scales.numel() // N)
            scales, zeros = scales.view(K // g, N), zeros.view(K // g, N)
            a.elements_per_sample, a.w_pack_bits, a.w_dtype = e, 32, TORCH_TO_DTYPE[torch.int32].value
            a.stride_wk, a.stride_wn = W_q.stride(0), W_q.stride(1)
            a.stride_meta_g, a.stride_meta_n = scales.stride(0), scales.stride(1)
            a.W_group_mode = 4 if fold_zeros else 3
        else:
            assert W_q.dtype == torch.uint8, "W_q should be uint8 codes [N, K] or int32 words [K / elements_per_sample, N]"
            W_q = W_q.view(tuple(shape)) if (shape is not None and W_q.dim() != 2) else W_q
            assert W_q.dim() == 2, "flat codes need shape=(N, K)"
            N, K = W_q.shape
            g = (N * K) // scales.numel()
            scales, zeros = scales.reshape(N, K // g), zeros.reshape(N, K // g)
            a.elements_per_sample, a.w_pack_bits, a.w_dtype = 1, 0, TORCH_TO_DTYPE[torch.uint8].value
            a.stride_wk, a.stride_wn = W_q.stride(1), W_q.stride(0)
            a.stride_meta_g, a.stride_meta_n = scales.stride(1), scales.stride(0)
            a.W_group_mode = 3
        assert zeros.stride() == scales.stride(), "scales and zeros should share one layout"
        out = torch.empty((N, K), dtype=dtype, device=dev)
        a.struct_size = _hip.C.sizeof(_hip.DequantizeArgs)
        a.w_q, a.scales, a.zeros, a.out = W_q.data_ptr(), scales.data_ptr(), zeros.data_ptr(), out.data_ptr()
        a.N, a.K, a.ld_out, a.W_nbits, a.group_size = N, K, K, self.W_nbits, g
        a.out_dtype, a.input_dtype = TORCH_TO_DTYPE[dtype].value, TORCH_TO_DTYPE[dtype].value
        a.meta_dtype, a.zeros_dtype = TORCH_TO_DTYPE[scales.dtype].value, TORCH_TO_DTYPE[zeros.dtype].value
        a.post_scale = 1.0
        with _hip.on_device(dev):
            rc = _hip.load().gemlite_hip_dequantize(_hip.C.byref(a), _hip.current_stream_handle(dev))
        _hip.raise_for_status(rc, "gemlite_hip_dequantize")
        return out if shape is None else out.view(tuple(shape))


class WeightQuantizerHQQ(WeightQuantizerINT):
    """``WeightQuantizerINT`` with HQQ's proximal optimiser on every group's zero, inside the same single launch
    (`gemlite_hip_quantize_groups_hqq`): same tensors, shapes and layouts returned; the scale is round to nearest's, the
    zero is the best of up to ``iters`` candidates, judged per group by the error of what the layer computes — no group ends worse
    than ``WeightQuantizerINT``'s, and ``iters=0`` is ``WeightQuantizerINT``.  The defaults are HQQ's.  GPU tensors only."""

    def __init__(self, W_nbits: int, group_size: int, dtype=None, device="cuda:0", iters: int = 20, lp_norm: float = 0.7,
                 beta: float = 10.0, kappa: float = 1.01):
        super().__init__(W_nbits, group_size, dtype=dtype, device=device)
        self.iters, self.lp_norm, self.beta, self.kappa = int(iters), float(lp_norm), float(beta), float(kappa)
        if not (0 <= self.iters <= 100 and 0.0 < self.lp_norm <= 1.0 and 0.0 < self.beta < float("inf") and 0.0 < self.kappa < float("inf")):
            raise ValueError(f"WeightQuantizerHQQ: need 0 <= iters <= 100, 0 < lp_norm <= 1, beta > 0, kappa > 0; got iters={iters}, "
                             f"lp_norm={lp_norm}, beta={beta}, kappa={kappa}")

    def _hqq(self):
        return (self.iters, self.lp_norm, self.beta, self.kappa)

    def quantize(self, W: torch.Tensor):
        return _quantize_groups(W, self.W_nbits, self.group_size, self.meta_dtype(W), packed=False, hqq=self._hqq())

    def quantize_packed(self, W: torch.Tensor, fold_zeros: bool):
        return _quantize_groups(W, self.W_nbits, self.group_size, self.meta_dtype(W), packed=True, fold_zeros=fold_zeros, hqq=self._hqq())


# ------------------------------------------------------------------------------------------------------
# channel-wise symmetric 8-bit weights: one scale per output channel (one HIP launch)
# ------------------------------------------------------------------------------------------------------
ROWS_FORMATS = {torch.int8: 0, torch.float8_e4m3fn: 1, torch.float8_e5m2: 2}  # code dtype -> format of gemlite_hip_quantize_rows
_ROWS_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
# The scale rule the processors pass: 0 divides amax by the format's maximum, 1 multiplies by the fp32 reciprocal of it.  Rule 1 is
# what torch's `tensor / python_scalar` computes on a GPU tensor, so the layers equal what the torch sequence built there.
ROWS_SCALE_RULE = 1


def _quantize_rows_torch(weight: torch.Tensor, w_dtype: torch.dtype, device=None):
    """The reference's sequence (helper.py:110-118, :437-444), torch ops on `device`: (W_q [N, K] of w_dtype, scales fp32 [N, 1])."""
    info = torch.finfo(w_dtype) if w_dtype.is_floating_point else torch.iinfo(w_dtype)
    W = weight.to(device=device, dtype=torch.float32)
    scales = (W.abs().amax(dim=1, keepdim=True) / info.max).clamp_(min=1e-6)
    W_q = (W / scales).clamp_(info.min, info.max)
    W_q = W_q.to(w_dtype) if w_dtype.is_floating_point else W_q.round_().to(w_dtype)
    return W_q, scales


def _takes_rows_kernel(weight: torch.Tensor, w_dtype: torch.dtype, device) -> bool:
    """The inputs `gemlite_hip_quantize_rows` takes for a layer on `device`; everything else stays on the torch sequence above."""
    return (torch.device(device).type == "cuda" and w_dtype in ROWS_FORMATS and weight.dim() == 2 and weight.dtype in _ROWS_KERNEL_DTYPES
            and weight.shape[0] > 0 and weight.shape[1] > 0 and weight.stride(1) == 1)


def _quantize_rows(W: torch.Tensor, w_dtype: torch.dtype, scale_dtype: torch.dtype, scale_rule: int):
    """One `gemlite_hip_quantize_rows` launch on W's device and current stream (contract: DESIGN §2.4, include/gemlite_hip.h):
    (codes [N, K] of w_dtype, scales [N, 1] of scale_dtype).  W is read in its own dtype through its row stride."""
    _hip.require_gpu_tensor(W, "W")
    assert W.dim() == 2 and W.stride(1) == 1, "W should be [out_features, in_features] with unit inner stride"
    N, K = W.shape
    dev = W.device
    q = torch.empty((N, K), dtype=w_dtype, device=dev)
    scales = torch.empty((N, 1), dtype=scale_dtype, device=dev)
    a = _hip.QuantizeRowsArgs()
    a.struct_size = _hip.C.sizeof(_hip.QuantizeRowsArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, N, K, (W.stride(0) if N > 1 else max(K, W.stride(0)))
    a.format, a.scale_rule, a.q_out, a.ld_q = ROWS_FORMATS[w_dtype], int(scale_rule), q.data_ptr(), K
    a.scales, a.stride_s, a.scale_dtype, a.reserved = scales.data_ptr(), 1, TORCH_TO_DTYPE[scale_dtype].value, 0
    with _hip.on_device(dev):
        rc = _hip.load().gemlite_hip_quantize_rows(_hip.C.byref(a), _hip.current_stream_handle(dev))
    _hip.raise_for_status(rc, "quantize_rows")
    return q, scales


class WeightQuantizerRows:
    """Float weights -> (W_q [N, K] int8 / float8_e4m3fn / float8_e5m2, scales [N, 1]): symmetric, one scale per output channel,
    ``s = max(amax / qmax, 1e-6)``, ``W_q = clamp(W / s)`` rounded to nearest even — what ``from_weights(W_q, bias, scales)`` of the
    ``A16W8*`` / ``A8W8*_dynamic`` processors takes.  A 2-D fp32 / fp16 / bf16 GPU weight with unit inner stride is quantised by ONE HIP
    launch in its own dtype (`gemlite_hip_quantize_rows`); CPU tensors (and ``*fnuz`` fp8, other layouts) run the reference's
    torch sequence.  ``fp32_scale=False`` returns the scales rounded once to ``dtype`` (None = W.dtype if that is fp16 / bf16, else fp16).
    ``scale_rule``: 0 = amax / qmax (torch on a CPU tensor), 1 = amax * (1 / qmax) (torch on a GPU tensor), None = ``ROWS_SCALE_RULE``."""

    def __init__(self, w_dtype: torch.dtype, dtype=None, device="cuda:0", fp32_scale: bool = True, scale_rule=None):
        assert w_dtype.itemsize == 1, f"w_dtype should be an 8-bit type (INT8 or FP8), got {w_dtype}"
        assert scale_rule in (None, 0, 1), "scale_rule should be 0, 1 or None"
        self.w_dtype, self.dtype, self.device, self.fp32_scale = w_dtype, dtype, device, fp32_scale
        self.scale_rule = ROWS_SCALE_RULE if scale_rule is None else scale_rule

    def scale_dtype(self, W: torch.Tensor) -> torch.dtype:
        if self.fp32_scale:
            return torch.float32
        if self.dtype is not None:
            return self.dtype
        return W.dtype if W.dtype in (torch.float16, torch.bfloat16) else torch.float16

    def quantize(self, W: torch.Tensor):
        if W.is_cuda and _takes_rows_kernel(W, self.w_dtype, W.device):
            return _quantize_rows(W, self.w_dtype, self.scale_dtype(W), self.scale_rule)
        W_q, scales = _quantize_rows_torch(W, self.w_dtype)
        return W_q, scales.to(self.scale_dtype(W))

    def dequantize(self, W_q: torch.Tensor, scales: torch.Tensor, dtype=None):
        """The float weights [N, K] the tensors of ``quantize()`` stand for, ``code * s`` (one fp32 multiplication, then one rounding to
        ``dtype``: float16 / bfloat16 / float32, default ``self.dtype`` or float16), in one `gemlite_hip_dequantize` launch."""
        _hip.require_gpu_tensor(W_q, "W_q")
        assert W_q.dim() == 2 and W_q.element_size() == 1 and scales.numel() == W_q.shape[0], "W_q [N, K] 8-bit codes, one scale per row"
        if dtype is None:
            dtype = self.dtype if self.dtype is not None else torch.float16
        N, K = W_q.shape
        dev = W_q.device
        scales = scales.reshape(N, 1)
        out = torch.empty((N, K), dtype=dtype, device=dev)
        a = _hip.DequantizeArgs()
        a.struct_size = _hip.C.sizeof(_hip.DequantizeArgs)
        a.w_q, a.scales, a.out = W_q.data_ptr(), scales.data_ptr(), out.data_ptr()
        a.N, a.K, a.ld_out, a.W_nbits, a.group_size = N, K, K, 8, K
        a.stride_wk, a.stride_wn, a.stride_meta_g, a.stride_meta_n = W_q.stride(1), W_q.stride(0), 0, scales.stride(0)
        a.elements_per_sample, a.w_pack_bits, a.w_dtype = 1, 0, TORCH_TO_DTYPE[W_q.dtype].value
        a.out_dtype, a.input_dtype, a.meta_dtype = TORCH_TO_DTYPE[dtype].value, TORCH_TO_DTYPE[dtype].value, TORCH_TO_DTYPE[scales.dtype].value
        a.W_group_mode, a.channel_scale_mode, a.post_scale = 0, 1, 1.0
        with _hip.on_device(dev):
            rc = _hip.load().gemlite_hip_dequantize(_hip.C.byref(a), _hip.current_stream_handle(dev))
        _hip.raise_for_status(rc, "gemlite_hip_dequantize")
        return out


# ------------------------------------------------------------------------------------------------------
# block-scaled formats
# ------------------------------------------------------------------------------------------------------
NVFP4_META_SCALE = 0.05  # the reference's fixed second-level scale of NVFP4 (quant_utils.py:21)
MX_EPS_EXP = -30         # smallest block scale: 2^-30
FP4_POS_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)          # e2m1 magnitudes, code = index (+8: negative)
FP4_THRESHOLDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)          # midpoints: a magnitude ON a midpoint rounds down


MX_FORMATS = {"mxfp8": (0, 32), "mxfp4": (1, 32), "nvfp4": (2, 16)}  # name -> (format code of gemlite_hip_quantize_mx, block size)
_MX_KERNEL_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _takes_mx_kernel(W: torch.Tensor, index: bool, window_size: int = 0) -> bool:
    """The inputs `gemlite_hip_quantize_mx` takes; everything else stays on the torch code below."""
    return (W.is_cuda and index and window_size == 0 and W.dim() == 2 and W.dtype in _MX_KERNEL_DTYPES
            and W.shape[0] > 0 and W.shape[1] > 0 and W.shape[1] % 32 == 0)


def _quantize_mx(W: torch.Tensor, fmt: str, layer_layout: bool):
    """One `gemlite_hip_quantize_mx` launch on W's device and current stream (contract: DESIGN §2.2, include/gemlite_hip.h).
    layer_layout: (elements [N, K] fp8 or [N, K/2] uint8 with two codes per byte, scale bytes [K/g, N]) — what a packed layer holds;
    else (elements [N, K] fp8 / uint8 codes, scale bytes [N * K/g, 1])."""
    _hip.require_gpu_tensor(W, "W")
    assert W.dim() == 2, "W should be [out_features, in_features]"
    code, g = MX_FORMATS[fmt]
    if W.dtype not in _MX_KERNEL_DTYPES:
        W = W.float()
    if W.stride(1) != 1:
        W = W.contiguous()
    N, K = W.shape
    if K % 32 != 0:
        raise ValueError(f"block-scaled weight quantisation needs in_features % 32 == 0, got {K}")
    dev = W.device
    pack = int(layer_layout and code != 0)
    q = torch.empty((N, K // 2 if pack else K), dtype=torch.float8_e4m3fn if code == 0 else torch.uint8, device=dev)
    a = _hip.QuantizeMxArgs()
    if layer_layout:
        scales = torch.empty((K // g, N), dtype=torch.uint8, device=dev)
        a.stride_scale_g, a.stride_scale_n = N, 1
    else:
        scales = torch.empty((N * (K // g), 1), dtype=torch.uint8, device=dev)
        a.stride_scale_g, a.stride_scale_n = 1, K // g
    a.struct_size = _hip.C.sizeof(_hip.QuantizeMxArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, N, K, W.stride(0)
    a.format, a.pack_nibbles, a.q_out, a.ld_q, a.scales, a.reserved = code, pack, q.data_ptr(), q.stride(0), scales.data_ptr(), 0
    with _hip.on_device(dev):
        rc = _hip.load().gemlite_hip_quantize_mx(_hip.C.byref(a), _hip.current_stream_handle(dev))
    _hip.raise_for_status(rc, "quantize_mx")
    return q, scales


def _fp4_tables(device, dtype=torch.float32):
    pos = torch.tensor(FP4_POS_VALUES, dtype=dtype, device=device)
    return pos, torch.tensor(FP4_THRESHOLDS, dtype=dtype, device=device), torch.cat([pos, -pos])


class WeightQuantizerMXFP:
    """Weights -> (elements, block scales) in the OCP microscaling formats, arithmetic of the reference quantiser
    (quant_utils.py:70-225): MXFP8 / MXFP4 = e4m3 / e2m1 elements with one power-of-two (e8m0) scale per 32 weights,
    ``scale = 2^ceil(log2(amax / qmax))`` floored at 2^-30; NVFP4 = e2m1 elements with an e4m3 scale per 16 weights on
    top of the fixed meta scale 0.05.  ``index=True`` returns what ``GemLiteLinear.pack`` takes (fp8 tensor / uint8
    codes), otherwise the rounded values as floats.  ``window_size`` > 0 searches neighbouring scales for the smallest
    mean absolute error, like the reference.
    A 2-D fp32 / fp16 / bf16 weight on a GPU with ``index=True``, no window and ``in_features % 32 == 0`` is quantised by ONE HIP
    launch (`gemlite_hip_quantize_mx`; same shapes and dtypes returned, finite blocks equal to this torch code on the CPU, a block that
    holds a NaN / Inf gets the scale format's NaN code); every other call runs the torch code below unchanged."""

    def __init__(self, compute_dtype=torch.bfloat16, device="cuda:0"):
        self.compute_dtype = compute_dtype
        self.device = device

    @staticmethod
    def round_to_closest_fp4(tensor: torch.Tensor) -> torch.Tensor:
        pos, thr, _ = _fp4_tables(tensor.device)
        out = pos[torch.searchsorted(thr.to(tensor.dtype), tensor.abs())].to(tensor.dtype)
        return out * tensor.sign()

    @staticmethod
    def to_index(W_q: torch.Tensor) -> torch.Tensor:
        assert W_q.is_floating_point(), "Input should be floating point fp4 values."
        _, _, values = _fp4_tables(W_q.device, W_q.dtype)
        hit = W_q.reshape(-1, 1) == values.view(1, -1)  # -0.0 == 0.0: both zeros map to code 0 (first match)
        return hit.to(torch.uint8).argmax(dim=1).to(torch.uint8).view(W_q.shape)

    def quantize_packed(self, W: torch.Tensor, fmt: str):
        """The layer's own tensors in one launch, fmt = "mxfp8" | "mxfp4" | "nvfp4": elements [N, K] float8_e4m3fn or [N, K/2] uint8
        (two e2m1 codes per byte, even k in the low nibble) and the block scales [K/g, N] (uint8 e8m0 bytes; NVFP4: float8_e4m3fn)."""
        q, scales = _quantize_mx(W, fmt, layer_layout=True)
        return q, (scales.view(torch.float8_e4m3fn) if fmt == "nvfp4" else scales)

    def quantize_mxfp8(self, W, index: bool = False, mx_fp8_dtype: torch.dtype = torch.float8_e4m3fn):
        if mx_fp8_dtype == torch.float8_e4m3fn and _takes_mx_kernel(W, index):
            q, scales = _quantize_mx(W, "mxfp8", layer_layout=False)
            return q.view(-1, 32), scales.view(torch.float8_e8m0fnu)
        eps = 2.0 ** MX_EPS_EXP
        lo, hi = get_dtype_range(mx_fp8_dtype)
        flat = W.reshape(-1, 32).float()
        ideal = flat.abs().amax(dim=1, keepdim=True) / hi
        scales = (2 ** torch.ceil(torch.log2(ideal))).clamp_(min=eps)
        W_q = (flat / scales).clamp_(min=lo, max=hi).to(mx_fp8_dtype)
        if not index:
            W_q = W_q.to(flat.dtype)
        return W_q, scales.to(torch.float8_e8m0fnu)

    def _search(self, flat, candidates, full_scale_of):
        """candidate with the smallest mean |W - round(W / s) * s| per block"""
        q = self.round_to_closest_fp4(flat.unsqueeze(1) / full_scale_of(candidates).unsqueeze(-1))
        err = (flat.unsqueeze(1) - q * candidates.unsqueeze(-1)).abs().mean(dim=-1)
        return torch.gather(candidates, 1, torch.argmin(err, dim=1, keepdim=True))

    def quantize_mxfp4(self, W, window_size: int = 0, index: bool = False):
        if _takes_mx_kernel(W, index, window_size):
            q, scales = _quantize_mx(W, "mxfp4", layer_layout=False)
            return q.view(-1, 32), scales.view(torch.float8_e8m0fnu)
        eps = 2.0 ** MX_EPS_EXP
        flat = W.reshape(-1, 32).float()
        ideal = flat.abs().amax(dim=1, keepdim=True) / 6
        log2s = torch.ceil(torch.log2(ideal))
        if window_size == 0:
            scales = 2 ** log2s
        else:
            offs = torch.arange(-window_size, window_size + 1, device=W.device, dtype=log2s.dtype).view(1, -1)
            cand = torch.pow(2, log2s + offs)
            cand[cand < eps] = eps
            scales = self._search(flat, cand, lambda c: c)
        scales = scales.clamp_(eps)
        W_q = self.round_to_closest_fp4(flat / scales)
        if index:
            W_q = self.to_index(W_q)
        return W_q, scales.to(torch.float8_e8m0fnu)

    def quantize_nvfp4(self, W, window_size: int = 0, index: bool = False):
        if _takes_mx_kernel(W, index, window_size):
            q, scales = _quantize_mx(W, "nvfp4", layer_layout=False)
            return q.view(-1, 16), scales.view(torch.float8_e4m3fn)
        eps, fp8 = 1e-6, torch.float8_e4m3fn
        flat = W.reshape(-1, 16).float()
        ideal = flat.abs().amax(dim=1, keepdim=True) / 6
        ideal = (ideal / NVFP4_META_SCALE).clamp_(max=torch.finfo(fp8).max).to(fp8)
        if window_size == 0:
            scales = ideal
        else:
            offs = torch.arange(-window_size, window_size + 1, device=W.device, dtype=torch.int).view(1, -1)
            cand = (ideal.view(torch.int8) + offs).clamp_(-128, 127).to(torch.int8)
            cand[cand == -1] = 1   # the two NaN encodings of e4m3
            cand[cand == 127] = 1
            cand = cand.view(fp8).float()
            cand[cand < eps] = eps
            q = self.round_to_closest_fp4(flat.unsqueeze(1) / (cand * NVFP4_META_SCALE).unsqueeze(-1))
            err = (flat.unsqueeze(1) - q * cand.unsqueeze(-1)).abs().mean(dim=-1)
            scales = torch.gather(cand, 1, torch.argmin(err, dim=1, keepdim=True)).to(fp8)
        full = (scales.to(flat.dtype) * NVFP4_META_SCALE).clamp_(min=eps)
        W_q = self.round_to_closest_fp4(flat / full)
        if index:
            W_q = self.to_index(W_q)
        return W_q, scales

    def _dequantize_kernel(self, W_q, scales, shape, dtype):
        """One `gemlite_hip_dequantize` launch for what the kernel takes — GPU e4m3 elements or uint8 e2m1 codes with e8m0 scales per 32
        or e4m3 scales per 16, to fp16 / bf16 / fp32 — bit-identical to the torch code below; None for everything else.  Elements and
        scales are walked flat, as rows of a power-of-two length that divides them."""
        import math
        if not (W_q.is_cuda and scales.is_cuda and W_q.device == scales.device and dtype in _MX_KERNEL_DTYPES
                and W_q.is_contiguous() and scales.is_contiguous() and scales.numel() > 0):
            return None
        fp8 = W_q.dtype == torch.float8_e4m3fn
        if not (fp8 or W_q.dtype == torch.uint8) or W_q.numel() % scales.numel() != 0:
            return None
        group = W_q.numel() // scales.numel()
        if scales.dtype == torch.float8_e8m0fnu and group == 32:
            in_dt = DType.MXFP8.value if fp8 else DType.MXFP4.value
        elif scales.dtype == torch.float8_e4m3fn and group == 16 and not fp8:
            in_dt = DType.NVFP4.value
        else:
            return None
        K = math.gcd(W_q.numel(), 8192)
        if K % 32 != 0:
            return None
        N = W_q.numel() // K
        out = torch.empty((N, K), dtype=dtype, device=W_q.device)
        a = _hip.DequantizeArgs()
        a.struct_size = _hip.C.sizeof(_hip.DequantizeArgs)
        a.w_q, a.scales, a.out = W_q.data_ptr(), scales.data_ptr(), out.data_ptr()
        a.N, a.K, a.ld_out, a.stride_wk, a.stride_wn, a.stride_meta_g, a.stride_meta_n = N, K, K, 1, K, 1, K // group
        a.W_nbits, a.group_size, a.elements_per_sample, a.w_pack_bits = (8 if fp8 else 4), group, 1, 0
        a.w_dtype, a.input_dtype, a.out_dtype = TORCH_TO_DTYPE[W_q.dtype].value, in_dt, TORCH_TO_DTYPE[dtype].value
        a.meta_dtype, a.post_scale = TORCH_TO_DTYPE[torch.uint8].value, 1.0
        with _hip.on_device(W_q.device):
            rc = _hip.load().gemlite_hip_dequantize(_hip.C.byref(a), _hip.current_stream_handle(W_q.device))
        _hip.raise_for_status(rc, "gemlite_hip_dequantize")
        return out.view(-1, group) if shape is None else out.view(shape)

    def dequantize(self, W_q, scales, shape=None, dtype=None):
        out = self._dequantize_kernel(W_q, scales, shape, self.compute_dtype if dtype is None else dtype)
        if out is not None:
            return out
        if W_q.dtype == torch.uint8:  # e2m1 codes
            _, _, values = _fp4_tables(W_q.device)
            W_q = values[W_q.int()]
        group = W_q.numel() // scales.numel()
        out = W_q.reshape(-1, group).float() * scales.float().reshape(-1, 1)
        if shape is not None:
            out = out.view(shape)
        return out.to(self.compute_dtype if dtype is None else dtype)


def _scale_activations_mx(tensor: torch.Tensor, mode: str):
    """(x_q, block scales) of the activations.  x_q: fp8 [.., K] (mxfp8) or uint8 [.., K/2] e2m1 codes, k even in the low
    nibble (mxfp4 / nvfp4); scales: uint8 e8m0 [M_pad, K/32] (nvfp4: float8_e4m3fn [M_pad, K/16]) with M_pad = M rounded up
    to the block size — shapes and padding of scale_activations_*_triton_v2 (quant_utils.py:546-590, 820-855, 917-954)."""
    _hip.require_gpu_tensor(tensor, "tensor")
    group = 16 if mode == "nvfp4" else 32
    x2 = tensor.reshape(-1, tensor.shape[-1])
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    M, K = x2.shape
    if K % 32 != 0:
        raise NotImplementedError(f"block-scaled activation quantisation needs K % 32 == 0, got K = {K}")
    m_pad = (M + group - 1) // group * group
    lib = _hip.load()
    if mode == "mxfp8":
        y = torch.empty((M, K), dtype=torch.float8_e4m3fn, device=tensor.device)
        fn = lib.gemlite_hip_scale_activations_mxfp8
    else:
        y = torch.empty((M, K // 2), dtype=torch.uint8, device=tensor.device)
        fn = lib.gemlite_hip_scale_activations_mxfp4 if mode == "mxfp4" else lib.gemlite_hip_scale_activations_nvfp4
    scales = torch.empty((m_pad, K // group), dtype=torch.uint8, device=tensor.device)
    with _hip.on_device(tensor.device):
        rc = fn(x2.data_ptr(), y.data_ptr(), scales.data_ptr(), M, K, x2.stride(0), TORCH_TO_DTYPE[x2.dtype].value,
                _hip.current_stream_handle(tensor.device))
    _hip.raise_for_status(rc, "scale_activations_" + mode)
    if mode == "nvfp4":
        scales = scales.view(torch.float8_e4m3fn)
    return y, scales


def scale_activations_mxfp8(tensor: torch.Tensor, w_dtype: torch.dtype = torch.float8_e4m3fn):
    if w_dtype != torch.float8_e4m3fn:
        raise NotImplementedError("MXFP8 activations are OCP e4m3 on gfx950")
    return _scale_activations_mx(tensor, "mxfp8")


def scale_activations_mxfp4(tensor: torch.Tensor):
    return _scale_activations_mx(tensor, "mxfp4")


def scale_activations_nvfp4(tensor: torch.Tensor):
    return _scale_activations_mx(tensor, "nvfp4")


# the reference's export names for the same entry points
scale_activations_mxfp8_triton_v2, scale_activations_mxfp4_triton_v2 = scale_activations_mxfp8, scale_activations_mxfp4
scale_activations_nvfp4_triton_v2 = scale_activations_nvfp4
