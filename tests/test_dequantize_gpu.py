"""The weight dequantiser on the GPU: gemlite_hip_dequantize against the torch restatement of its contract (tests/dequant_spec.py) bit
for bit — the three kernels, every layout and mode — then GemLiteLinear.dequantize on the layer of every processor, its agreement with
the matmul the layer runs, the round trip through the quantiser, the quantiser-level calls, views, guard bands, planted non-finite
metadata and graph capture.  Shapes are the smallest that reach each path of the kernels."""
import ctypes as C
import functools
import itertools
import types

import pytest
import torch

from gemlite_amd import GemLiteLinear, _hip, helper
from gemlite_amd.dtypes import DTYPE_TO_TORCH, TORCH_TO_DTYPE, DType
from gemlite_amd.quant_utils import WeightQuantizerINT, WeightQuantizerMXFP
from oracle import gemlite_oracle as orc
from tests import dequant_spec as ds
from tests.quant_int_spec import error_bound, half_spacing, planted_weights
from tests.quant_mx_spec import pack_nibbles, planted_weights_mx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# N below a tile | N and K ragged, K ends inside a 256-tile | several tiles along K | several tiles both ways, groups of 96 / 192 straddle
SHAPES = [(16, 128), (80, 320), (64, 1024), (200, 768)]
OUTS = [torch.float16, torch.bfloat16, torch.float32]
METAS = [torch.float16, torch.bfloat16]
# (W_group_mode, zeros): every mode with a scalar and a tensor zero where it has one
MODES = [(0, "none"), (2, "none"), (1, "scalar"), (1, "tensor"), (3, "scalar"), (3, "tensor"), (4, "tensor")]
MXFP8, MXFP4, NVFP4 = DType.MXFP8.value, DType.MXFP4.value, DType.NVFP4.value


def groups_of(K):
    return [g for g in (32, 64, 128, K) + ((96, 192) if K == 768 else ()) if K % g == 0]


def launch(out, W_q, scales, zeros, *, N, K, nbits, e, group, w_mode=0, c_mode=0, input_dtype=None, meta_strides=(0, 1), post=1.0):
    """Raw C ABI call: W_q [K/e, N] words or [K, N] elements (any strides), out any [N, K] view with unit inner stride."""
    a = _hip.DequantizeArgs()
    a.struct_size = C.sizeof(_hip.DequantizeArgs)
    a.w_q, a.out = W_q.data_ptr(), out.data_ptr()
    a.scales = scales.data_ptr() if scales is not None else None
    a.zeros = zeros.data_ptr() if zeros is not None else None
    a.N, a.K, a.ld_out, a.out_dtype = N, K, out.stride(0), TORCH_TO_DTYPE[out.dtype].value
    a.stride_wk, a.stride_wn = W_q.stride(0), W_q.stride(1)
    a.stride_meta_g, a.stride_meta_n = meta_strides
    a.W_nbits, a.group_size, a.elements_per_sample = nbits, group, e
    a.w_pack_bits, a.w_dtype = (W_q.element_size() * 8 if e > 1 else 0), TORCH_TO_DTYPE[W_q.dtype].value
    a.input_dtype = TORCH_TO_DTYPE[torch.float16].value if input_dtype is None else input_dtype
    a.meta_dtype = TORCH_TO_DTYPE[scales.dtype].value if scales is not None else 1
    a.zeros_dtype = TORCH_TO_DTYPE[zeros.dtype].value if zeros is not None else 1
    a.zero_is_scalar = int(zeros is not None and zeros.numel() == 1)
    a.W_group_mode, a.channel_scale_mode, a.post_scale = w_mode, c_mode, post
    rc = _hip.load().gemlite_hip_dequantize(C.byref(a), _hip.current_stream_handle(out.device))
    assert rc == 0, _hip.status_string(rc)


def check(got, want, what=""):
    assert ds.same(got, want), f"{what}: {ds.describe_mismatch(got, want)}"


def _meta(gen, shape, T, lo=-6, hi=6, signed=False):
    v = torch.exp2(torch.rand(shape, generator=gen) * (hi - lo) + lo)
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return v.to(T)


@functools.lru_cache(maxsize=None)
def codes(N, K, nbits):
    """random codes [N, K] on the CPU: computed once, shared, never modified"""
    return torch.randint(0, 2 ** nbits, (N, K), generator=torch.Generator().manual_seed(N + K + nbits)).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def words(N, K, nbits, bits):
    tdt = {32: torch.int32, 16: torch.int16, 8: torch.uint8}[bits]
    return torch.from_numpy(orc.pack_over_cols(codes(N, K, nbits).numpy(), nbits, bits)).view(tdt).to(DEV)


@functools.lru_cache(maxsize=None)
def metadata(N, K, g, T, signed, hi):
    gen = torch.Generator().manual_seed(N * 3 + K + g)
    return _meta(gen, (K // g, N), T), _meta(gen, (K // g, N), T, lo=-4, hi=hi, signed=signed)


def int_case(N, K, nbits, g, w_mode, zeros_kind, c_mode, T):
    """(scales, zeros) on the CPU in the layer's [K/g, N] layout and what the restatement makes of them with codes(N, K, nbits)"""
    s, z = metadata(N, K, g, T, w_mode == 4, nbits)
    need_s, need_z, chan = w_mode >= 2, w_mode in (1, 3, 4), c_mode in (1, 3)
    if chan and not need_s:  # the layer's [1, N] fp32 weight scale
        s = _meta(torch.Generator().manual_seed(N), (1, N), torch.float32, lo=-8, hi=2)
    if zeros_kind == "scalar":
        z = torch.tensor(2 ** (nbits - 1), dtype=torch.int32)
    sN = ds.expand_groups(s, g, K) if need_s else None
    zN = (z.float().reshape(1, 1) if zeros_kind == "scalar" else ds.expand_groups(z, g, K)) if need_z else None
    c = s[0].float() if chan else None
    return (s if (need_s or chan) else None), (z if need_z else None), (sN, zN, c)


def run_int(W_q, N, K, nbits, e, g, w_mode, zeros_kind, c_mode, T, out_dt, q_float):
    s, z, (sN, zN, c) = int_case(N, K, nbits, g, w_mode, zeros_kind, c_mode, T)
    out = torch.empty((N, K), dtype=out_dt, device=DEV)
    launch(out, W_q, None if s is None else s.to(DEV), None if z is None else z.to(DEV), N=N, K=K, nbits=nbits, e=e, group=g,
           w_mode=w_mode, c_mode=c_mode, meta_strides=(N, 1))
    want = ds.dequant_int_spec(q_float, sN, zN, c, w_mode, out_dt)
    check(out, want, f"{N}x{K} {nbits}-bit g{g} mode {w_mode} {zeros_kind} c{c_mode} {T} -> {out_dt}")


# ------------------------------------------------------------------------------------------------ kernel == restatement, bit for bit
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("N,K", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_packed_words_match_the_restatement(N, K, nbits):
    """32-bit words, the tiled kernel: every mode x channel mode x group; metadata and result types take turns"""
    W_q, q_float = words(N, K, nbits, 32), codes(N, K, nbits).float()
    for i, ((w_mode, zk), c_mode, g) in enumerate(itertools.product(MODES, (0, 1, 3), groups_of(K))):
        run_int(W_q, N, K, nbits, 32 // nbits, g, w_mode, zk, c_mode, METAS[i % 2], OUTS[i % 3], q_float)


@pytest.mark.parametrize("T", METAS, ids=["fp16", "bf16"])
@pytest.mark.parametrize("out_dt", OUTS, ids=["fp16", "bf16", "fp32"])
def test_every_type_pair_on_the_tiled_kernel(out_dt, T):
    N, K = 80, 320
    for nbits, (w_mode, zk) in itertools.product((8, 4, 2, 1), MODES):
        run_int(words(N, K, nbits, 32), N, K, nbits, 32 // nbits, 64, w_mode, zk, 0, T, out_dt, codes(N, K, nbits).float())


@pytest.mark.parametrize("form", ["b8", "b16", "not_contiguous", "group_20_or_24"])
@pytest.mark.parametrize("N,K", [(80, 320), (200, 768)], ids=["80x320", "200x768"])
def test_general_path_matches_the_restatement(N, K, form):
    """8- / 16-bit words, a contiguous=False pack (words [N, K/e] seen as [K/e, N]), a group that is no multiple of 8"""
    for i, (nbits, (w_mode, zk)) in enumerate(itertools.product((8, 4, 2, 1), MODES)):
        bits = {"b8": 8, "b16": 16}.get(form, 32)
        W_q = words(N, K, nbits, bits)
        if form == "not_contiguous":
            W_q = W_q.t().contiguous().t()
            assert W_q.stride() == (1, K * nbits // 32)
        g = (20 if K == 320 else 24) if form == "group_20_or_24" else 64
        run_int(W_q, N, K, nbits, bits // nbits, g, w_mode, zk, (0, 1, 3)[i % 3], METAS[i % 2], OUTS[i % 3], codes(N, K, nbits).float())


@pytest.mark.parametrize("wdt", [torch.int8, torch.float8_e4m3fn, torch.float8_e5m2, torch.uint8, torch.float16, torch.bfloat16, torch.float32],
                         ids=["int8", "e4m3", "e5m2", "uint8", "fp16", "bf16", "fp32"])
@pytest.mark.parametrize("N,K", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_unpacked_elements_match_the_restatement(N, K, wdt):
    """[N, K] elements handed on as the [K, N] view, like pack() does: the streaming kernel (8-bit), the general path (16- / 32-bit)"""
    gen = torch.Generator().manual_seed(K)
    byt = torch.randint(0, 256, (N, K), generator=gen).to(torch.uint8)
    if wdt == torch.float8_e4m3fn:
        byt[(byt & 0x7F) == 0x7F] = 0x41  # finite elements (NaN elements: test_non_finite below)
    if wdt == torch.float8_e5m2:
        byt[(byt & 0x7F) >= 0x7C] = 0x41
    # float elements: multiples of 2^-10 below 8, so that q * s + z' stays exact in the restatement's float64 (dequant_spec.fma_once asserts it)
    W = byt.view(wdt) if wdt.itemsize == 1 else (torch.round(torch.randn(N, K, generator=gen).clamp(-2.6, 2.6) * 3072) / 1024).to(wdt)
    Wd = W.to(DEV)
    q_float = W.float()
    nbits = wdt.itemsize * 8
    for i, ((w_mode, zk), c_mode, g) in enumerate(itertools.product(MODES, (0, 1, 3), (64, K))):
        s, z, (sN, zN, c) = int_case(N, K, 4, g, w_mode, zk, c_mode, METAS[i % 2])
        out = torch.empty((N, K), dtype=OUTS[i % 3], device=DEV)
        launch(out, Wd.t(), None if s is None else s.to(DEV), None if z is None else z.to(DEV), N=N, K=K, nbits=nbits, e=1, group=g,
               w_mode=w_mode, c_mode=c_mode, meta_strides=(N, 1))
        check(out, ds.dequant_int_spec(q_float, sN, zN, c, w_mode, out.dtype), f"{wdt} {N}x{K} g{g} mode {w_mode} {zk} c{c_mode}")


def _mx_case(N, K, fmt, seed=0):
    """(element bytes [N, K] uint8: e4m3 or one e2m1 code per byte, scale bytes [N, K/g], element values fp32) with one NaN block planted"""
    g = 16 if fmt == "nvfp4" else 32
    gen = torch.Generator().manual_seed(N + K + seed)
    if fmt == "mxfp8":
        el = torch.randint(0, 256, (N, K), generator=gen).to(torch.uint8)
        el[(el & 0x7F) == 0x7F] = 0x33
        val = el.view(torch.float8_e4m3fn).float()
        sb = torch.randint(97, 140, (N, K // g), generator=gen).to(torch.uint8)
    else:
        el = torch.randint(0, 16, (N, K), generator=gen).to(torch.uint8)
        val = ds.E2M1[el.long()]
        sb = (torch.randint(0x08, 0x7F, (N, K // g), generator=gen) if fmt == "nvfp4" else torch.randint(97, 160, (N, K // g), generator=gen)).to(torch.uint8)
    sb[N // 2, (K // g) // 2] = 0x7F if fmt == "nvfp4" else 0xFF
    return el, sb, val, g


@pytest.mark.parametrize("scale_layout", ["by_group", "by_row"])
@pytest.mark.parametrize("fmt,form", [("mxfp8", "layer"), ("mxfp4", "layer"), ("mxfp4", "codes"), ("nvfp4", "layer"), ("nvfp4", "codes")])
@pytest.mark.parametrize("N,K", [(16, 128), (80, 320), (64, 1024)], ids=["16x128", "80x320", "64x1024"])
def test_block_scaled_match_the_restatement(N, K, fmt, form, scale_layout):
    """layer: fp8 [N, K] / two codes per byte [N, K/2] seen as the [K(/2), N] view; codes: one code per byte.  Scales [K/g, N] or [N, K/g]"""
    el, sb, val, g = _mx_case(N, K, fmt)
    nibbles = fmt != "mxfp8" and form == "layer"
    W = (pack_nibbles(el) if nibbles else el).to(DEV)
    W = W.view(torch.float8_e4m3fn) if fmt == "mxfp8" else W
    if scale_layout == "by_group":
        S, strides = sb.t().contiguous().to(DEV), (N, 1)
    else:
        S, strides = sb.contiguous().to(DEV), (1, K // g)
    in_dt = {"mxfp8": MXFP8, "mxfp4": MXFP4, "nvfp4": NVFP4}[fmt]
    for out_dt, post in itertools.product(OUTS, (1.0, 0.05) if fmt == "nvfp4" else (1.0,)):
        out = torch.empty((N, K), dtype=out_dt, device=DEV)
        launch(out, W.t(), S, None, N=N, K=K, nbits=8 if fmt == "mxfp8" else 4, e=2 if nibbles else 1, group=g, input_dtype=in_dt,
               meta_strides=strides, post=post)
        want = ds.dequant_mx_spec(val, sb, g, fmt == "nvfp4", out_dt, post)
        check(out, want, f"{fmt} {form} {scale_layout} -> {out_dt} post {post}")
        bad = torch.isnan(want)
        assert int(bad.sum()) == g and bad[N // 2, (K // g) // 2 * g:(K // g) // 2 * g + g].all()  # the planted NaN scale: its block, nothing else
    # the same through the general path: a weight view that is not K-contiguous
    Wn = W.t().contiguous()
    out = torch.empty((N, K), dtype=torch.float32, device=DEV)
    launch(out, Wn, S, None, N=N, K=K, nbits=8 if fmt == "mxfp8" else 4, e=2 if nibbles else 1, group=g, input_dtype=in_dt, meta_strides=strides)
    check(out, ds.dequant_mx_spec(val, sb, g, fmt == "nvfp4", torch.float32), f"{fmt} general path")


# ------------------------------------------------------------------------------------------------ every processor
def _linear(N, K, dtype, seed=0, bias=False):
    lin = torch.nn.Linear(K, N, bias=bias, dtype=dtype, device=DEV)
    with torch.no_grad():
        lin.weight.copy_((torch.randn(N, K, generator=torch.Generator().manual_seed(seed + N + K)) * 0.05).to(dtype))
    return lin


def _hqq_tensors(N, K, nbits, g, dtype, seed=0):
    return WeightQuantizerINT(nbits, g, dtype=dtype).quantize(_linear(N, K, dtype, seed).weight.data)


def _bitlinear(N, K, dtype):
    w = torch.randint(-1, 2, (N, K), generator=torch.Generator().manual_seed(N)).to(dtype).to(DEV)
    return types.SimpleNamespace(weight=w, weight_scale=torch.tensor(0.0371), bias=None)


def _packed(N, K, nbits, g, bits, dtype, **kw):
    layer = GemLiteLinear(nbits, group_size=g, in_features=K, out_features=N, input_dtype=TORCH_TO_DTYPE[dtype], output_dtype=TORCH_TO_DTYPE[dtype])
    q, s, z = _hqq_tensors(N, K, nbits, g, dtype)
    return layer.pack(q, s, z, packing_bitwidth=bits, **kw)


F16, B16 = torch.float16, torch.bfloat16
# name -> (builder(N, K), runs on 16-bit activations: compared with the matmul as well)
PROCESSORS = {
    "A16W8_INT8": (lambda N, K: helper.A16W8_INT8(device=DEV).from_linear(_linear(N, K, F16)), True),
    "A16W8_INT8_post_scale": (lambda N, K: helper.A16W8_INT8(device=DEV, post_scale=True).from_linear(_linear(N, K, B16)), True),
    "A16W8_FP8": (lambda N, K: helper.A16W8_FP8(device=DEV).from_linear(_linear(N, K, B16)), True),
    "A16W8_FP8_post_scale": (lambda N, K: helper.A16W8_FP8(device=DEV, post_scale=True).from_linear(_linear(N, K, F16)), True),
    "A16W8_HQQ_INT": (lambda N, K: helper.A16W8_HQQ_INT(device=DEV).from_weights(*_hqq_tensors(N, K, 8, 64, F16), 8, 64), True),
    "A16W4_HQQ_INT": (lambda N, K: helper.A16W4_HQQ_INT(device=DEV).from_weights(*_hqq_tensors(N, K, 4, 64, B16), 4, 64), True),
    "A16W4_HQQ_INT_channelwise": (lambda N, K: helper.A16W4_HQQ_INT(device=DEV).from_weights(*_hqq_tensors(N, K, 4, K, F16), 4, K), True),
    "A16W2_HQQ_INT": (lambda N, K: helper.A16W2_HQQ_INT(device=DEV).from_weights(*_hqq_tensors(N, K, 2, 32, F16), 2, 32), True),
    "A16W1_HQQ_INT": (lambda N, K: helper.A16W1_HQQ_INT(device=DEV).from_weights(*_hqq_tensors(N, K, 1, 64, F16), 1, 64), True),
    "A16W8_RTN_INT": (lambda N, K: helper.A16W8_RTN_INT(device=DEV).from_linear(_linear(N, K, B16), group_size=64), True),
    "A16W4_RTN_INT": (lambda N, K: helper.A16W4_RTN_INT(device=DEV).from_linear(_linear(N, K, F16), group_size=64), True),
    "A16W2_RTN_INT": (lambda N, K: helper.A16W2_RTN_INT(device=DEV).from_linear(_linear(N, K, F16), group_size=32), True),
    "A16W1_RTN_INT": (lambda N, K: helper.A16W1_RTN_INT(device=DEV).from_linear(_linear(N, K, B16), group_size=64), True),
    "A8W4_HQQ_INT_dynamic": (lambda N, K: helper.A8W4_HQQ_INT_dynamic(device=DEV).from_weights(*_hqq_tensors(N, K, 4, 64, F16)), False),
    "A8W2_HQQ_INT_dynamic": (lambda N, K: helper.A8W2_HQQ_INT_dynamic(device=DEV).from_weights(*_hqq_tensors(N, K, 2, 64, B16)), False),
    "A8W4_HQQ_INT_dynamic_channelwise": (lambda N, K: helper.A8W4_HQQ_INT_dynamic(device=DEV).from_weights(*_hqq_tensors(N, K, 4, K, F16)), False),
    "A8W4_RTN_INT_dynamic": (lambda N, K: helper.A8W4_RTN_INT_dynamic(device=DEV).from_linear(_linear(N, K, F16), group_size=64), False),
    "A8W2_RTN_INT_dynamic": (lambda N, K: helper.A8W2_RTN_INT_dynamic(device=DEV).from_linear(_linear(N, K, F16), group_size=64), False),
    "A16W158_INT": (lambda N, K: helper.A16W158_INT(device=DEV).from_bitlinear(_bitlinear(N, K, F16), del_orig=False), True),
    "A8W158_INT_dynamic": (lambda N, K: helper.A8W158_INT_dynamic(device=DEV).from_bitlinear(_bitlinear(N, K, B16), del_orig=False), False),
    "A8W8_int8_dynamic": (lambda N, K: helper.A8W8_int8_dynamic(device=DEV).from_linear(_linear(N, K, F16)), False),
    "A8W8_fp8_dynamic": (lambda N, K: helper.A8W8_fp8_dynamic(device=DEV).from_linear(_linear(N, K, B16)), False),
    "A16W8_MXFP": (lambda N, K: helper.A16W8_MXFP(device=DEV, dtype=B16).from_linear(_linear(N, K, B16)), True),
    "A16W4_MXFP": (lambda N, K: helper.A16W4_MXFP(device=DEV, dtype=F16).from_linear(_linear(N, K, F16)), True),
    "A8W8_MXFP_dynamic": (lambda N, K: helper.A8W8_MXFP_dynamic(device=DEV, dtype=B16).from_linear(_linear(N, K, B16)), False),
    "A8W4_MXFP_dynamic": (lambda N, K: helper.A8W4_MXFP_dynamic(device=DEV, dtype=B16, post_scale=False).from_linear(_linear(N, K, B16)), False),
    "A4W4_MXFP_dynamic": (lambda N, K: helper.A4W4_MXFP_dynamic(device=DEV, dtype=F16).from_linear(_linear(N, K, F16)), False),
    "A4W4_NVFP_dynamic": (lambda N, K: helper.A4W4_NVFP_dynamic(device=DEV, dtype=B16).from_linear(_linear(N, K, B16)), False),
    "pack_32bit": (lambda N, K: _packed(N, K, 4, 64, 32, F16), True),
    "pack_16bit": (lambda N, K: _packed(N, K, 4, 64, 16, F16), True),
    "pack_8bit": (lambda N, K: _packed(N, K, 2, 64, 8, B16), True),
    "pack_32bit_mode3": (lambda N, K: _packed(N, K, 4, 64, 32, B16, fma_mode=False), True),
    "pack_32bit_not_contiguous": (lambda N, K: _packed(N, K, 4, 64, 32, F16, contiguous=False), True),
}


@pytest.mark.parametrize("N,K", [(80, 320), (64, 1024)], ids=["80x320", "64x1024"])
@pytest.mark.parametrize("name", list(PROCESSORS))
def test_every_processor(name, N, K):
    layer = PROCESSORS[name][0](N, K)
    default = layer.dequantize()
    assert tuple(default.shape) == (N, K) and default.dtype in (F16, B16) and default.is_cuda
    assert default.dtype == (layer.compute_dtype if layer.compute_dtype in (F16, B16) else DTYPE_TO_TORCH[layer.output_dtype.value])
    results = {}
    for dt in OUTS:
        results[dt] = layer.dequantize(dt)
        check(results[dt], ds.layer_spec(*layer.get_tensor_args(), layer.get_meta_args(), dt), f"{name} -> {dt}")
    check(default, results[default.dtype], "default dtype")
    # ... from the registered tensors and the metadata alone: a state_dict round trip changes nothing
    fresh = GemLiteLinear(layer.W_nbits, group_size=layer.group_size, in_features=K, out_features=N, input_dtype=layer.input_dtype,
                          output_dtype=layer.output_dtype)
    fresh.load_state_dict({k: v.clone() for k, v in layer.state_dict().items()})
    for dt in OUTS:
        check(fresh.dequantize(dt), results[dt], f"{name} after load_state_dict -> {dt}")


@pytest.mark.parametrize("N,K", [(64, 128), (80, 320)], ids=["64x128", "80x320"])
@pytest.mark.parametrize("name", [n for n, (_, a16) in PROCESSORS.items() if a16])
def test_agrees_with_the_matmul_the_layer_runs(name, N, K):
    """layer(I) is the matmul kernels' own dequantisation: a transposed tile or a wrong group index shows here, whatever the restatement says"""
    layer = PROCESSORS[name][0](N, K)
    dt = layer.compute_dtype
    y = layer(torch.eye(K, dtype=dt, device=DEV)).float()
    want = layer.dequantize(torch.float32).t()
    tol = 1e-3 if dt == F16 else 4e-3
    err = (y - want).abs()
    gate = 10 * tol * want.abs().mean() + 4 * tol * want.abs()
    print(f"{name} {N}x{K}: max err {err.max().item():.3e}, max err / gate {(err / gate).max().item():.3f}")
    assert torch.isfinite(y).all() and bool((err <= gate).all())


# ------------------------------------------------------------------------------------------------ round trip
@pytest.mark.parametrize("T", METAS, ids=["fp16", "bf16"])
def test_round_trip_meets_the_quantisers_bound(T):
    N, K, g, nbits = 80, 320, 64, 4
    W = planted_weights(N, K, g, T, seed=21).to(DEV)
    q, s, z = WeightQuantizerINT(nbits, g, dtype=T).quantize(W)
    s_r, z_r = s.cpu().float().view(N, K // g), z.cpu().float().view(N, K // g)
    bound = error_bound(nbits, s_r, z_r, T).repeat_interleave(g, dim=1)
    layer3 = GemLiteLinear(nbits, group_size=g, in_features=K, out_features=N, input_dtype=TORCH_TO_DTYPE[T], output_dtype=TORCH_TO_DTYPE[T])
    layer3.pack(q, s, z, fma_mode=False)
    assert layer3.W_group_mode == 3
    err = (layer3.dequantize(torch.float32).cpu() - W.cpu().float()).abs()
    print(f"mode 3: max (err - bound) = {(err - bound).max().item():.3e}")
    assert bool((err <= bound).all())
    lin = torch.nn.Linear(K, N, bias=False, dtype=T, device=DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
    layer4 = helper.A16W4_RTN_INT(device=DEV).from_linear(lin, group_size=g)
    assert layer4.W_group_mode == 4
    zf = layer4.zeros.detach().cpu().float().t()  # [N, K/g] folded zeros: their rounding adds half a unit of T at |z'|
    err = (layer4.dequantize(torch.float32).cpu() - W.cpu().float()).abs()
    bound4 = bound + half_spacing(zf, T).repeat_interleave(g, dim=1)
    print(f"mode 4: max (err - bound) = {(err - bound4).max().item():.3e}")
    assert bool((err <= bound4).all())


# ------------------------------------------------------------------------------------------------ quantiser-level calls
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("N,K,g", [(80, 320, 64), (200, 768, 96)], ids=["80x320g64", "200x768g96"])
def test_weight_quantizer_int_dequantize(N, K, g, nbits):
    T = torch.float16 if nbits % 4 == 0 else torch.bfloat16
    W = planted_weights(N, K, g, T, seed=5).to(DEV)
    wq = WeightQuantizerINT(nbits, g, dtype=T)
    q, s, z = wq.quantize(W)
    sN, zN = (t.cpu().float().view(N, K // g).repeat_interleave(g, dim=1) for t in (s, z))
    for dt in (None, torch.float32):
        got = wq.dequantize(q, s, z, dtype=dt)
        check(got, ds.dequant_int_spec(q.cpu().float(), sN, zN, None, 3, T if dt is None else dt), "quantize()")
    check(wq.dequantize(q.view(-1), s, z, shape=(N, K), dtype=torch.float32), ds.dequant_int_spec(q.cpu().float(), sN, zN, None, 3, torch.float32))
    for fold in (False, True):
        qp, sp, zp = wq.quantize_packed(W, fold_zeros=fold)
        want = ds.dequant_int_spec(ds.unpack_words(qp, nbits).float(), ds.expand_groups(sp, g, K), ds.expand_groups(zp, g, K), None,
                                   4 if fold else 3, torch.float32)
        check(wq.dequantize(qp, sp, zp, dtype=torch.float32, fold_zeros=fold), want, f"quantize_packed(fold_zeros={fold})")


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4", "nvfp4"])
@pytest.mark.parametrize("dt", [None, torch.float16, torch.float32], ids=["default", "fp16", "fp32"])
def test_weight_quantizer_mxfp_dequantize_keeps_its_bits(fmt, dt):
    N, K = 80, 320
    W = planted_weights_mx(N, K, torch.bfloat16, seed=3).to(DEV)
    wq = WeightQuantizerMXFP(compute_dtype=torch.bfloat16, device=DEV)
    q, s = {"mxfp8": wq.quantize_mxfp8, "mxfp4": wq.quantize_mxfp4, "nvfp4": wq.quantize_nvfp4}[fmt](W, index=True)
    assert wq._dequantize_kernel(q, s, None, torch.float32) is not None  # these inputs take the kernel
    cpu = WeightQuantizerMXFP(compute_dtype=torch.bfloat16, device="cpu")
    for shape in (None, (N, K)):
        got = wq.dequantize(q, s, shape=shape, dtype=dt)
        want = cpu.dequantize(q.cpu(), s.cpu(), shape=shape, dtype=dt)  # the torch code
        assert got.is_cuda and got.shape == want.shape
        check(got, want, f"{fmt} shape {shape}")
    # what the kernel does not take stays on the torch code, on the GPU
    vals = wq.dequantize(q, s, dtype=torch.float32)
    assert wq._dequantize_kernel(vals, s, None, torch.float32) is None
    assert wq._dequantize_kernel(q, s, None, torch.float64) is None
    check(wq.dequantize(q, s, dtype=torch.float64).float(), vals)


# ------------------------------------------------------------------------------------------------ views, alignment, guard bands
@pytest.mark.parametrize("kind", ["words", "bytes", "mxfp4"])
@pytest.mark.parametrize("out_dt", OUTS, ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("offset", [8, 3], ids=["aligned", "odd"])
def test_guard_bands(offset, out_dt, kind):
    """out as a window of a larger matrix (ld_out > K): 16-byte aligned it takes the tiled kernels, at an odd element offset the general
    path; nothing outside the window changes either way"""
    N, K, g = 80, 320, 64
    buf = torch.full((N + 2, K + 24), 7.0, dtype=out_dt, device=DEV)
    win = buf[1:1 + N, offset:offset + K]
    assert (win.data_ptr() % 16 == 0) == (offset == 8) and win.stride(0) == K + 24
    before = buf.clone()
    if kind == "words":
        s, z, (sN, zN, c) = int_case(N, K, 4, g, 4, "tensor", 0, torch.float16)
        launch(win, words(N, K, 4, 32), s.to(DEV), z.to(DEV), N=N, K=K, nbits=4, e=8, group=g, w_mode=4, meta_strides=(N, 1))
        want = ds.dequant_int_spec(codes(N, K, 4).float(), sN, zN, None, 4, out_dt)
    elif kind == "bytes":
        s, z, (sN, zN, c) = int_case(N, K, 8, K, 2, "none", 0, torch.bfloat16)
        W = codes(N, K, 8).view(torch.int8)
        launch(win, W.to(DEV).t(), s.to(DEV), None, N=N, K=K, nbits=8, e=1, group=K, w_mode=2, meta_strides=(N, 1))
        want = ds.dequant_int_spec(W.float(), sN, None, None, 2, out_dt)
    else:
        el, sb, val, gg = _mx_case(N, K, "mxfp4", seed=1)
        launch(win, pack_nibbles(el).to(DEV).t(), sb.t().contiguous().to(DEV), None, N=N, K=K, nbits=4, e=2, group=gg, input_dtype=MXFP4,
               meta_strides=(N, 1))
        want = ds.dequant_mx_spec(val, sb, gg, False, out_dt)
    torch.cuda.synchronize()
    check(win, want, f"{kind} window at {offset}")
    outside = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(outside, win.shape, win.stride(), win.storage_offset()).fill_(False)
    assert torch.equal(buf[outside], before[outside])


def test_layer_out_argument_takes_a_row_strided_view():
    layer = PROCESSORS["A16W4_RTN_INT"][0](80, 320)
    buf = torch.zeros((80, 400), dtype=torch.float32, device=DEV)
    got = layer.dequantize(out=buf[:, 40:360])
    assert got.data_ptr() == buf[:, 40:360].data_ptr() and not buf[:, :40].any() and not buf[:, 360:].any()
    check(got, layer.dequantize(torch.float32))
    with pytest.raises(ValueError):
        layer.dequantize(out=buf[:, :100])
    with pytest.raises(ValueError):
        layer.dequantize(torch.float16, out=buf[:, 40:360])


@pytest.mark.parametrize("path", ["tiled", "general"])
def test_non_finite_metadata_stays_in_its_group(path):
    """a NaN scale in one (group, row) and an Inf zero in another: exactly those groups' elements, and nothing faults"""
    N, K, g, nbits = 80, 320, 64, 4
    s, z, _ = int_case(N, K, nbits, g, 3, "tensor", 0, torch.float16)
    s, z = s.clone(), z.clone()
    s[1, 70], z[3, 5] = float("nan"), float("inf")
    bits = 32 if path == "tiled" else 16
    out = torch.empty((N, K), dtype=torch.float32, device=DEV)
    launch(out, words(N, K, nbits, bits), s.to(DEV), z.to(DEV), N=N, K=K, nbits=nbits, e=bits // nbits, group=g, w_mode=3, meta_strides=(N, 1))
    want = ds.dequant_int_spec(codes(N, K, nbits).float(), ds.expand_groups(s, g, K), ds.expand_groups(z, g, K), None, 3, torch.float32)
    check(out, want)
    out = out.cpu()
    nan, inf = torch.isnan(out), torch.isinf(out)
    assert int(nan.sum()) == g and nan[70, g:2 * g].all()
    assert int(inf.sum()) == g and inf[5, 3 * g:4 * g].all()


def test_non_finite_elements_and_overflow():
    N, K = 16, 128
    byt = torch.arange(N * K, dtype=torch.int64).remainder(256).to(torch.uint8).reshape(N, K)  # every e4m3 / e5m2 byte, NaN and Inf included
    s = torch.full((1, N), 300.0, dtype=torch.float32)
    for wdt in (torch.float8_e4m3fn, torch.float8_e5m2):
        for out_dt in OUTS:
            out = torch.empty((N, K), dtype=out_dt, device=DEV)
            launch(out, byt.view(wdt).to(DEV).t(), s.to(DEV), None, N=N, K=K, nbits=8, e=1, group=K, w_mode=2, meta_strides=(N, 1))
            want = ds.dequant_int_spec(byt.view(wdt).float(), s.t().expand(N, K), None, None, 2, out_dt)
            check(out, want, f"{wdt} -> {out_dt}")
            if out_dt == torch.float16:
                assert torch.isinf(want).any() and torch.isnan(want).any()  # 448 * 300 overflows fp16; the NaN bytes stay NaN


# ------------------------------------------------------------------------------------------------ determinism, capture
def test_deterministic():
    layer = PROCESSORS["A16W4_HQQ_INT"][0](200, 768)
    a, b = layer.dequantize(torch.bfloat16), layer.dequantize(torch.bfloat16)
    check(a, b)


@pytest.mark.parametrize("name", ["A16W4_RTN_INT", "A8W8_fp8_dynamic", "A4W4_NVFP_dynamic", "pack_16bit"])
def test_capturable_on_a_side_stream(name):
    layer = PROCESSORS[name][0](80, 320)
    want = layer.dequantize(torch.bfloat16)
    out = torch.zeros_like(want)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):  # (captures on a side stream)
        layer.dequantize(out=out)
    assert not out.any()  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    check(out, want)
