"""Guard-band tests of every writer in the C ABI (run on a real MI355X via `pytest -m gpu`).

Every entry of tests/test_abi_bounds_cpu.py::CASES calls gemlite_hip_forward directly, in three layouts:
  dense       contiguous tensors, each inside a larger allocation;
  aligned     x rows at stride K + 64 from 64 elements in; out a window at row 3, column 64, row stride N + 128, with guard rows
              behind it; w_q / scales / zeros offset views whose non-unit stride is 64 elements longer;
  misaligned  the same with every offset and stride extra cut to one element (nothing 16-byte aligned any more).
Before each call the whole output allocation holds 0xFF bytes (NaN in fp16 / bf16 / fp32) and the workspace is what the library asked
for, zeroed, plus 1 MiB of 0xFF.  After it: nothing outside the window changed, the window passes the float64 oracle with the gates of
test_gpu_parity, a guarded call on the same plan as the dense call is bit-identical to it, the workspace guard and the counters are
as they were, and no input byte changed.  The activation quantisers and the bit packers get the same output guard."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, _hip
from gemlite_amd.quant_utils import (scale_activations_mxfp4, scale_activations_mxfp8, scale_activations_nvfp4,
                                     scale_activations_per_token)
from oracle import gemlite_oracle as O
from oracle import mx_oracle as MX
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, kernel_name, plan_args, x_format
from tests.test_gpu_parity import _compare, _oracle_from_layer
from tests.test_mx_gpu import _oracle as _mx_oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 1 << 16  # bytes of guard behind every input view
WS_GUARD = 1 << 20
COUNTER_BYTES = 65536 * 4  # the arrival counters at the head of a workspace (gl_common.h)
# (offset, stride extra) in elements of each tensor's own dtype
LAYOUTS = {"dense": None, "aligned": 64, "misaligned": 1}


def _lib():
    return _hip.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _place(t, extra):
    """(view of t's values inside a fresh 0xFF-filled allocation, the allocation).  extra None: contiguous at a 256-byte offset;
    else offset `extra` elements and the non-unit stride `extra` elements longer."""
    if t.numel() == 0:
        return t, None
    t = t.detach()
    es = t.element_size()
    if t.dim() == 2 and t.shape[0] > 1 and t.shape[1] > 1 and t.stride(0) == 1:  # a transposed view: place its transpose
        v, buf = _place(t.t(), extra)
        return v.t(), buf
    flat = t.dim() != 2 or min(t.shape) == 1  # vectors, [N, 1] / [1, N] scales, scalar zeros: offset only, contiguous
    rows, cols = (1, t.numel()) if flat else tuple(t.shape)
    off = 256 // es if extra is None else extra
    rs = cols if (extra is None or flat) else cols + extra
    n = off + rows * rs + GUARD // es
    buf = torch.full((n * es,), 0xFF, dtype=torch.uint8, device=DEV).view(t.dtype)
    v = buf.as_strided((rows, cols), (rs, 1), off)
    v.copy_(t.reshape(rows, cols))
    return (v.view(t.shape) if flat else v), buf


def _raw(t):
    """the bits of a 16- / 32-bit tensor as integers"""
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _bytes(t):
    return t.contiguous().view(torch.uint8).clone() if t is not None else None


# ------------------------------------------------------------------------------------------------ oracle per (layer, M)
def _quantised_inputs(lin, x16, fused):
    """(x as the kernel reads it, scales_x tensor or None) of one call"""
    if fused:
        return x16, None
    code = lin.input_dtype
    if code in (DType.FP16, DType.BF16, DType.MXFP16, DType.MXBF16):
        return x16, None
    if code == DType.MXFP8:
        if lin.channel_scale_mode == 2:
            xq, sx = scale_activations_per_token(x16, w_dtype=torch.float8_e4m3fn)
            return xq, sx.reshape(-1).contiguous()
        return scale_activations_mxfp8(x16)
    if code == DType.MXFP4:
        return scale_activations_mxfp4(x16)
    if code == DType.NVFP4:
        return scale_activations_nvfp4(x16)
    qdt = torch.int8 if code == DType.INT8 else torch.float8_e4m3fn
    xq, sx = scale_activations_per_token(x16, w_dtype=qdt)
    return xq, sx.reshape(-1).contiguous()


def _oracle(lin, x16, name):
    """float64 result of the layer on x16 (16-bit activations; 8-bit and block-scaled layers quantise them like the library) as kernel
    `name` computes it"""
    code = lin.input_dtype
    if code in (DType.MXFP16, DType.MXBF16, DType.MXFP8, DType.MXFP4, DType.NVFP4):
        return _mx_oracle(lin, x16), None
    if code in (DType.FP16, DType.BF16):
        return _oracle_from_layer(lin, x16), 5e-3 if lin.elements_per_sample == 1 else 1e-3
    ocode = O.INT8 if code == DType.INT8 else O.FP8E4
    xq, sx = O.scale_activations_per_token(x16, ocode)
    if lin.elements_per_sample == 1:  # A8W8: integer / fp8 products, channel and token scales after the reduction
        return _oracle_from_layer(lin, torch.from_numpy(xq), scales_x=sx), 1e-3
    out_code = lin.output_dtype.value
    # fp8 activations x packed words: the dequantised weight is rounded to e4m3 before the dot (the one-row GEMV family keeps it in the
    # output type, like the reference's GEMV kernels), as in test_gpu_parity.test_a8wn_fp8_activations_on_the_mfma_kernel
    wcast = None if ocode == O.INT8 else (out_code if name.startswith("gemv_a8w") else O.FP8E4)
    z = O.to_f64(lin.zeros.data).reshape(-1) if lin.zeros.numel() == 1 else O.to_f64(lin.zeros.data)
    y = O.forward_packed(xq, lin.W_q.data.cpu().numpy(), O.to_f64(lin.scales.data), z, W_nbits=lin.W_nbits, group_size=lin.group_size,
                         W_group_mode=lin.W_group_mode, channel_scale_mode=lin.channel_scale_mode, scales_x=sx,
                         zero_is_scalar=lin.zeros.numel() == 1, weight_cast_code=wcast)
    return y, None


# ------------------------------------------------------------------------------------------------ one guarded call
def _run(lin, case, xk, sx, extra, w_extra="same", out_layout=None):
    """One gemlite_hip_forward of `case` in layout `extra` (w_q in layout `w_extra`; out_layout: (first column, row stride) of the output
    window instead); checks the guards and returns (window, kernel name, workspace bytes), or None where the library answers
    GEMLITE_ERR_NO_FUSED_QUANT (nothing launched, nothing written)."""
    M, N = case["M"], lin.out_features
    fused = case["fused"]
    w_extra = extra if w_extra == "same" else w_extra
    views = [_place(t, w_extra if i == 1 else extra) for i, t in enumerate((xk, lin.W_q.data, lin.scales.data, lin.zeros.data))]
    (xv, xbuf), (wv, wbuf), (sv, sbuf), (zv, zbuf) = views
    sxv, sxbuf = _place(sx, None) if sx is not None else (None, None)
    odt = gemlite_amd.dtypes.DTYPE_TO_TORCH[lin.output_dtype.value]  # (MXFP16 / MXBF16 outputs: fp16 / bf16)
    es = torch.empty((), dtype=odt).element_size()
    if extra is None:
        r0, c0, so, rows = 0, 256 // es, N, M + 64
    else:
        r0, c0, so = 3, extra, N + (2 * extra if extra > 1 else 1)
        if out_layout is not None:
            c0, so = out_layout
        rows = r0 + M + (M + 255) // 256 * 256 - M + 256
    obuf = torch.full((rows * so + c0 + 64,), float("nan"), dtype=odt, device=DEV)
    obuf.view(torch.uint8).fill_(0xFF)
    win = obuf.as_strided((M, N), (so, 1), r0 * so + c0)
    a = plan_args(lin, M, case["tuning"], fused, x=xv.data_ptr(), out=win.data_ptr(), stride_xm=xv.stride(0), stride_om=so,
                  tensors=(wv, sv, zv))
    if sxv is not None:
        a.scales_x = sxv.data_ptr()
        a.stride_sx_m = sxv.stride(0) if sxv.dim() == 2 else 1
    need = int(_lib().gemlite_hip_workspace_bytes(C.byref(a)))
    ws = torch.full((need + WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[:need].zero_()
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    name = kernel_name(a)
    before = [_bytes(b) for b in (xbuf, wbuf, sbuf, zbuf, sxbuf) if b is not None]
    rc = _lib().gemlite_hip_forward(C.byref(a), _stream())
    torch.cuda.synchronize()
    if fused and extra is not None and rc == _hip.ERR_NO_FUSED_QUANT:  # the documented answer where no fused kernel takes the views
        assert bool((_raw(obuf) == -1).all()), "refused call wrote its output"
        return None
    assert rc == 0, (name, _hip.status_string(rc))
    # 1. nothing outside the window changed
    mask = torch.ones(obuf.numel(), dtype=torch.bool, device=DEV)
    mask.as_strided((M, N), (so, 1), r0 * so + c0).fill_(False)
    changed = (_raw(obuf) != -1) & mask
    if changed.any():
        i = int(changed.nonzero()[0])
        rel = i - (r0 * so + c0)
        pytest.fail(f"{name}: store outside the window at (row {rel // so}, column {rel % so}) relative to it "
                    f"({int(changed.sum())} elements)")
    # 4. workspace guard untouched, counters back at zero
    assert bool((ws[need:] == 0xFF).all()), f"{name}: write past the {need} workspace bytes it asked for"
    if need >= COUNTER_BYTES:
        assert bool((ws[:COUNTER_BYTES] == 0).all()), f"{name}: arrival counters not left at zero"
    # 5. inputs untouched
    after = [_bytes(b) for b in (xbuf, wbuf, sbuf, zbuf, sxbuf) if b is not None]
    for i, (b0, b1) in enumerate(zip(before, after)):
        assert torch.equal(b0, b1), f"{name}: input {('x', 'w_q', 'scales', 'zeros', 'scales_x')[i]} changed"
    return win.clone(), name, need


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_kernel_stays_inside_its_window_under_views(case):
    r = case["recipe"]
    lin = build_layer(r, DEV)
    M, K = case["M"], lin.in_features
    assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
    tdt = torch.bfloat16 if lin.output_dtype in (DType.BF16, DType.MXBF16) else torch.float16
    x16 = torch.from_numpy(O.gen_x(M, K, seed=M).astype(np.float32)).to(tdt).to(DEV)
    xk, sx = _quantised_inputs(lin, x16, case["fused"])
    assert xk.element_size() == x_format(lin, case["fused"])[0].itemsize
    oracles = {}  # once per case and weight rounding: the three layouts compute the same thing
    out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    dense = None
    for lay, extra in LAYOUTS.items():
        res = _run(lin, case, xk, sx, extra)
        if res is None:
            continue
        y, name, need = res
        okey = name.startswith("gemv_a8w")
        if okey not in oracles:
            oracles[okey] = _oracle(lin, x16, name)
        y_ref, abs_gate = oracles[okey]
        if lay == "dense":
            assert name == case["name"], name
            dense = (y, name, need)
        _compare(f"bounds/{case_id(case)}/{lay}", y, y_ref, out_code, abs_gate=abs_gate, extra=dict(kernel=name))
        if lay != "dense" and (name, need) == dense[1:]:
            assert torch.equal(_raw(y), _raw(dense[0])), f"{name}: {lay} result differs from the dense one on the same plan"


@pytest.mark.parametrize("M,tuning,name", [(255, (0, 0, 0, 0), "gemm_w4_mma_kernel<64x64>"),
                                            (129, (0, 2, 4, 128), "gemm_w4_mma_kernel<128x128>")])
@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_lds_dma_word_tiles_with_a_misaligned_w_q(M, tuning, name, tdt):
    """The 4-bit 64 x 64 / 128 x 128 tiles fetch their packed words by 16-byte LDS-DMA only from a 16-byte aligned w_q and row stride.
    Here everything else is aligned and w_q sits 4 bytes off with row stride N + 1 words: the same kernel (on register loads) must match
    the oracle, and the aligned layout stays bit-identical to the dense one."""
    case = dict(recipe=dict(kind="wn", N=4096, K=4096, nbits=4, gs=128, tdt=tdt), M=M, tuning=tuning, fused=False, name=name)
    lin = build_layer(case["recipe"], DEV)
    x16 = torch.from_numpy(O.gen_x(M, 4096, seed=M).astype(np.float32)).to(tdt).to(DEV)
    y_ref = _oracle_from_layer(lin, x16)
    out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    y0, n0, _ = _run(lin, case, x16, None, None)
    assert n0 == name
    for w_extra in (64, 1):
        y, n, _ = _run(lin, case, x16, None, 64, w_extra=w_extra)
        assert n == name, n
        _compare(f"bounds/wl/{name}/M{M}/w{w_extra}", y, y_ref, out_code, extra=dict(kernel=n))
        if w_extra == 64:
            assert torch.equal(_raw(y), _raw(y0))


@pytest.mark.parametrize("M", [48, 64])
@pytest.mark.parametrize("out_layout", [(2, 4096 + 128), (64, 4096 + 2)], ids=["out_4_bytes_off", "stride_om_N+2"])
def test_group32_layers_on_an_output_the_tiles_decline_run_on_the_rows_kernel(M, out_layout):
    """A16W4 g32 4096^2 at M = 48 / 64: the 32-row tiles take the aligned request; an output 4 bytes off 8-byte alignment, or a row stride
    that is not a multiple of 4 outputs, goes to the rows kernel (not the streaming kernel) — which must then store exactly that window."""
    case = dict(recipe=dict(kind="wn", N=4096, K=4096, nbits=4, gs=32), M=M, tuning=(0, 0, 0, 0), fused=False, name="")
    lin = build_layer(case["recipe"], DEV)
    x16 = torch.from_numpy(O.gen_x(M, 4096, seed=M).astype(np.float32)).to(torch.float16).to(DEV)
    y_ref = _oracle_from_layer(lin, x16)
    y0, n0, _ = _run(lin, case, x16, None, 64)
    assert n0 == "gemm_w4_mma_kernel<32x128,g32>", n0
    _compare(f"bounds/g32/M{M}/tiles", y0, y_ref, 1, extra=dict(kernel=n0))
    y, n, _ = _run(lin, case, x16, None, 64, out_layout=out_layout)
    assert n.startswith("gemm_w4_rows_kernel<"), n
    _compare(f"bounds/g32/M{M}/{out_layout}", y, y_ref, 1, extra=dict(kernel=n))


# ------------------------------------------------------------------------------------------------ the other writers
def _guarded(shape, dtype, rows_valid=None):
    """(view [rows, cols] at row 3, column 64 of a 0xFF allocation with row stride cols + 128, the allocation, offset, row stride)"""
    rows, cols = shape
    rs = cols + 128
    n = (3 + rows + 64) * rs
    buf = torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xFF, dtype=torch.uint8, device=DEV).view(dtype)
    off = 3 * rs + 64
    return buf.as_strided((rows, cols), (rs, 1), off), buf, off, rs


def _outside_unchanged(buf, off, rs, rows, cols, what):
    m = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    m.as_strided((rows, cols), (rs, 1), off).fill_(False)
    u8 = buf.view(torch.uint8).reshape(buf.numel(), -1)
    bad = (u8 != 0xFF).any(dim=1) & m
    if bad.any():
        i = int(bad.nonzero()[0]) - off
        pytest.fail(f"{what}: store outside the window at (row {i // rs}, column {i % rs}) relative to it")


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("kind", ["int8", "fp8", "mxfp8", "mxfp4", "nvfp4"])
@pytest.mark.parametrize("M,K", [(1, 256), (17, 1024), (33, 4096)])
def test_activation_quantisers_stay_inside_their_outputs(kind, tdt, M, K):
    """x at row stride K + 64; y and the scales in guarded buffers.  Block scales are written up to M_pad rows and not one further;
    y and the scales (padded rows included) are bit-identical to the float64 oracle's quantisers."""
    lib = _lib()
    xb = torch.randn(M, K + 64, device=DEV).to(tdt)
    x = xb[:, 64:]
    in_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    xin = xb.clone()
    if kind in ("int8", "fp8"):
        qdt = torch.int8 if kind == "int8" else torch.float8_e4m3fn
        y, ybuf, yoff, yrs = _guarded((M, K), qdt)
        y = ybuf.as_strided((M, K), (K, 1), yoff)  # the per-token quantiser writes y contiguous: a guarded offset view
        s, sbuf, soff, srs = _guarded((1, M), torch.float32)
        rc = lib.gemlite_hip_scale_activations_per_token(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(s.data_ptr()),
                                                         M, K, x.stride(0), in_code, gemlite_amd.dtypes.TORCH_TO_DTYPE[qdt].value,
                                                         C.c_void_p(_stream()))
        torch.cuda.synchronize()
        assert rc == 0
        _outside_unchanged(ybuf, yoff, K, M, K, f"per-token {kind} y")
        _outside_unchanged(sbuf, soff, srs, 1, M, f"per-token {kind} scales")
        y_o, s_o = O.scale_activations_per_token(x, O.INT8 if kind == "int8" else O.FP8E4)  # the float64 oracle's quantiser
        assert np.array_equal(y.float().cpu().numpy().astype(np.float64), y_o)
        assert np.array_equal(s.reshape(-1).cpu().numpy(), s_o.reshape(-1))
    else:
        g = 16 if kind == "nvfp4" else 32
        mp = (M + g - 1) // g * g if kind == "nvfp4" else (M + 31) // 32 * 32
        yk = K if kind == "mxfp8" else K // 2
        ydt = torch.float8_e4m3fn if kind == "mxfp8" else torch.uint8
        ybuf = torch.full(((3 + M + 64) * yk,), 0xFF, dtype=torch.uint8, device=DEV).view(ydt)
        yoff = 3 * yk + 64
        y = ybuf.as_strided((M, yk), (yk, 1), yoff)
        sbuf = torch.full((256 + (mp + 64) * (K // g),), 0xFF, dtype=torch.uint8, device=DEV)
        soff = 256
        s = sbuf.as_strided((mp, K // g), (K // g, 1), soff)
        fn = {"mxfp8": lib.gemlite_hip_scale_activations_mxfp8, "mxfp4": lib.gemlite_hip_scale_activations_mxfp4,
              "nvfp4": lib.gemlite_hip_scale_activations_nvfp4}[kind]
        rc = fn(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(s.data_ptr()), M, K, x.stride(0), in_code, C.c_void_p(_stream()))
        torch.cuda.synchronize()
        assert rc == 0
        _outside_unchanged(ybuf, yoff, yk, M, yk, f"{kind} y")
        _outside_unchanged(sbuf, soff, K // g, mp, K // g, f"{kind} scales (M_pad = {mp})")
        y_o, s_o = getattr(MX, "scale_activations_" + kind)(x.float().cpu().numpy())  # the oracle's quantiser, padded rows included
        assert np.array_equal(y.contiguous().view(torch.uint8).cpu().numpy(), y_o)
        assert np.array_equal(s.contiguous().view(torch.uint8).cpu().numpy(), s_o)
    assert torch.equal(xb, xin), "x changed"


@pytest.mark.parametrize("nbits,pb", [(4, 32), (2, 32), (1, 32), (8, 32), (4, 8), (2, 16)])
@pytest.mark.parametrize("N,K", [(1000, 512), (64, 4096)])
def test_bit_packers_stay_inside_their_outputs(nbits, pb, N, K):
    """pack_over_cols from rows at ld_in = K + 64 into a guarded output; unpack_over_cols back into a guarded output; bit-exact both ways."""
    lib = _lib()
    e = pb // nbits
    Wb = torch.randint(0, 2 ** nbits, (N, K + 64), dtype=torch.uint8, device=DEV)
    W = Wb[:, 64:]
    Win = Wb.clone()
    pdt = {8: torch.uint8, 16: torch.int16, 32: torch.int32}[pb]
    esz = pb // 8
    prow = K // e
    pbuf = torch.full(((3 + prow + 64) * N * esz,), 0xFF, dtype=torch.uint8, device=DEV).view(pdt)
    poff = 3 * N + 64
    packed = pbuf.as_strided((prow, N), (N, 1), poff)
    rc = lib.gemlite_hip_pack_over_cols(C.c_void_p(W.data_ptr()), C.c_void_p(packed.data_ptr()), N, K, W.stride(0), nbits, pb, C.c_void_p(_stream()))
    torch.cuda.synchronize()
    assert rc == 0
    _outside_unchanged(pbuf, poff, N, prow, N, "pack_over_cols")
    assert torch.equal(Wb, Win)
    ubuf = torch.full(((3 + N + 64) * K,), 0xFF, dtype=torch.uint8, device=DEV)
    uoff = 3 * K + 64
    un = ubuf.as_strided((N, K), (K, 1), uoff)
    pin = pbuf.clone()
    rc = lib.gemlite_hip_unpack_over_cols(C.c_void_p(packed.data_ptr()), C.c_void_p(un.data_ptr()), N, K, nbits, pb, C.c_void_p(_stream()))
    torch.cuda.synchronize()
    assert rc == 0
    _outside_unchanged(ubuf, uoff, K, N, K, "unpack_over_cols")
    assert torch.equal(pbuf, pin)
    assert torch.equal(un, W)
