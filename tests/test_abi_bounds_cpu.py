"""Guard-band case table (no GPU): one launch site per entry of CASES — a layer recipe, an M, a tuning[4] and the kernel the planner
must pick for it.  tests/test_abi_bounds_gpu.py runs every entry through gemlite_hip_forward with guarded, strided and misaligned
views; this module checks, on the CPU, that every entry still reaches the kernel it names, that every kernel the planner fuzz
reaches has an entry, and the planner properties the guard-band work brought with it.

Out of scope (not in CASES): the `make AB=1`-only forms and the GL_MMA_EXPERIMENTS builds (not in the shipped library)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear, _hip
from gemlite_amd import helper as H
from gemlite_amd.core import _static_args
from oracle import gemlite_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def _layer_wn(N, K, nbits, gs, tdt, device, seed):
    W_q, scales, zeros = O.gen_data(N, K, nbits, gs, seed=seed, np_float=np.float16)
    lin = GemLiteLinear(nbits, gs, K, N, gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt], gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt])
    lin.pack(torch.from_numpy(W_q).to(device), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(device),
             torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(device), None, fma_mode=True)
    return lin


def _mx_weights(N, K, nbits, group, g):
    if nbits == 8:  # e4m3 codes without NaN (0x7f / 0xff), magnitudes up to ~2
        b = torch.randint(0, 0x40, (N, K), generator=g, dtype=torch.uint8) | (torch.randint(0, 2, (N, K), generator=g, dtype=torch.uint8) << 7)
        w = b.view(torch.float8_e4m3fn)
    else:
        w = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    if group == 16:
        s = (torch.rand(N, K // 16, generator=g) * 3 + 0.5).to(torch.float8_e4m3fn)
    else:
        s = torch.randint(122, 129, (N, K // group), generator=g, dtype=torch.uint8)
    return w, s


def build_layer(r, device="cpu", seed=0):
    """The GemLiteLinear of recipe r = dict(kind, N, K, ...) on `device` (random weights, fixed seed)."""
    kind, N, K = r["kind"], r["N"], r["K"]
    g = torch.Generator().manual_seed(seed)
    tdt = r.get("tdt", torch.float16)
    if kind == "wn":
        return _layer_wn(N, K, r["nbits"], r["gs"], tdt, device, seed)
    if kind == "bitnet16":
        return H.A16W158_INT(device=device).from_weights(torch.randint(-1, 2, (N, K), generator=g).half(), torch.tensor(0.02))
    if kind == "bitnet8":
        return H.A8W158_INT_dynamic(device=device).from_weights(torch.randint(-1, 2, (N, K), generator=g).half(), torch.tensor(0.02))
    if kind in ("a16w8i", "a16w8f"):
        W = (torch.randn(N, K, generator=g) / 30).to(tdt)
        proc = H.A16W8(device=device, post_scale=r.get("post", False)) if kind == "a16w8i" else H.A16W8_FP8(device=device)
        return proc.from_weights(W)
    if kind in ("a8w8i", "a8w8f"):
        W = (torch.randn(N, K, generator=g) / 30).to(tdt)
        proc = H.A8W8_int8_dynamic(device=device, dtype=tdt) if kind == "a8w8i" else H.A8W8_fp8_dynamic(device=device, dtype=tdt)
        return proc.from_weights(W)
    if kind in ("a8w4", "a8w2"):
        nbits = 4 if kind == "a8w4" else 2
        W_q, sc, zr = O.gen_data(N, K, nbits, r["gs"], seed=seed)
        return H.A8Wn_HQQ_INT_dynamic(device=device, dtype=tdt, W_nbits=nbits).from_weights(
            torch.from_numpy(W_q), torch.from_numpy(sc).to(tdt), torch.from_numpy(zr).to(tdt))
    if kind in ("mx16w8", "mx16w4"):
        w, s = _mx_weights(N, K, 8 if kind == "mx16w8" else 4, 32, g)
        return (H.A16W8_MXFP if kind == "mx16w8" else H.A16W4_MXFP)(device=device, dtype=tdt).from_weights(w.to(device), s.to(device))
    if kind in ("mx88", "mx84"):
        nbits = 8 if kind == "mx88" else 4
        w, s = _mx_weights(N, K, nbits, 32, g)
        return H.A8Wn_MXFP_dynamic(device=device, dtype=tdt, post_scale=r.get("post", False), W_nbits=nbits).from_weights(
            w.to(device), scales=s.to(device))
    if kind == "mx44":
        w, s = _mx_weights(N, K, 4, 32, g)
        return H.A4W4_MXFP_dynamic(device=device, dtype=tdt).from_weights(w.to(device), scales=s.to(device))
    if kind == "nv":
        w, s = _mx_weights(N, K, 4, 16, g)
        return H.A4W4_NVFP_dynamic(device=device, dtype=tdt).from_weights(w.to(device), scales=s.to(device))
    raise ValueError(kind)


def x_format(lin, fused):
    """(torch dtype of x as passed, elements per row of x, ABI input_dtype) of a call of this layer"""
    code = lin.input_dtype
    K = lin.in_features
    x16 = torch.bfloat16 if lin.output_dtype in (DType.BF16, DType.MXBF16) else torch.float16
    if fused or code in (DType.FP16, DType.BF16, DType.MXFP16, DType.MXBF16):
        t = x16 if fused else gemlite_amd.dtypes.DTYPE_TO_TORCH[code.value]
        if code in (DType.MXFP16, DType.MXBF16):
            t = torch.float16 if code == DType.MXFP16 else torch.bfloat16
        return t, K, (gemlite_amd.dtypes.TORCH_TO_DTYPE[t].value if fused else code.value)
    if code in (DType.MXFP4, DType.NVFP4):
        return torch.uint8, K // 2, code.value
    if code == DType.MXFP8:
        return torch.float8_e4m3fn, K, code.value
    return gemlite_amd.dtypes.DTYPE_TO_TORCH[code.value], K, code.value


def scales_x_kind(lin):
    """None (no activation scales) | 'token' (fp32 per row) | 'block' (uint8 [M_pad, K / group])"""
    c = lin.channel_scale_mode
    if c in (2, 3):
        return "token"
    if c == 4:
        return "block"
    return None


def plan_args(lin, M, tuning=(0, 0, 0, 0), fused=False, x=0x1000, out=0x1000, stride_xm=None, stride_om=None, tensors=None):
    """gemlite_hip_forward_args of one call, with placeholder pointers where none are given (planning never dereferences them).
    tensors: (W_q, scales, zeros) views to use instead of the layer's own."""
    W_q, scales, zeros = tensors if tensors is not None else (lin.W_q, lin.scales, lin.zeros)
    a = _static_args(W_q, scales, zeros, lin.get_meta_args())
    _, xrow, in_code = x_format(lin, fused)
    a.matmul_type, a.M = -1, M
    a.x, a.out = x, out
    a.input_dtype = in_code
    a.stride_xm, a.stride_xk = (xrow if stride_xm is None else stride_xm), 1
    a.stride_om, a.stride_on = (a.N if stride_om is None else stride_om), 1
    sk = scales_x_kind(lin)
    if sk and not fused:
        a.scales_x = 0x1000
        a.stride_sx_m = lin.in_features // lin.group_size if sk == "block" else 1
    for i in range(4):
        a.tuning[i] = tuning[i]
    return a


def kernel_name(a):
    return _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode()


def _c(kind, N, K, M, name, tuning=(0, 0, 0, 0), fused=False, **kw):
    return dict(recipe=dict(kind=kind, N=N, K=K, **kw), M=M, tuning=tuning, fused=fused, name=name)


BF = torch.bfloat16
# One launch site per entry.  M sits at the partial edges of each family's tile (tile - 1, tile + 1) or its upper bound; N is not a
# multiple of the tile width where the family takes that.
CASES = [
    # packed words under 16-bit activations, one row
    _c("wn", 512, 512, 1, "gemv_w4_decode3_kernel<tile16,16w>", nbits=4, gs=128, tdt=BF),
    _c("wn", 1024, 1536, 1, "gemv_w4_decode_kernel<tile16,16w>", (0, 0, 0, 4096), nbits=4, gs=128, tdt=BF),
    _c("wn", 1024, 2048, 1, "gemv_wn_kernel<tile64>", nbits=1, gs=32),
    _c("wn", 3072, 128, 1, "gemv_w2_mfma_kernel<tile16>", nbits=2, gs=128),
    # 2 .. 4 rows on the matrix-core GEMV
    _c("wn", 1024, 512, 3, "gemv_mfma_kernel<tile16,rows4>", nbits=4, gs=128),
    _c("wn", 1024, 512, 2, "gemv_mfma_kernel<tile16,rows4>", nbits=4, gs=128),
    _c("wn", 4096, 4096, 4, "gemv_mfma_kernel<tile16,rows4>", nbits=4, gs=128),
    # registers-only few-row kernel, streaming kernel, decode-shaped rows kernels
    _c("wn", 4096, 4096, 7, "gemm_wn_direct_kernel<tile32,8w>", nbits=4, gs=128),
    _c("wn", 1024, 512, 17, "gemm_wn_stream_kernel", (0, 0, 1, 0), nbits=4, gs=128),
    _c("wn", 1008, 512, 17, "gemm_w4_rows_kernel<32x16>", nbits=4, gs=32, tdt=BF),
    _c("wn", 4096, 4096, 64, "gemm_w4_rows_kernel<64x16>", nbits=4, gs=128),
    _c("wn", 1008, 512, 33, "gemm_w2_rows_kernel<16x16>", nbits=2, gs=32),
    # the 8-wave MFMA tiles: 32-row tiles, 64 x 64 narrow tiles, 128 x 128 / wide tiles, round-1 tiled kernel, groups of 32
    _c("wn", 1024, 512, 31, "gemm_w4_mma_kernel<32x128>", (3, 0, 0, 0), nbits=4, gs=64),
    _c("wn", 4096, 4096, 255, "gemm_w4_mma_kernel<64x64>", nbits=4, gs=128),
    _c("wn", 4096, 4096, 129, "gemm_w4_mma_kernel<128x128>", (0, 2, 4, 128), nbits=4, gs=128),   # K slices: slabs + ticket
    _c("wn", 4096, 4096, 255, "gemm_w2_mma_kernel<128x128>", (0, 4, 4, 0), nbits=2, gs=128),     # K slices: reduce-scatter
    _c("wn", 1024, 1024, 65, "gemm_w1_mma_kernel<128x128>", nbits=1, gs=64),
    _c("wn", 1024, 512, 33, "gemm_w8_mma_kernel<64x128>", nbits=8, gs=128),
    _c("wn", 1024, 192, 33, "gemm_w4_tiled_kernel<128x128>", nbits=4, gs=64, tdt=BF),
    _c("wn", 4096, 4096, 300, "gemm_w4_mma_kernel<32x128,g32>", nbits=4, gs=32),
    _c("bitnet16", 1024, 1024, 1, "gemv_wn_kernel<tile32>"),
    # coverage kernel (group size 32 and a K the tiles cannot divide)
    _c("wn", 1000, 64, 2, "generic_matmul_kernel", nbits=4, gs=32, tdt=BF),
    # unpacked 8-bit weights under 16-bit activations
    _c("a16w8i", 1024, 1024, 1, "a16w8_decode_kernel<tile16,16w>", (0, 0, 0, 16384)),
    _c("a16w8i", 1008, 512, 3, "a16w8_rows_kernel<16x16>"),
    _c("a16w8f", 1008, 512, 17, "a16w8_rows_lds_kernel<32x16>", tdt=BF),
    _c("a16w8i", 1024, 512, 65, "gemm_a16w8_kernel<128x128>"),
    _c("a16w8f", 2048, 256, 33, "kmajor_w8a16_kernel", (7, 0, 0, 1024), tdt=BF),
    # unpacked 8-bit weights under 8-bit activations
    _c("a8w8f", 1024, 4096, 1, "a8w8_decode_kernel<tile16,16w>", tdt=BF),
    _c("a8w8f", 1008, 512, 33, "a8w8_rows_kernel<64x16>", (0, 0, 0, 524288), tdt=BF),
    _c("a8w8i", 1024, 512, 17, "a8w8_rows_lds_kernel<32x16>"),
    _c("a8w8f", 1024, 512, 129, "gemm_a8w8_kernel<64x64>", (2, 0, 0, 0), tdt=BF),
    _c("a8w8i", 1024, 1280, 65, "gemm_a8w8_lds_kernel<128x128>", (0, 3, 4, 0)),
    _c("a8w8i", 1024, 512, 17, "gemm_a8w8_mma_kernel<32x128>", (0, 2, 0, 128)),
    _c("a8w8f", 1024, 512, 65, "gemm_a8w8_sq_kernel<64x64>", tdt=BF),
    _c("a8w8f", 1000, 64, 1, "kmajor_matmul_kernel", tdt=BF),
    # 8-bit activations x packed words (A8Wn dynamic, BitNet int8)
    _c("a8w4", 1024, 256, 1, "gemv_a8w4_kernel<tile16,16w>", gs=128, tdt=BF),
    _c("bitnet8", 1280, 256, 1, "gemv_a8w2_kernel<tile16,16w>"),
    _c("a8w4", 1024, 512, 17, "a8w4_rows_kernel<32x16>", gs=64, tdt=BF),
    _c("bitnet8", 1024, 512, 64, "a8w2_rows_kernel<64x16>"),
    _c("a8w4", 1024, 512, 65, "gemm_a8w4_mma_kernel<64x128>", gs=128, tdt=BF),
    _c("a8w2", 1024, 512, 129, "gemm_a8w2_mma_kernel<256x128>", gs=128),
    # block-scaled formats
    _c("mx16w4", 1024, 512, 17, "a16w4_mxfp_rows_kernel<32x16>"),
    _c("mx16w8", 1024, 512, 33, "a16w8_mxfp_rows_kernel<64x16>", tdt=BF),
    _c("mx16w4", 1024, 512, 257, "gemm_a16w4_mxfp_kernel<128x128>"),
    _c("mx16w8", 1024, 512, 129, "gemm_a16w8_mxfp_kernel<128x128>", tdt=BF),
    _c("mx44", 1024, 512, 3, "mx_gemv_w4_kernel", (5, 0, 0, 0)),
    _c("mx88", 1024, 512, 2, "mx_gemv_w8_kernel", (5, 0, 0, 0), post=True),
    _c("mx44", 1024, 512, 17, "mx_rows_a4w4_kernel<32x16>"),
    _c("mx84", 1024, 512, 15, "mx_rows_a8w4_kernel<16x16>", post=True),
    _c("mx88", 1024, 512, 33, "mx_rows_a8w8_kernel<64x16>", post=True),
    _c("nv", 1024, 512, 31, "nvfp4_rows_kernel<32x16>"),
    _c("mx44", 1024, 512, 17, "gemm_mx_a4w4_kernel<32x128>", (0, 0, 3, 16)),
    _c("mx84", 1024, 2048, 23, "gemm_mx_a8w4_kernel<32x128>", (0, 6, 0, 0), post=True),
    _c("mx88", 1024, 512, 47, "gemm_mx_a8w8_kernel<128x128>", (0, 0, 4, 0)),
    _c("mx44", 1024, 512, 129, "gemm_mx_a4w4_sq_kernel<64x64>"),
    _c("mx84", 1024, 1024, 65, "gemm_mx_a8w4_sq_kernel<64x64>", post=True),
    _c("mx88", 1024, 512, 127, "gemm_mx_a8w8_sq_kernel<64x64>", post=True),
    _c("mx44", 1024, 512, 3, "gemm_mx_a4w4_tile_kernel<256x256>", (3, 0, 0, 0)),
    _c("mx84", 1024, 512, 33, "gemm_mx_a8w4_tile_kernel<256x256>", (3, 0, 0, 0), post=True),
    _c("mx88", 1024, 512, 40, "gemm_mx_a8w8_tile_kernel<256x256>", (3, 0, 0, 0), post=True),
    _c("nv", 1024, 1280, 65, "gemm_nvfp4_f16_kernel<128x128>"),
    _c("mx84", 1024, 512, 5, "mx_generic_kernel", (1, 0, 0, 0)),
    # 16-bit activations quantised inside the launch (scales_x = NULL)
    _c("a8w8f", 1024, 4096, 1, "a8w8_decode_fused_quant_kernel<tile16,16w>", fused=True, tdt=BF),
    _c("a8w4", 1024, 256, 1, "gemv_a8w4_fused_quant_kernel<tile16,16w>", fused=True, gs=128, tdt=BF),
    _c("bitnet8", 1280, 256, 1, "gemv_a8w2_fused_quant_kernel<tile16,16w>", fused=True),
    _c("a8w8f", 1000, 64, 1, "kmajor_fused_quant_kernel", fused=True, tdt=BF),
    # ... 2 .. 64 rows: producer blocks of the launch quantise the rows into the workspace (flags + M K bytes + M scales)
    _c("a8w8i", 1024, 512, 17, "a8w8_rows_fq_kernel<32x16>", fused=True),
    _c("a8w8f", 1008, 512, 64, "a8w8_rows_fq_kernel<64x16>", fused=True, tdt=BF),
    _c("mx88", 1024, 512, 1, "mx_rows_a8w8_fused_quant_kernel<16x16>", fused=True),
    _c("mx84", 1024, 512, 1, "mx_rows_a8w4_fused_quant_kernel<16x16>", fused=True),
    _c("mx44", 1024, 512, 1, "mx_rows_a4w4_fused_quant_kernel<16x16>", fused=True),
    _c("nv", 1024, 512, 1, "nvfp4_rows_fused_quant_kernel<16x16>", fused=True),
]


def case_id(c):
    r = c["recipe"]
    extra = "".join(f"-{k}{v}" for k, v in r.items() if k not in ("kind", "N", "K", "tdt"))
    return f"{c['name']}-{r['kind']}{extra}-{r['N']}x{r['K']}-M{c['M']}" + ("-fused" if c["fused"] else "")


_LAYERS = {}


def cpu_layer(r):
    key = tuple(sorted((k, str(v)) for k, v in r.items()))
    if key not in _LAYERS:
        _LAYERS[key] = build_layer(r, "cpu")
    return _LAYERS[key]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_case_plans_the_kernel_it_names(case):
    lin = cpu_layer(case["recipe"])
    a = plan_args(lin, case["M"], case["tuning"], case["fused"])
    assert _hip.load().gemlite_hip_query(C.byref(a)) == 0
    assert kernel_name(a) == case["name"]


def test_every_kernel_the_planner_fuzz_reaches_has_a_case():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import fuzz_planner
    cnt, _ = fuzz_planner.run(0, 20000)
    reached = {k for k in cnt if not k.startswith("status")}
    covered = {c["name"].split("<")[0] for c in CASES}
    assert len(reached) >= 55
    assert reached <= covered, sorted(reached - covered)


def test_every_kernel_name_the_library_can_report_has_a_case():
    """The fuzz never sends scales_x = NULL, so it cannot reach the fused-quantisation kernels: every kernel name literal in the library's
    sources (what gemlite_hip_kernel_name can return; comments left out) must have a case too."""
    csrc = os.path.join(ROOT, "gemlite_amd", "csrc")
    names = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".inc", ".h")):
            src = re.sub(r"//[^\n]*|/\*.*?\*/", "", open(os.path.join(csrc, f)).read(), flags=re.S)
            names |= set(re.findall(r'"([a-z][a-z0-9_]*_kernel)[<"]', src))
    covered = {c["name"].split("<")[0] for c in CASES}
    assert len(names) >= 60
    assert names <= covered, sorted(names - covered)


@pytest.mark.parametrize("M", [48, 64])
@pytest.mark.parametrize("how", ["out4", "stride_om"])
def test_group32_layers_keep_the_rows_kernel_when_the_tiles_decline(M, how):
    """A16W4 g32 at M = 48 / 64: the 32-row tiles take an aligned request; where their planner declines the output (4 bytes off, or
    a row stride that is not a multiple of 4 outputs) the rows kernel takes it — not the streaming kernel, 5 - 7x behind it."""
    lin = cpu_layer(dict(kind="wn", N=4096, K=4096, nbits=4, gs=32))
    assert kernel_name(plan_args(lin, M)) == "gemm_w4_mma_kernel<32x128,g32>"
    a = plan_args(lin, M, out=0x1004) if how == "out4" else plan_args(lin, M, stride_om=4096 + 2)
    assert kernel_name(a).startswith("gemm_w4_rows_kernel<")


def test_lds_dma_word_path_keeps_its_kernel_name_when_w_q_is_misaligned():
    """The 64 x 64 / 128 x 128 4-bit tiles take their packed words by 16-byte LDS-DMA only from a 16-byte aligned w_q and row stride;
    otherwise the register loads of the same kernel.  The kernel name cannot tell the two forms apart, so this only checks that the
    gate keeps the kernel; test_abi_bounds_gpu.py::test_lds_dma_word_tiles_with_a_misaligned_w_q checks the result.  (The 32 x 128 tiles
    have no LDS-DMA weight form: WL exists only for the narrow variant 0 and for MI = 4.)"""
    lin = cpu_layer(dict(kind="wn", N=4096, K=4096, nbits=4, gs=128))
    for M in (256, 129):
        a = plan_args(lin, M)
        name = kernel_name(a)
        a.w_q += 4
        assert kernel_name(a) == name
        a = plan_args(lin, M)
        a.stride_wk = 4096 + 1
        assert kernel_name(a) == name


def test_fused_quant_request_the_kernels_cannot_take_is_answered_no_fused_quant():
    """A one-row fused-quantisation request whose x or w_q is not 16-byte aligned has no kernel: the header's answer is
    GEMLITE_ERR_NO_FUSED_QUANT (quantise x and call again), not an unsupported layer."""
    lin = cpu_layer(dict(kind="a8w8f", N=1000, K=64, tdt=torch.bfloat16))
    a = plan_args(lin, 1, fused=True)
    assert _hip.load().gemlite_hip_query(C.byref(a)) == 0
    a.x += 2
    assert _hip.load().gemlite_hip_query(C.byref(a)) == _hip.ERR_NO_FUSED_QUANT


def test_matrix_core_gemv_keeps_strided_rows():
    """gemv_mfma_kernel reads x chunks past a row's end (the next row, or what lies between strided rows) for units past a wave's end and
    leaves them out by a select; strided rows stay on it, so the GPU module's aligned layout runs it with NaN between the rows."""
    lin = cpu_layer(dict(kind="wn", N=1024, K=512, nbits=4, gs=128))
    for M in (2, 3):
        assert kernel_name(plan_args(lin, M, stride_xm=512 + 64)).startswith("gemv_mfma_kernel<")
