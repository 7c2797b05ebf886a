"""Structured-input exactness per kernel family (`pytest -m gpu`).

Random-data parity absorbs an indexing slip that touches few outputs or that permutes values of similar size (that is how the
`a8w8_rows` miscompile of round 2 slipped past the mean gates at first).  Here every number is exactly representable at every step
of every kernel, so the only acceptable result is the exact one:

  * x rows are one-hot (1.0 at a single k, a different k per row; passes shift the hot positions until every k was hit once),
  * weight codes are position-coded, W[n][k] = f(k, n) mod 2^bits, zero points are integer codes and scales are powers of two
    ({0.5, 1, 2} by group and column), so (W - z) * s is a small integer times a power of two in fp16, bf16, e4m3 and fp32 alike,
  * 8-bit x 8-bit families use position-coded int8 / e4m3 bytes and power-of-two channel scales; the MX families use the layer's
    own element bytes and e8m0 block scales (powers of two by construction) through the float64 oracle.

Stacking the passes gives the whole dequantised matrix [K, N]; it must equal the expected one bit for bit.  A wrong k, a wrong
column, a dropped or doubled K step, a row mix-up inside an MFMA fragment, a split-K slice combined twice: each shows up as a
wrong integer.  The second half checks that the reduce-scatter split-K combine of the 8-wave MFMA kernel returns the same bits as
the slab + ticket combine."""
import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear, _hip, helper as H
from gemlite_amd.core import _hip_matmul, _static_args
from gemlite_amd.quant_utils import scale_activations_mxfp4, scale_activations_mxfp8

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


def _name(lin, M, mt, tuning, scaled=False, k_stride=None):
    a = _static_args(lin.W_q, lin.scales, lin.zeros, lin.get_meta_args())
    a.matmul_type, a.M = mt, M
    a.x = a.out = 0x1000
    K = lin.in_features
    a.stride_xm, a.stride_xk, a.stride_om, a.stride_on = (k_stride or K), 1, a.N, 1
    if scaled:
        a.scales_x = 0x1000
        a.stride_sx_m = max(1, K // lin.group_size)
    a.input_dtype = lin.input_dtype.value
    for i in range(4):
        a.tuning[i] = tuning[i]
    return _hip.load().gemlite_hip_kernel_name(_hip.C.byref(a)).decode()


def _coded_wn(N, K, nbits, gs, tdt, fma):
    """position-coded packed layer and its exact dequantised matrix [K, N] (float32)"""
    k = torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    mask = (1 << nbits) - 1
    W = ((k * 5 + n * 3 + (k >> 4) + (n >> 3)) & mask).to(torch.uint8)             # [N, K]
    g = torch.arange(K // gs).view(1, -1)
    z = ((g * 3 + n) & mask).float()                                               # [N, K/gs]
    s = torch.pow(2.0, ((g + n) % 3 - 1).float())                                  # 0.5, 1, 2
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(nbits, gs, K, N, code, code)
    lin.pack(W.to(DEV), s.reshape(-1, 1).to(tdt).to(DEV), z.reshape(-1, 1).to(tdt).to(DEV), None, fma_mode=fma)
    E = (W.float() - z.repeat_interleave(gs, dim=1)) * s.repeat_interleave(gs, dim=1)  # [N, K]
    return lin, E.t().contiguous()


_EYE = {}


def _eye(K, M, dt):
    """[K + M, K] on the device: identity followed by M zero rows (the ragged last pass reads into them)"""
    key = (K, M, dt)
    if key not in _EYE:
        _EYE.clear()
        I = torch.zeros(K + M, K, device=DEV)
        I[torch.arange(K), torch.arange(K)] = 1.0
        _EYE[key] = I.to(dt)
    return _EYE[key]


def _sweep(call, M, K, dt):
    """every k hot exactly once: pass p feeds rows [p M, p M + M) of the identity; returns the stacked outputs [K, N] (float32, on
    the device).  Nothing is copied or synchronised per pass — with several test processes on one GPU every sync costs a time slice."""
    I = _eye(K, M, dt)
    rows = []
    for p in range((K + M - 1) // M):
        y = call(I[p * M:(p + 1) * M])
        n = min(M, K - p * M)
        rows.append(y[:n])
        if n < M:
            rows.append(None)
            tail = y[n:]
    Y = torch.cat([r for r in rows if r is not None], 0).float()
    if rows and rows[-1] is None:
        assert torch.count_nonzero(tail) == 0, "rows of an all-zero input must be zero"
    return Y


def _exact(tag, Y, E):
    bad = (Y != E.to(Y.device))
    if bad.any():
        bad, Y = bad.cpu(), Y.cpu()
        idx = bad.nonzero()
        k, n = [int(v) for v in idx[0]]
        raise AssertionError(f"{tag}: {int(bad.sum())} wrong outputs of {E.numel()}; first at k={k} n={n}: got {float(Y[k, n])}, "
                             f"exact {float(E[k, n])}; wrong k rows {sorted(set(idx[:, 0].tolist()))[:12]}, "
                             f"wrong columns {sorted(set(idx[:, 1].tolist()))[:12]}")


# families of the packed-weight x 16-bit-activation path: (label, matmul_type, M, tuning, expected name prefix)
WN_FAMILIES = [
    ("gemv", -1, 1, (0, 0, 0, 512), "gemv_w"),
    ("gemv_default", -1, 1, (0, 0, 0, 0), ""),
    ("gemv_mfma16", -1, 1, (21, 0, 0, 1024), "gemv_"),
    ("gemv_mfma32", -1, 1, (22, 0, 0, 1024), "gemv_"),
    ("gemv_mfma64", -1, 1, (24, 0, 0, 1024), "gemv_"),
    ("gemv_mfma_rows3", -1, 3, (0, 0, 0, 1024), "gemv_"),
    ("gemv_mfma_rows4", -1, 4, (22, 0, 0, 1024), "gemv_"),
    ("direct16", 3, 13, (1, 0, 0, 0), "gemm_wn_direct_kernel"),
    ("direct32", 3, 16, (2, 0, 0, 0), "gemm_wn_direct_kernel"),
    ("direct64_sk2", 3, 32, (4, 2, 0, 0), "gemm_wn_direct_kernel"),
    ("direct32_8w", 3, 16, (2, 1, 8, 0), "gemm_wn_direct_kernel<tile32,8w>"),
    ("direct64_8w_sk2", 3, 13, (4, 2, 8, 0), "gemm_wn_direct_kernel<tile64,8w>"),
    ("stream", 3, 8, (0, 0, 1, 0), "gemm_wn_stream_kernel"),
    # round 5: the decode-shaped rows kernel (gemm_wn_rows.hip): every row-tile count, 8 waves, 64-row blocks along grid.y
    ("rows5_m13", 3, 13, (9, 0, 0, 0), "gemm_w4_rows_kernel<16x16>"),
    ("rows5_m32", 3, 32, (9, 0, 0, 0), "gemm_w4_rows_kernel<32x16>"),
    ("rows5_m32_auto", -1, 32, (9, 0, 0, 0), "gemm_w4_rows_kernel<32x16>"),
    ("rows5_m40", 3, 40, (9, 0, 0, 0), "gemm_w4_rows_kernel<48x16>"),
    ("rows5_m64", -1, 64, (9, 0, 0, 0), "gemm_w4_rows_kernel<64x16>"),
    ("rows5_m150_gridy", -1, 150, (9, 0, 0, 0), "gemm_w4_rows_kernel<64x16>"),
    ("mma32", 4, 29, (0, 1, 1, 0), "gemm_w{b}_mma_kernel<32x128>"),
    ("mma64_sk3", 4, 64, (0, 3, 2, 0), "gemm_w{b}_mma_kernel<64x128>"),
    ("mma64_xch2", 4, 64, (0, 2, 2, 2048), "gemm_w{b}_mma_kernel<64x128>"),
    ("mma128_xch4", 4, 128, (0, 4, 4, 0), "gemm_w{b}_mma_kernel<128x128>"),
    ("mma128_ticket4", 4, 128, (0, 4, 4, 128), "gemm_w{b}_mma_kernel<128x128>"),
    ("mma256", 4, 256, (0, 1, 8, 0), "gemm_w{b}_mma_kernel<256x128>"),
    ("mma256_xch2", 4, 256, (0, 2, 8, 2048), "gemm_w{b}_mma_kernel<256x128>"),
    ("mma_wide128_sk2", 4, 128, (0, 2, 20, 0), "gemm_w{b}_mma_kernel<128x256>"),
    ("mma_wide256", 4, 256, (0, 1, 24, 0), "gemm_w{b}_mma_kernel<256x256>"),
    ("auto_m2", -1, 2, (0, 0, 0, 0), ""),
    ("auto_m24", -1, 24, (0, 0, 0, 0), ""),
    ("auto_m100", -1, 100, (0, 0, 0, 0), ""),
    ("auto_m256", -1, 256, (0, 0, 0, 0), ""),
]


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("K", [1280, 2048])
@pytest.mark.parametrize("nbits,fma", [(4, True), (4, False), (2, True), (1, True), (8, True)])
def test_packed_weight_families_one_hot_times_position_coded_is_exact(nbits, fma, K, tdt):
    # K = 1280: 10 groups, 20 / 10 / 5 K steps (uneven split-K slices); K = 2048: the few-row kernels (direct MFMA, streaming) apply.
    # N / 16 = 64 blocks for the decode kernels
    N, gs = 1024, 128
    lin, E = _coded_wn(N, K, nbits, gs, tdt, fma)
    assert E.abs().max() <= 2 * 255 and torch.equal(E.to(tdt).float(), E)  # representable: the test is about indexing only
    ran = {}
    for label, mt, M, tuning, prefix in WN_FAMILIES:
        try:
            name = _name(lin, M, mt, tuning)
        except Exception:
            name = ""
        if not name or "unsupported" in name:
            continue  # this bit width has no such variant (e.g. 1- / 8-bit wide tiles)
        if prefix and not name.startswith(prefix.format(b=nbits)):
            continue  # the forced variant does not exist for this width and the planner chose another family: covered elsewhere
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), mt, tuning), M, K, tdt)
        _exact(f"{label} [{name}] w{nbits} {'fma' if fma else 'sub'} {tdt}", Y, E)
        ran[label] = name
    # the families this width must have
    must = {"gemv_default" if nbits == 8 else "gemv", "auto_m2", "auto_m24", "auto_m100", "auto_m256", "mma32", "mma256"}
    if nbits in (4, 2):
        must |= {"gemv_mfma16", "gemv_mfma32", "mma64_xch2", "mma128_xch4", "mma_wide256"}
        if K == 2048:
            must |= {"direct16", "direct32", "direct64_sk2", "direct32_8w", "direct64_8w_sk2", "stream"}
    if nbits == 4:
        must |= {"rows5_m13", "rows5_m32", "rows5_m32_auto", "rows5_m40", "rows5_m64", "rows5_m150_gridy"}
    assert must <= set(ran), (sorted(must - set(ran)), ran)


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
def test_packed_weight_long_k_many_ring_passes_is_exact(tdt):
    """K = 8192 + 128 (65 groups): many passes over the LDS ring / chunk loops, uneven last chunks — decode and tile kernels"""
    N, K, gs = 512, 8320, 128
    lin, E = _coded_wn(N, K, 4, gs, tdt, True)
    meta = lin.get_meta_args()
    for label, mt, M, tuning in (("auto_m1", -1, 1, (0, 0, 0, 0)), ("gemv", -1, 1, (0, 0, 0, 512)), ("mfma", -1, 1, (0, 0, 0, 1024)),
                                 ("auto_m4", -1, 4, (0, 0, 0, 0)), ("auto_m32", -1, 32, (0, 0, 0, 0)),
                                 ("mma256_sk4", 4, 256, (0, 4, 8, 0)), ("mma256_sk5", 4, 256, (0, 5, 8, 0))):
        if M == 1:   # every 8th k plus the tail (1170 launches)
            ks = sorted(set(range(0, K, 8)) | set(range(K - 130, K)))
            I = _eye(K, 1, tdt)
            rows = [_hip_matmul(I[k:k + 1], lin.W_q, lin.scales, lin.zeros, None, meta, mt, tuning) for k in ks]
            _exact(f"long-k {label} {tdt}", torch.cat(rows, 0).float(), E[ks])
        else:
            Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), mt, tuning), M, K, tdt)
            _exact(f"long-k {label} {tdt}", Y, E)


# ------------------------------------------------------------------------------------------------ 8-bit x 8-bit
def _coded_a8w8(N, K, kind, tdt):
    k = torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    if kind == "int8":
        Wq = (((k * 3 + n * 5 + (k >> 6)) % 255) - 127).to(torch.int8)
        vals = Wq.float()
        proc = H.A8W8_int8_dynamic(device=DEV, dtype=tdt)
    else:
        b = ((k * 3 + n * 5 + (k >> 6)) % 256).to(torch.uint8)
        b[(b & 0x7F) == 0x7F] = 0x3A   # the two NaN bytes of e4m3fn
        Wq = b.view(torch.float8_e4m3fn)
        vals = Wq.float()
        proc = H.A8W8_dynamic(device=DEV, dtype=tdt, fp8=torch.float8_e4m3fn)
    s = torch.pow(2.0, ((n % 4) - 2).float())    # [N, 1]: 0.25 .. 2
    lin = proc.from_weights(Wq.to(DEV), scales=s.to(tdt).to(DEV))
    return lin, (vals * s).t().contiguous()


A8_FAMILIES = [("streaming", 1, (1, 0, 0, 0)), ("rows_m1", 1, (4, 0, 0, 524288)), ("rows", 2, (0, 0, 0, 524288)), ("rows", 16, (0, 0, 0, 524288)),
               ("rows32", 17, (0, 0, 0, 524288)), ("rows32", 32, (0, 0, 0, 524288)), ("rows64", 33, (0, 0, 0, 524288)), ("rows64", 64, (4, 0, 0, 524288)),
               # round 6: x through LDS (gemm_w8_rows.hip) — the default from 2 rows; tuning[3] & 524288 = the round-3 kernel above
               ("rows_lds16", 1, (4, 0, 0, 0)), ("rows_lds16", 9, (0, 0, 0, 0)), ("rows_lds32", 17, (0, 0, 0, 0)), ("rows_lds32", 32, (0, 0, 0, 0)), ("rows_lds48", 40, (0, 0, 0, 0)),
               ("rows_lds64", 64, (4, 0, 0, 0)),
               ("mfma_r1", 64, (2, 0, 0, 0)), ("mma32", 29, (0, 1, 1, 0)), ("mma64_sk3", 64, (0, 3, 2, 0)),
               ("mma128", 128, (0, 1, 4, 0)), ("mma128_direct_b", 128, (0, 2, 4, 64)), ("mma256_sk5", 256, (0, 5, 8, 0)),
               ("auto_m1", 1, (0, 0, 0, 0)), ("auto_m100", 100, (0, 0, 0, 0)), ("auto_m256", 256, (0, 0, 0, 0)),
               # the unsplit tiles, forced: four ragged row tiles of 64 / two of 128 (tests/test_k_order_gpu.py walks their K orders)
               ("sq64_m200", 200, (5, 0, 0, 0)), ("sq128_m200", 200, (10, 0, 0, 0))]


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("kind", ["int8", "fp8"])
def test_a8w8_families_one_hot_times_position_coded_is_exact(kind, tdt):
    N, K = 512, 1280  # 20 chunks of 64 k, 10 / 5 LDS steps; slices of 3 and 5 are uneven
    lin, E = _coded_a8w8(N, K, kind, tdt)
    if tdt == torch.bfloat16 and kind == "int8":
        E = E.to(tdt).float()  # 127 needs 7 bits: fine; kept for symmetry (the product is one term, the rounding is the output's)
    qdt = torch.int8 if kind == "int8" else torch.float8_e4m3fn
    ran = []
    for label, M, tuning in A8_FAMILIES:
        name = _name(lin, M, -1, tuning, scaled=True)
        if "unsupported" in name:
            continue
        sx = torch.ones(M, 1, dtype=torch.float32, device=DEV)
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, tuning), M, K, qdt)
        _exact(f"a8w8 {kind} {label} [{name}] {tdt}", Y, E)
        ran.append(name)
    assert {"a8w8_rows_kernel<16x16>", "a8w8_rows_kernel<32x16>", "a8w8_rows_kernel<64x16>"} <= set(ran), ran
    assert {"a8w8_rows_lds_kernel<16x16>", "a8w8_rows_lds_kernel<32x16>", "a8w8_rows_lds_kernel<48x16>", "a8w8_rows_lds_kernel<64x16>"} <= set(ran), ran
    assert any("gemm_a8w8_lds" in r for r in ran) and any("mma" in r for r in ran), ran
    assert {"gemm_a8w8_sq_kernel<64x64>", "gemm_a8w8_sq_kernel<128x128>"} <= set(ran), ran


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("kind", ["int8", "fp8"])
def test_a16w8_rows_families_one_hot_times_position_coded_is_exact(kind, tdt):
    """8-bit weight-only layers (round 6): one-hot 16-bit activations x position-coded int8 / e4m3 weights with power-of-two channel scales —
    every output is ONE weight times one scale, exactly; a wrong k -> slot map of the permuted A fragments of w8_rows_lds_kernel (or a wrong
    swizzle of a piece geometry) shows as a wrong row."""
    N, K = 256, 1280
    k = torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    s = torch.pow(2.0, ((n % 4) - 2).float())
    if kind == "int8":
        Wq = (((k * 3 + n * 5 + (k >> 6)) % 255) - 127).to(torch.int8)
        lin = H.A16W8(device=DEV, dtype=tdt).from_weights(Wq.to(DEV), scales=s.to(tdt).to(DEV))
    else:
        b = ((k * 3 + n * 5 + (k >> 6)) % 256).to(torch.uint8)
        b[(b & 0x7F) == 0x7F] = 0x3A
        Wq = b.view(torch.float8_e4m3fn)
        lin = H.A16W8_FP8(device=DEV, dtype=tdt).from_weights(Wq.to(DEV), scales=s.to(tdt).to(DEV))
    E = (Wq.float() * s).t().contiguous()
    if tdt == torch.bfloat16:
        E = E.to(tdt).float()  # (the output's own rounding: |w| <= 127 * 2 fits 8 bits, e4m3 has 4)
    ran = []
    for M, tuning in ((2, (4, 0, 0, 1048576)), (5, (0, 0, 0, 0)), (16, (0, 0, 0, 524288)), (17, (0, 0, 0, 0)), (32, (0, 0, 0, 0)), (40, (0, 0, 0, 0)), (64, (4, 0, 0, 0)), (100, (4, 0, 0, 0)),
                      (17, (0, 0, 0, 524288)), (64, (4, 0, 0, 524288))):
        name = _name(lin, M, -1, tuning)
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, tuning), M, K, tdt)
        _exact(f"a16w8 {kind} M={M} [{name}] {tdt}", Y, E)
        ran.append(name)
    assert {"a16w8_rows_lds_kernel<16x16>", "a16w8_rows_lds_kernel<32x16>", "a16w8_rows_lds_kernel<48x16>", "a16w8_rows_lds_kernel<64x16>",
            "a16w8_rows_kernel<16x16>", "a16w8_rows_kernel<32x16>", "a16w8_rows_kernel<64x16>"} <= set(ran), ran


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("nbits", [4, 2])
def test_a8wn_fp8_activation_families_one_hot_is_exact(nbits, tdt):
    """fp8 activations x packed weights (A8Wn dynamic): dequantised weights are rounded to e4m3 before the MFMA — integers up to
    15 times a power of two survive that rounding"""
    N, K, gs = 1024, 1280, 128
    k = torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    mask = (1 << nbits) - 1
    W = ((k * 5 + n * 3 + (k >> 4)) & mask).to(torch.uint8)
    g = torch.arange(K // gs).view(1, -1)
    z = ((g * 3 + n) & mask).float()
    s = torch.pow(2.0, ((g + n) % 3 - 1).float())
    lin = H.A8Wn_HQQ_INT_dynamic(device=DEV, dtype=tdt, post_scale=False, W_nbits=nbits).from_weights(
        W, s.reshape(-1, 1).to(tdt), z.reshape(-1, 1).to(tdt))
    E = ((W.float() - z.repeat_interleave(gs, 1)) * s.repeat_interleave(gs, 1)).t().contiguous()
    for label, M, tuning in (("gemv", 1, (0, 0, 0, 0)), ("gemv_m3", 3, (0, 0, 0, 0)), ("mma32", 29, (0, 1, 1, 0)),
                             ("mma64_sk3", 64, (0, 3, 2, 0)), ("mma256", 256, (0, 2, 8, 0)), ("auto_m100", 100, (0, 0, 0, 0))):
        sx = torch.ones(M, 1, dtype=torch.float32, device=DEV)
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, tuning), M, K,
                   torch.float8_e4m3fn)
        _exact(f"a8w{nbits} {label} {tdt}", Y, E)


# ------------------------------------------------------------------------------------------------ block-scaled (MX) families
@pytest.mark.parametrize("proc_name,M,tuning", [
    ("A8W8_MXFP_dynamic", 1, (0, 0, 0, 0)), ("A8W8_MXFP_dynamic", 64, (0, 0, 0, 0)), ("A8W8_MXFP_dynamic", 128, (0, 3, 4, 0)),
    ("A8W8_MXFP_dynamic", 128, (3, 0, 0, 0)),
    ("A8W4_MXFP_dynamic", 1, (0, 0, 0, 0)), ("A8W4_MXFP_dynamic", 128, (0, 0, 0, 0)),
    ("A4W4_MXFP_dynamic", 1, (0, 0, 0, 0)), ("A4W4_MXFP_dynamic", 128, (0, 2, 2, 0)), ("A4W4_MXFP_dynamic", 128, (3, 0, 0, 0)),
    ("A16W4_MXFP", 1, (0, 0, 0, 0)), ("A16W4_MXFP", 128, (0, 0, 0, 0)), ("A16W8_MXFP", 128, (0, 0, 0, 0))])
def test_mx_families_one_hot_is_exact(proc_name, M, tuning):
    """one-hot activations (1.0 quantises exactly in mxfp8 and mxfp4: block scale 2^-8 x 256, 2^-2 x 4) x the layer's own element
    bytes and e8m0 scales: y[k][n] = element(k, n) * 2^(scale - 127) exactly"""
    from tests.test_mx_gpu import _weights_nk
    from oracle import mx_oracle as MX
    N, K = 512, 1024
    g = torch.Generator().manual_seed(11)
    W = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
    tdt = torch.bfloat16
    lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=tdt)
    lin.weight.data = W.to(tdt).to(DEV)
    lin.weight.requires_grad = False
    kw = dict(post_scale=False) if proc_name.startswith("A8W") else {}   # e8m0 microscales inside the contraction: all powers of two
    layer = getattr(H, proc_name)(device=DEV, dtype=tdt, **kw).from_linear(lin, del_orig=False)
    wv, ws = _weights_nk(layer)                                                   # [N, K] values, [N, K/32] e8m0 bytes
    E = torch.from_numpy((wv.astype(np.float64) * np.repeat(np.exp2(ws.astype(np.float64) - 127.0), layer.group_size, axis=1))
                         .astype(np.float32)).t().contiguous()
    assert torch.equal(E.to(tdt).float(), E)
    C = gemlite_amd.core
    C.TUNING_OVERRIDE = tuning if any(tuning) else None
    try:
        Y = _sweep(lambda x: layer(x), M, K, tdt)
    finally:
        C.TUNING_OVERRIDE = None
    _exact(f"mx {proc_name} M{M} {tuning}", Y, E)


# ------------------------------------------------------------------------------------------------ split-K combine protocols
@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("nbits", [4, 2])
def test_reduce_scatter_combine_equals_the_ticket_combine_bit_for_bit(nbits, tdt):
    """8-wave MFMA kernel, K split S ways: peers write the row blocks they do not own into the owner's inbox and the owner adds
    the copies in slice order (default from 4 slices on when tiles x S fit one wave of resident blocks; tuning[3] & 2048: with 2 too) — the same additions in the same order as
    the slab + ticket protocol (tuning[3] & 128).  Random data, ragged M, every (tile rows, S) pair, repeated calls on one
    workspace (the arrival counters must come back to zero)."""
    from oracle import gemlite_oracle as O
    N, K = 1024, 2048
    W_q, sc, zr = O.gen_data(N, K, nbits, 128, seed=90 + nbits)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(nbits, 128, K, N, code, code)
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(sc.astype(np.float32)).to(tdt).to(DEV),
             torch.from_numpy(zr.astype(np.float32)).to(tdt).to(DEV), None)
    for mi, S, M in ((2, 2, 64), (2, 2, 50), (4, 2, 128), (4, 4, 128), (4, 4, 100), (8, 2, 256), (8, 4, 256), (8, 8, 256),
                     (8, 8, 200), (8, 4, 512)):
        x = torch.from_numpy(O.gen_x(M, K, seed=M + S).astype(np.float32)).to(tdt).to(DEV)
        meta = lin.get_meta_args()
        y_t = _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, S, mi, 128))
        outs = [_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, S, mi, 2048)) for _ in range(3)]  # (2 slices: opt-in)
        # tuning[3] & 256: every block polls once and then hands its rows over (own partial into its inbox, "left" bit): the
        # peer that delivers last finishes them — or the block itself when everybody had delivered by then.  Same bits again,
        # and the arrival words are back at zero (the plain launches in between would otherwise miscount).
        outs += [_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, S, mi, 256)) for _ in range(3)]
        outs += [_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, S, mi, 2048))]
        torch.cuda.synchronize()
        for i, y in enumerate(outs):
            assert torch.equal(y, y_t), (mi, S, M, i, float((y.float() - y_t.float()).abs().max()))


def test_two_streams_of_reduce_scatter_launches_cannot_park_each_other():
    """Two streams, each launching 256-block reduce-scatter kernels back to back: the launches share the device, so the slices of
    a tile are NOT all resident at once.  The wait for the peers is bounded (a late peer's rows are handed over), so both streams
    finish, and every result equals the ticket protocol's bits."""
    from oracle import gemlite_oracle as O
    N, K, M = 4096, 4096, 256
    tdt = torch.bfloat16
    W_q, sc, zr = O.gen_data(N, K, 4, 128, seed=5)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, 128, K, N, code, code)
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(sc.astype(np.float32)).to(tdt).to(DEV),
             torch.from_numpy(zr.astype(np.float32)).to(tdt).to(DEV), None)
    meta = lin.get_meta_args()
    xs = [torch.from_numpy(O.gen_x(M, K, seed=i).astype(np.float32)).to(tdt).to(DEV) for i in range(4)]
    assert _name(lin, M, 4, (0, 4, 4, 0)) == "gemm_w4_mma_kernel<128x128>"
    ref = [_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, 4, 4, 128)) for x in xs]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [[], []]
    for rep in range(60):
        for si, st in enumerate(streams):
            with torch.cuda.stream(st):
                outs[si].append(_hip_matmul(xs[(rep + si) % 4], lin.W_q, lin.scales, lin.zeros, None, meta, 4, (0, 4, 4, 0)))
    for st in streams:
        st.synchronize()
    for si in range(2):
        for rep, y in enumerate(outs[si]):
            assert torch.equal(y, ref[(rep + si) % 4]), (si, rep)
