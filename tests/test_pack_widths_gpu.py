"""8- and 16-bit packed words on the MI355X (`pytest -m gpu`): layers packed with packing_bitwidth=8 / 16 (uint8 / int16 W_q) run on the
GEMV and the MFMA tile kernel, not on the coverage kernel.

  * exactness: one-hot x times position-coded codes and power-of-two scales (tests/test_structured_exact_gpu.py), kernel label asserted;
  * same bits: the same W_q packed into 32-, 16- and 8-bit words gives bit-identical outputs wherever the labels agree but for the suffix
    (the byte / short rows concatenate to the int32 words: only the word source differs), the float64 oracle elsewhere;
  * the public surface (processors, set_packing_bitwidth, state_dict round trip, torch.compile, graph capture, no coverage warning);
  * guard bands around the output and a W_q view at an offset."""
import logging

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear, helper as H
from gemlite_amd.core import _hip_matmul
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_gpu import _run
from tests.test_gpu_parity import _compare, _oracle_from_layer
from tests.test_structured_exact_gpu import _exact, _name, _sweep

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TDTS = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]
SUFFIX = {8: ",b8>", 16: ",b16>", 32: ">"}


def _coded(N, K, nbits, gs, tdt, pb):
    """position-coded layer packed into pb-bit words and its exact dequantised matrix [K, N] (float32)"""
    k = torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    mask = (1 << nbits) - 1
    W = ((k * 5 + n * 3 + (k >> 4) + (n >> 3)) & mask).to(torch.uint8)
    g = torch.arange(K // gs).view(1, -1)
    z = ((g * 3 + n) & mask).float()
    s = torch.pow(2.0, ((g + n) % 3 - 1).float())
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(nbits, gs, K, N, code, code)
    lin.pack(W.to(DEV), s.reshape(-1, 1).to(tdt).to(DEV), z.reshape(-1, 1).to(tdt).to(DEV), None, packing_bitwidth=pb)
    E = (W.float() - z.repeat_interleave(gs, dim=1)) * s.repeat_interleave(gs, dim=1)
    return lin, E.t().contiguous()


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("pb", [8, 16])
@pytest.mark.parametrize("nbits", [4, 2])
def test_pack_widths_one_hot_is_exact(nbits, pb, tdt):
    N, K, gs = 1024, 2048, 128
    lin, E = _coded(N, K, nbits, gs, tdt, pb)
    assert lin.W_q.element_size() * 8 == pb
    meta = lin.get_meta_args()
    ran = {}
    # (label, matmul_type, M, tuning): auto plans at every row count, a forced split-K tile plan, the reduce-scatter combine, the wide tiles
    for label, mt, M, tuning in (("m1", -1, 1, (0, 0, 0, 0)), ("m3", -1, 3, (0, 0, 0, 0)), ("m17", -1, 17, (0, 0, 0, 0)),
                                 ("m64", -1, 64, (0, 0, 0, 0)), ("m256", -1, 256, (0, 0, 0, 0)),
                                 ("mma64_sk3", 4, 64, (0, 3, 2, 0)), ("mma128_xch4", 4, 128, (0, 4, 4, 0)),
                                 ("mma_wide256", 4, 256, (0, 1, 24, 0)), ("gemv_tile64_sk2", -1, 1, (4, 2, 0, 0))):
        name = _name(lin, M, mt, tuning)
        assert name.endswith(SUFFIX[pb]) and "generic" not in name, (label, name)
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, mt, tuning), M, K, tdt)
        _exact(f"{label} [{name}] w{nbits} b{pb} {tdt}", Y, E)
        # the label the layer itself reports for the same call
        ran[label] = name
    assert ran["mma128_xch4"].startswith(f"gemm_w{nbits}_mma_kernel<128x128")
    assert ran["m1"].startswith("gemv_wn_kernel<")


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("pb", [8, 16])
def test_pack_widths_long_k_is_exact(pb, tdt):
    """K = 8192 + 128 (65 groups): many passes over the register ring / chunk loops, uneven K slices"""
    N, K, gs = 512, 8320, 128
    lin, E = _coded(N, K, 4, gs, tdt, pb)
    meta = lin.get_meta_args()
    for label, mt, M, tuning in (("auto_m32", -1, 32, (0, 0, 0, 0)), ("mma256_sk5", 4, 256, (0, 5, 8, 0))):
        name = _name(lin, M, mt, tuning)
        assert name.endswith(SUFFIX[pb]), name
        Y = _sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, mt, tuning), M, K, tdt)
        _exact(f"long-k {label} [{name}] b{pb} {tdt}", Y, E)
    ks = sorted(set(range(0, K, 16)) | set(range(K - 130, K)))
    I = torch.zeros(len(ks), K, device=DEV, dtype=tdt)
    I[torch.arange(len(ks)), torch.tensor(ks)] = 1
    assert _name(lin, 1, -1, (0, 0, 0, 0)).endswith(SUFFIX[pb])
    rows = [_hip_matmul(I[i:i + 1], lin.W_q, lin.scales, lin.zeros, None, meta, -1, (0, 0, 0, 0)) for i in range(len(ks))]
    _exact(f"long-k m1 b{pb} {tdt}", torch.cat(rows, 0).float(), E[ks])


def _layers(N, K, nbits, gs, tdt, seed=0):
    W_q, scales, zeros = O.gen_data(N, K, nbits, gs, seed=seed)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    out = {}
    for pb in (32, 16, 8):
        lin = GemLiteLinear(nbits, gs, K, N, code, code)
        lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales).to(tdt).to(DEV), torch.from_numpy(zeros).to(tdt).to(DEV), packing_bitwidth=pb)
        out[pb] = lin
    return out


@pytest.mark.parametrize("tdt", TDTS, ids=IDS)
@pytest.mark.parametrize("nbits", [4, 2])
@pytest.mark.parametrize("N,K", [(4096, 4096), (1536, 8960)])
def test_pack_widths_same_bits_as_32_bit_words(N, K, nbits, tdt):
    layers = _layers(N, K, nbits, 128, tdt)
    same = 0
    for M in (1, 3, 17, 64, 100, 256, 1024):
        x = torch.from_numpy(O.gen_x(M, K, seed=M).astype(np.float32)).to(tdt).to(DEV)
        y32 = layers[32](x)
        n32 = _name(layers[32], M, -1, (0, 0, 0, 0))
        y_ref = None
        for pb in (16, 8):
            lin = layers[pb]
            name = _name(lin, M, -1, (0, 0, 0, 0))
            assert name.endswith(SUFFIX[pb]), (M, pb, name)
            y = lin(x)
            if name == n32[:-1] + SUFFIX[pb]:
                assert torch.equal(y, y32), (M, pb, name)
                same += 1
            else:
                if y_ref is None:
                    y_ref = _oracle_from_layer(lin, x)
                _compare(f"pack_widths/{N}x{K}/M{M}/b{pb}", y, y_ref, gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value, extra=dict(kernel=name))
    assert same >= 4


def test_pack_widths_public_surface(caplog):
    torch.manual_seed(0)
    N, K = 2048, 4096
    Wc, sc, zc = (torch.from_numpy(t) for t in O.gen_data(N, K, 4, 128, seed=2))
    x = torch.randn(64, K, device=DEV, dtype=torch.float16) / 8
    ref = H.A16W4_HQQ_INT(device=DEV, dtype=torch.float16).from_weights(Wc, sc, zc, 4, 128)
    with caplog.at_level(logging.WARNING):
        layer8 = H.A16W4_HQQ_INT(device=DEV, dtype=torch.float16, packing_bitwidth=8).from_weights(Wc, sc, zc, 4, 128)
        assert layer8.W_q.dtype == torch.uint8
        prev = gemlite_amd.core.GemLiteLinearHIP.PACKING_BITWIDTH
        try:
            gemlite_amd.set_packing_bitwidth(16)
            W_q, s, z = O.gen_data(N, K, 4, 128, seed=3)
            layer16 = GemLiteLinear(4, 128, K, N, DType.FP16, DType.FP16)
            layer16.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(s).half().to(DEV), torch.from_numpy(z).half().to(DEV))
        finally:
            gemlite_amd.set_packing_bitwidth(prev)
        assert layer16.W_q.dtype == torch.int16
        for M in (1, 5, 64):
            xm = x[:M].contiguous()
            y8, yr = layer8(xm), ref(xm)
            assert _name(layer8, M, -1, (0, 0, 0, 0)).endswith(",b8>")
            assert _name(layer16, M, -1, (0, 0, 0, 0)).endswith(",b16>")
            if _name(layer8, M, -1, (0, 0, 0, 0))[:-4] == _name(ref, M, -1, (0, 0, 0, 0))[:-1]:
                assert torch.equal(y8, yr)
            else:
                assert (y8.float() - yr.float()).abs().max() <= 1e-2 * yr.float().abs().max()
            layer16(xm)
        torch.cuda.synchronize()
    assert not [r for r in caplog.records if "coverage" in r.getMessage()], [r.getMessage() for r in caplog.records]

    # state_dict round trip keeps the width and the kernels
    sd = layer8.state_dict()
    assert sd["W_q"].dtype == torch.uint8
    fresh = GemLiteLinear(4, 128, K, N, DType.FP16, DType.FP16)
    fresh.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert fresh.W_q.dtype == torch.uint8
    assert torch.equal(fresh(x), layer8(x))

    # torch.compile(fullgraph=True) and a captured graph
    xs = x[:16].contiguous()
    eager = layer8(xs)
    comp = torch.compile(lambda t: layer8(t), fullgraph=True)
    assert torch.equal(comp(xs), eager)
    static_x = xs.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        layer8(static_x)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = layer8(static_x)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, eager)


@pytest.mark.parametrize("pb", [8, 16])
@pytest.mark.parametrize("M", [1, 17, 129])
def test_pack_widths_guard_bands(M, pb):
    """output window with canaries and a strided output (layout 'aligned' of tests/test_abi_bounds_gpu.py), and W_q as a view one element
    off (not 4-byte aligned for 8-bit words: whatever the planner picks for it must still be right)"""
    tdt = torch.float16
    W_q, scales, zeros = O.gen_data(1024, 2048, 4, 128, seed=1)
    lin = GemLiteLinear(4, 128, 2048, 1024, DType.FP16, DType.FP16)
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales).half().to(DEV), torch.from_numpy(zeros).half().to(DEV), packing_bitwidth=pb)
    case = dict(M=M, tuning=(0, 0, 0, 0), fused=False)
    x16 = torch.from_numpy(O.gen_x(M, 2048, seed=M).astype(np.float32)).to(tdt).to(DEV)
    y_ref = _oracle_from_layer(lin, x16)
    y0, n0, _ = _run(lin, case, x16, None, None)
    assert n0.endswith(SUFFIX[pb]), n0
    for w_extra in (64, 1):
        y, n, _ = _run(lin, case, x16, None, 64, w_extra=w_extra)
        _compare(f"pack_widths/bounds/b{pb}/M{M}/w{w_extra}", y, y_ref, DType.FP16.value, extra=dict(kernel=n))
        if w_extra == 64:
            assert n == n0
            assert torch.equal(y.view(torch.int16), y0.view(torch.int16))
