"""The block-scaled weight quantiser on the GPU: gemlite_hip_quantize_mx against the torch restatement of its contract
(tests/quant_mx_spec.py) and against the reference's recorded results (tests/golden/mx.npz) bit for bit, both element forms, both scale
layouts, views, guard bands, non-finite blocks, graph capture, and the layers the MXFP / NVFP processors and patch_model build from it.
Shapes are the smallest that reach each path of the kernel."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from gemlite_amd import GemLiteLinear, _hip, helper
from gemlite_amd.dtypes import TORCH_TO_DTYPE
from gemlite_amd.quant_utils import WeightQuantizerMXFP
from tests.quant_mx_spec import E4M3_NAN, E8M0_NAN, FORMATS, pack_nibbles, planted_weights_mx, quantize_mx_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mx.npz"))

# one tile | the smallest | the golden's shape | ragged N with K no multiple of 256 | several tiles both ways
SHAPES = [(64, 256), (1, 32), (48, 256), (80, 384), (200, 1024)]
RAGGED = (80, 384)
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
FORMS = [("mxfp8", 0), ("mxfp4", 0), ("mxfp4", 1), ("nvfp4", 0), ("nvfp4", 1)]  # (format, two codes per byte)


def launch(W, fmt, pack, q, ld_q, scales, stride_g, stride_n, expect=0):
    """Raw C ABI call: W any 2-D view with unit inner stride; q / scales tensors (or views) written in place."""
    a = _hip.QuantizeMxArgs()
    a.struct_size = C.sizeof(_hip.QuantizeMxArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, W.shape[0], W.shape[1], W.stride(0)
    a.format, a.pack_nibbles, a.q_out, a.ld_q = FORMATS[fmt][0], pack, q.data_ptr(), ld_q
    a.scales, a.stride_scale_g, a.stride_scale_n = scales.data_ptr(), stride_g, stride_n
    rc = _hip.load().gemlite_hip_quantize_mx(C.byref(a), _hip.current_stream_handle(W.device))
    assert rc == expect, _hip.status_string(rc)


def run(W, fmt, pack, by_group):
    """-> (element bytes [N, K or K/2], scale bytes [N, K/g]); by_group: the scales are written as the layer's [K/g, N]"""
    N, K = W.shape
    g = FORMATS[fmt][1]
    q = torch.empty((N, K // 2 if pack else K), dtype=torch.uint8, device=W.device)
    if by_group:
        s = torch.empty((K // g, N), dtype=torch.uint8, device=W.device)
        launch(W, fmt, pack, q, q.stride(0), s, N, 1)
        return q, s.t()
    s = torch.empty((N, K // g), dtype=torch.uint8, device=W.device)
    launch(W, fmt, pack, q, q.stride(0), s, 1, K // g)
    return q, s


@functools.lru_cache(maxsize=None)
def reference(N, K, dt, fmt):
    """(W on the CPU, spec elements, spec scale bytes): computed once, shared, never modified."""
    W = planted_weights_mx(N, K, DTYPES[dt], seed=N * 7 + K)
    el, sb, bad = quantize_mx_spec(W, fmt)
    assert not bad.any()
    return W, el, sb


# ------------------------------------------------------------------------------------------------ kernel against the restatement
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("N,K", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_matches_the_restatement(N, K, fmt, dt):
    W, el, sb = reference(N, K, dt, fmt)
    Wd = W.to(DEV)
    for pack in ((0,) if fmt == "mxfp8" else (0, 1)):
        want = pack_nibbles(el) if pack else el
        for by_group in (False, True):
            q, s = run(Wd, fmt, pack, by_group)
            assert torch.equal(s.cpu(), sb), (pack, by_group)
            assert torch.equal(q.cpu(), want), (pack, by_group)


@pytest.mark.parametrize("dt", list(DTYPES))
def test_quantizer_methods_take_the_kernel_and_keep_their_return_types(dt):
    N, K = RAGGED
    wq = WeightQuantizerMXFP(device=DEV)
    for fmt, fn, qdt, sdt in (("mxfp8", wq.quantize_mxfp8, torch.float8_e4m3fn, torch.float8_e8m0fnu),
                              ("mxfp4", wq.quantize_mxfp4, torch.uint8, torch.float8_e8m0fnu),
                              ("nvfp4", wq.quantize_nvfp4, torch.uint8, torch.float8_e4m3fn)):
        W, el, sb = reference(N, K, dt, fmt)
        g = FORMATS[fmt][1]
        q, s = fn(W.to(DEV), index=True)
        assert q.dtype == qdt and tuple(q.shape) == (N * K // g, g) and s.dtype == sdt and tuple(s.shape) == (N * K // g, 1)
        assert torch.equal(q.view(torch.uint8).cpu().view(N, K), el) and torch.equal(s.view(torch.uint8).cpu().view(N, K // g), sb)
        qp, sp = wq.quantize_packed(W.to(DEV), fmt)
        assert tuple(qp.shape) == ((N, K) if fmt == "mxfp8" else (N, K // 2)) and qp.dtype == qdt and qp.is_contiguous()
        assert tuple(sp.shape) == (K // g, N) and sp.is_contiguous() and sp.dtype == (torch.float8_e4m3fn if fmt == "nvfp4" else torch.uint8)
        assert torch.equal(qp.view(torch.uint8).cpu(), el if fmt == "mxfp8" else pack_nibbles(el))
        assert torch.equal(sp.view(torch.uint8).cpu().t(), sb)


# ------------------------------------------------------------------------------------------------ kernel against the reference's results
def _golden_W():
    return torch.from_numpy(Z["wq_in_W"].copy()).view(torch.bfloat16)


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_matches_the_reference_quantiser_results(fmt):
    W = _golden_W().to(DEV)
    for pack in ((0,) if fmt == "mxfp8" else (0, 1)):
        q, s = run(W, fmt, pack, by_group=bool(pack))
        want = torch.from_numpy(Z[f"wq_{fmt}_q"].reshape(48, 256))
        assert torch.equal(q.cpu(), pack_nibbles(want) if pack else want)
        assert np.array_equal(s.cpu().numpy().reshape(-1), Z[f"wq_{fmt}_s"].reshape(-1))
    wq = WeightQuantizerMXFP(compute_dtype=torch.bfloat16, device=DEV)
    q, s = {"mxfp8": wq.quantize_mxfp8, "mxfp4": wq.quantize_mxfp4, "nvfp4": wq.quantize_nvfp4}[fmt](W, index=True)
    assert np.array_equal(q.view(torch.uint8).cpu().numpy().reshape(-1), Z[f"wq_{fmt}_q"].reshape(-1))
    assert np.array_equal(s.view(torch.uint8).cpu().numpy().reshape(-1), Z[f"wq_{fmt}_s"].reshape(-1))


PROCS = {
    "a16w8_mxfp": lambda: helper.A16W8_MXFP(device=DEV, dtype=torch.bfloat16),
    "a16w4_mxfp": lambda: helper.A16W4_MXFP(device=DEV, dtype=torch.float16),
    "a8w8_mxfp_dyn_post": lambda: helper.A8W8_MXFP_dynamic(device=DEV, dtype=torch.bfloat16, post_scale=True),
    "a8w8_mxfp_dyn_micro": lambda: helper.A8W8_MXFP_dynamic(device=DEV, dtype=torch.bfloat16, post_scale=False),
    "a8w4_mxfp_dyn": lambda: helper.A8W4_MXFP_dynamic(device=DEV, dtype=torch.bfloat16, post_scale=False),
    "a4w4_mxfp_dyn": lambda: helper.A4W4_MXFP_dynamic(device=DEV, dtype=torch.bfloat16),
    "a4w4_nvfp_dyn": lambda: helper.A4W4_NVFP_dynamic(device=DEV, dtype=torch.float16),
}


@pytest.mark.parametrize("name", list(PROCS))
def test_processors_pack_like_the_reference_on_the_gpu(name):
    """The from_linear of tests/test_mx_cpu.py::test_processors_pack_like_the_reference with the layer on the GPU (the fused route)."""
    W = _golden_W()
    lin = torch.nn.Linear(W.shape[1], W.shape[0], bias=True, dtype=torch.bfloat16, device=DEV)
    with torch.no_grad():
        lin.weight.copy_(W)
        lin.bias.copy_(torch.from_numpy(Z["proc_in_bias"].copy()).view(torch.bfloat16))
    proc = PROCS[name]()
    assert proc._fused(lin.weight.data)
    layer = proc.from_linear(lin, del_orig=False)
    assert lin.weight is not None and lin.bias is not None
    wq, sc = layer.W_q.data, layer.scales.data
    assert wq.is_cuda and sc.is_cuda
    assert list(wq.shape) + list(wq.stride()) == [int(v) for v in Z[f"proc_{name}_W_q_shape_stride"]]
    assert list(sc.shape) + list(sc.stride()) == [int(v) for v in Z[f"proc_{name}_scales_shape_stride"]]
    assert np.array_equal(wq.contiguous().view(torch.uint8).cpu().numpy(), Z[f"proc_{name}_W_q"])
    assert np.array_equal(sc.contiguous().view(torch.uint8).cpu().numpy(), Z[f"proc_{name}_scales"])
    assert layer.get_meta_args() == [int(v) for v in Z[f"proc_{name}_meta"]]
    mine = layer.bias.data.cpu()
    mine = mine.view(torch.int16).numpy() if mine.dtype == torch.bfloat16 else mine.numpy()
    assert np.array_equal(mine, Z[f"proc_{name}_bias"])


# ------------------------------------------------------------------------------------------------ layers
def _same_layer(a: GemLiteLinear, b: GemLiteLinear):
    for name in ("W_q", "scales", "zeros", "bias"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is not None:
            assert ta.dtype == tb.dtype and ta.shape == tb.shape and ta.stride() == tb.stride(), name
            assert torch.equal(ta.view(torch.uint8) if ta.element_size() == 1 else ta, tb.view(torch.uint8) if tb.element_size() == 1 else tb), name
    assert a.get_meta_args() == b.get_meta_args()
    assert torch.equal(a.metadata, b.metadata) and torch.equal(a.orig_shape, b.orig_shape)
    assert list(a.state_dict().keys()) == list(b.state_dict().keys())
    for attr in ("W_nbits", "group_size", "elements_per_sample", "data_contiguous", "meta_is_channelwise", "scaled_activations"):
        assert getattr(a, attr) == getattr(b, attr), attr


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", list(PROCS))
def test_fused_layer_equals_from_weights_of_quantize(name, bias):
    N, K = 128, 256
    proc = PROCS[name]()
    dtype = proc.dtype
    W = planted_weights_mx(N, K, dtype, seed=3)
    W = torch.where(W.float().abs() > 1e3, torch.zeros_like(W), W).to(DEV)  # (the outputs below stay finite)
    b = (torch.randn(N, device=DEV) / 4).to(dtype) if bias else None
    lin = torch.nn.Linear(K, N, bias=bias, device=DEV, dtype=dtype)
    with torch.no_grad():
        lin.weight.copy_(W)
        if bias:
            lin.bias.copy_(b)
    layer = proc.from_linear(lin, del_orig=True)
    assert lin.weight is None and (lin.bias is None)  # cleanup_linear as before
    g = proc.group_size
    W_q, scales = proc._quantize(W)  # the unfused route: codes / fp8 [N * K/g, g], scales [N * K/g, 1]
    want = helper._BlockScaledProcessor.from_weights(PROCS[name](), weight=W_q.view(N, K), bias=b, scales=scales.view(N, K // g))
    _same_layer(layer, want)
    third = PROCS[name]().quantize_weights(W, b)
    _same_layer(third, want)
    for M in (1, 16):
        x = (torch.randn(M, K, device=DEV) / 10).to(dtype)
        y, y_want = layer(x), want(x)
        assert y.dtype == y_want.dtype and torch.isfinite(y).all() and torch.equal(y, y_want), f"M = {M}"


def test_quantize_weights_falls_back_for_inputs_the_kernel_does_not_take():
    proc = helper.A8W8_MXFP_dynamic(device=DEV, dtype=torch.bfloat16, fp8=torch.float8_e5m2)
    W = planted_weights_mx(32, 64, torch.bfloat16, seed=1).to(DEV)
    assert not proc._fused(W)
    layer = proc.quantize_weights(W)  # e5m2 elements: the torch code
    assert layer.W_q.dtype == torch.float8_e5m2 and tuple(layer.W_q.shape) == (64, 32)


def test_patch_model_builds_the_layers_of_from_linear():
    torch.manual_seed(5)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64))
            self.lm_head = torch.nn.Linear(64, 32)

        def forward(self, x):
            return self.lm_head(self.body(x))

    net = Net().to(device=DEV, dtype=torch.bfloat16)
    copies = []
    for src in (net.body[0], net.body[2]):
        lin = torch.nn.Linear(src.in_features, src.out_features).to(device=DEV, dtype=torch.bfloat16)
        lin.load_state_dict(src.state_dict())
        copies.append(lin)
    helper.patch_model(net, DEV, helper.A8W4_MXFP_dynamic(dtype=torch.bfloat16, post_scale=False))
    assert isinstance(net.body[0], GemLiteLinear) and isinstance(net.body[2], GemLiteLinear) and type(net.lm_head) is torch.nn.Linear
    for got, lin in zip((net.body[0], net.body[2]), copies):
        _same_layer(got, helper.A8W4_MXFP_dynamic(device=DEV, dtype=torch.bfloat16, post_scale=False).from_linear(lin))
    assert net(torch.randn(3, 256, device=DEV, dtype=torch.bfloat16)).shape == (3, 32)


# ------------------------------------------------------------------------------------------------ views, guard bands, non-finite, capture
@pytest.mark.parametrize("dt", ["fp16", "fp32"])
@pytest.mark.parametrize("fmt,pack", FORMS, ids=[f"{f}-pack{p}" for f, p in FORMS])
def test_view_of_a_larger_matrix(fmt, pack, dt):
    N, K = RAGGED
    W = planted_weights_mx(N, K, DTYPES[dt], seed=7).to(DEV)
    big = torch.zeros(N + 3, K + 72, device=DEV, dtype=DTYPES[dt])
    view = big[2:2 + N, 1:1 + K]  # ld_w > K, first element one element past an aligned address
    view.copy_(W)
    assert view.stride(0) > K and view.data_ptr() % 16 != 0
    for a, b in zip(run(view, fmt, pack, bool(pack)), run(W, fmt, pack, bool(pack))):
        assert torch.equal(a, b)


@pytest.mark.parametrize("fmt,pack", FORMS, ids=[f"{f}-pack{p}" for f, p in FORMS])
def test_guard_bands(fmt, pack):
    N, K = RAGGED
    g = FORMATS[fmt][1]
    G, row = K // g, (K // 2 if pack else K)
    W, el, sb = reference(N, K, "bf16", fmt)
    want_q = pack_nibbles(el) if pack else el
    qbuf = torch.full((N + 2, row + 24), 0xA5, dtype=torch.uint8, device=DEV)
    qwin = qbuf[1:1 + N, 5:5 + row]  # ld_q > row, unaligned start: the padding of every row is guard band too
    if pack:  # the layer's [K/g, N], inside a larger buffer
        sbuf = torch.full((G + 2, N + 5), 0x33, dtype=torch.uint8, device=DEV)
        swin, sg, sn = sbuf[1:1 + G, 3:3 + N], N + 5, 1
        want_s = sb.t()
    else:     # the quantiser's [N, K/g], inside a larger buffer
        sbuf = torch.full((N + 2, G + 3), 0x33, dtype=torch.uint8, device=DEV)
        swin, sg, sn = sbuf[1:1 + N, 2:2 + G], 1, G + 3
        want_s = sb
    before = [qbuf.clone(), sbuf.clone()]
    launch(W.to(DEV), fmt, pack, qwin, qbuf.stride(0), swin, sg, sn)
    torch.cuda.synchronize()
    assert torch.equal(qwin.cpu(), want_q) and torch.equal(swin.cpu(), want_s)
    for buf, win, old in ((qbuf, qwin, before[0]), (sbuf, swin, before[1])):
        outside = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(outside, win.shape, win.stride(), win.storage_offset()).fill_(False)
        assert torch.equal(buf[outside], old[outside])
    # an aligned window with padded rows: the vector stores leave the padding alone as well
    qbuf2 = torch.full((N, row + 8), 0xA5, dtype=torch.uint8, device=DEV)
    launch(W.to(DEV), fmt, pack, qbuf2, qbuf2.stride(0), swin, sg, sn)
    torch.cuda.synchronize()
    assert torch.equal(qbuf2[:, :row].cpu(), want_q) and (qbuf2[:, row:] == 0xA5).all()


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("fmt,pack", FORMS, ids=[f"{f}-pack{p}" for f, p in FORMS])
def test_non_finite_blocks_get_the_nan_code(fmt, pack, dt):
    N, K = RAGGED
    g = FORMATS[fmt][1]
    W = planted_weights_mx(N, K, DTYPES[dt], seed=21).clone()
    W[3, 40], W[70, 300], W[79, K - 1] = float("nan"), float("inf"), float("-inf")
    el, sb, bad = quantize_mx_spec(W, fmt)
    assert int(bad.sum()) == 3
    q, s = run(W.to(DEV), fmt, pack, bool(pack))  # (the launch returned OK)
    torch.cuda.synchronize()
    q, s = q.cpu(), s.cpu()
    assert torch.equal(s, sb) and (s[bad] == (E4M3_NAN if fmt == "nvfp4" else E8M0_NAN)).all()
    keep = ~bad.repeat_interleave(g // 2 if pack else g, dim=1)
    want = pack_nibbles(el) if pack else el
    assert torch.equal(q[keep], want[keep])


def test_deterministic_and_capturable_on_a_side_stream():
    N, K = RAGGED
    for fmt, pack in FORMS:
        W, el, sb = reference(N, K, "bf16", fmt)
        Wd = W.to(DEV)
        eager_q, eager_s = run(Wd, fmt, pack, True)
        again_q, again_s = run(Wd, fmt, pack, True)
        assert torch.equal(eager_q, again_q) and torch.equal(eager_s, again_s)
        q = torch.zeros_like(eager_q)
        s = torch.zeros((K // FORMATS[fmt][1], N), dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            launch(Wd, fmt, pack, q, q.stride(0), s, N, 1)
        assert not q.any() and not s.any()  # captured, not run
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(q, eager_q) and torch.equal(s.t(), eager_s)
