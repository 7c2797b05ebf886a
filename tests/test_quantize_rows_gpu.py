"""The channel-wise 8-bit weight quantiser on the GPU: gemlite_hip_quantize_rows against the torch restatement of its contract
(tests/quant_rows_spec.py) bit for bit — every form of the kernel, both scale rules, views, guard bands, non-finite rows, graph capture —
against the torch sequence the processors ran on the GPU before (the test that decides the processors' scale rule), and the layers the
A16W8 / A8W8 processors and patch_model build from it, with their peak memory.  Shapes are the smallest that reach each form."""
import ctypes as C
import functools

import pytest
import torch

from gemlite_amd import GemLiteLinear, _hip, helper, quant_utils
from gemlite_amd.dtypes import TORCH_TO_DTYPE
from gemlite_amd.quant_utils import WeightQuantizerRows, _quantize_rows_torch
from tests.quant_rows_spec import FORMATS, planted_weights_rows, quantize_rows_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KW, KR = _hip.QUANT_ROWS_WAVE_MAX_K, _hip.QUANT_ROWS_RESIDENT_MAX_K  # the longest row of the wave form / of the resident form
# one element | ragged, one wave | the longest wave row | the shortest block row, ragged | the longest resident row | the shortest
# re-read row | a re-read row with a ragged tail, unaligned rows
SHAPES = [(1, 1), (5, 17), (7, KW), (3, KW + 8), (2, KR), (2, KR + 8), (1, 2 * KR + 3)]
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
SCALE_DTYPES = {"fp16": (torch.float32, torch.float16), "bf16": (torch.float32, torch.bfloat16), "fp32": (torch.float32, torch.float16, torch.bfloat16)}


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def launch(W, fmt, rule, q, ld_q, scales, stride_s, expect=0):
    """Raw C ABI call: W any 2-D view with unit inner stride; q / scales tensors (or views) written in place."""
    a = _hip.QuantizeRowsArgs()
    a.struct_size = C.sizeof(_hip.QuantizeRowsArgs)
    a.w, a.w_dtype, a.N, a.K = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, W.shape[0], W.shape[1]
    a.ld_w = W.stride(0) if W.shape[0] > 1 else max(W.shape[1], W.stride(0))
    a.format, a.scale_rule, a.q_out, a.ld_q = FORMATS[fmt][0], rule, q.data_ptr(), ld_q
    a.scales, a.stride_s, a.scale_dtype = scales.data_ptr(), stride_s, TORCH_TO_DTYPE[scales.dtype].value
    rc = _hip.load().gemlite_hip_quantize_rows(C.byref(a), _hip.current_stream_handle(W.device))
    assert rc == expect, _hip.status_string(rc)


def run(W, fmt, rule, sdt=torch.float32):
    """-> (code bytes uint8 [N, K], scales [N, 1] of sdt)"""
    N, K = W.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=W.device)
    s = torch.empty((N, 1), dtype=sdt, device=W.device)
    launch(W, fmt, rule, q, K, s, 1)
    return q, s


@functools.lru_cache(maxsize=None)
def weights(N, K, dt):
    """W on the CPU: computed once, shared, never modified"""
    return planted_weights_rows(N, K, DTYPES[dt], seed=N * 7 + K)


@functools.lru_cache(maxsize=None)
def reference(N, K, dt, fmt, rule):
    """(spec code bytes, spec fp32 scales) of weights(N, K, dt)"""
    return quantize_rows_spec(weights(N, K, dt), fmt, rule)


# ------------------------------------------------------------------------------------------------ G1: kernel against the restatement
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("N,K", SHAPES, ids=[f"{n}x{k}" for n, k in SHAPES])
def test_matches_the_restatement(N, K, fmt, dt):
    Wd = weights(N, K, dt).to(DEV)
    for rule in (0, 1):
        codes, s = reference(N, K, dt, fmt, rule)
        for sdt in SCALE_DTYPES[dt]:
            q, sc = run(Wd, fmt, rule, sdt)
            q, sc = q.cpu(), sc.cpu()
            nq, ns = int((q != codes).sum()), int((_bits(sc) != _bits(s.to(sdt))).sum())
            print(f"{N} x {K} {fmt} {dt} rule {rule} scales {sdt}: {nq} codes, {ns} scales differ")
            assert ns == 0 and nq == 0, (rule, sdt)


# ------------------------------------------------------------------------------------------------ G2: views and guard bands
VIEW_SHAPES = [(5, 17), (3, KW + 8), (2, KR + 11)]  # one per form


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("N,K", VIEW_SHAPES, ids=[f"{n}x{k}" for n, k in VIEW_SHAPES])
def test_views_and_guard_bands(N, K, fmt, dt):
    W = weights(N, K, dt)
    codes, s = reference(N, K, dt, fmt, 1)
    sdt = torch.float32 if dt == "fp32" else torch.bfloat16
    esz = torch.empty(0, dtype=sdt).element_size()
    ld = (K + 8) // 4 * 4 + 5  # odd row pitches > K; ld + 1 is no multiple of 4: the windows below start off every 16-byte boundary
    big = torch.zeros(N + 2, ld, device=DEV, dtype=DTYPES[dt])
    view = big[1:1 + N, 1:1 + K]  # ld_w odd and > K, a first element that is not 16-byte aligned
    view.copy_(W)
    assert view.stride(0) == ld and ld % 2 == 1 and big.data_ptr() % 16 == 0 and view.data_ptr() % 16 != 0
    qbuf = torch.full((N + 2, ld), 0xA5, dtype=torch.uint8, device=DEV)
    qwin = qbuf[1:1 + N, 1:1 + K]  # ld_q odd and > K, unaligned start: the padding of every row is guard band too
    assert qbuf.data_ptr() % 16 == 0 and qwin.data_ptr() % 8 != 0
    sraw = torch.full(((N + 2) * 3 * esz,), 0x33, dtype=torch.uint8, device=DEV)
    sbuf = sraw.view(sdt).view(N + 2, 3)
    swin = sbuf[1:1 + N, 1:2]  # stride_s = 3
    before = [qbuf.clone(), sraw.clone()]
    launch(view, fmt, 1, qwin, ld, swin, 3)
    torch.cuda.synchronize()
    assert torch.equal(qwin.cpu(), codes) and torch.equal(_bits(swin.cpu()), _bits(s.to(sdt)))
    outside = torch.ones_like(qbuf, dtype=torch.bool)
    outside[1:1 + N, 1:1 + K] = False
    assert torch.equal(qbuf[outside], before[0][outside])
    souts = torch.ones((N + 2, 3, esz), dtype=torch.bool, device=DEV)
    souts[1:1 + N, 1] = False
    assert torch.equal(sraw[souts.view(-1)], before[1][souts.view(-1)])
    # aligned rows with padding behind a K that is no multiple of 8: the 8-byte stores leave the padding alone as well
    pitch = (K + 7) // 8 * 8 + 8
    qbuf2 = torch.full((N, pitch), 0xA5, dtype=torch.uint8, device=DEV)
    s2 = torch.empty((N, 1), dtype=sdt, device=DEV)
    launch(W.to(DEV), fmt, 1, qbuf2, pitch, s2, 1)
    torch.cuda.synchronize()
    assert torch.equal(qbuf2[:, :K].cpu(), codes) and bool((qbuf2[:, K:] == 0xA5).all()) and torch.equal(_bits(s2.cpu()), _bits(s.to(sdt)))


# ------------------------------------------------------------------------------------------------ G3: which rule the torch sequence follows on the GPU
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fmt", ["int8", "e4m3"])
@pytest.mark.parametrize("N,K", [(64, 520), (5, 17)], ids=["64x520", "5x17"])
def test_processors_rule_equals_the_torch_sequence_on_the_gpu(N, K, fmt, dt):
    """The decision test: with the rule the processors pass (quant_utils.ROWS_SCALE_RULE) the kernel gives the bytes the torch sequence gives
    on a GPU tensor — codes and scales, planted and random weights."""
    qdt = FORMATS[fmt][1]
    gen = torch.Generator().manual_seed(N + K)
    for kind, W in (("planted", weights(N, K, dt)), ("random", (torch.randn(N, K, generator=gen) * 0.05).to(DTYPES[dt]))):
        Wd = W.to(DEV)
        want_q, want_s = _quantize_rows_torch(Wd, qdt)
        assert want_q.is_cuda and want_s.dtype == torch.float32
        for rule in (0, 1):  # (the figures of both rules, before anything is asserted)
            q, s = run(Wd, fmt, rule)
            print(f"{kind} {N} x {K} {fmt} {dt} rule {rule}: {int((q != _bits(want_q)).sum())} codes, "
                  f"{int((_bits(s) != _bits(want_s)).sum())} scales differ from torch on the GPU")
        q, s = WeightQuantizerRows(qdt, device=DEV).quantize(Wd)
        assert q.dtype == qdt and tuple(q.shape) == (N, K) and s.dtype == torch.float32 and tuple(s.shape) == (N, 1)
        assert torch.equal(_bits(s), _bits(want_s)) and torch.equal(_bits(q), _bits(want_q)), kind


# ------------------------------------------------------------------------------------------------ G4: layers
F16, B16 = torch.float16, torch.bfloat16
PROCS = {
    "A16W8": (lambda: helper.A16W8(device=DEV, dtype=F16), "int8", F16),
    "A16W8_INT8": (lambda: helper.A16W8_INT8(device=DEV, dtype=B16), "int8", B16),
    "A16W8_INT8_post_scale": (lambda: helper.A16W8_INT8(device=DEV, dtype=F16, post_scale=True), "int8", F16),
    "A16W8_FP8": (lambda: helper.A16W8_FP8(device=DEV, dtype=B16), "e4m3", B16),
    "A16W8_FP8_e5m2_post_scale": (lambda: helper.A16W8_FP8(device=DEV, dtype=F16, fp8=torch.float8_e5m2, post_scale=True), "e5m2", F16),
    "A8W8_dynamic": (lambda: helper.A8W8_dynamic(device=DEV, dtype=F16), "int8", F16),
    "A8W8_dynamic_16bit_scale": (lambda: helper.A8W8_dynamic(device=DEV, dtype=B16, fp32_scale=False), "int8", B16),
    "A8W8_int8_dynamic": (lambda: helper.A8W8_int8_dynamic(device=DEV, dtype=B16), "int8", B16),
    "A8W8_fp8_dynamic": (lambda: helper.A8W8_fp8_dynamic(device=DEV, dtype=F16), "e4m3", F16),
    "A8W8_fp8_dynamic_16bit_scale": (lambda: helper.A8W8_dynamic(device=DEV, dtype=F16, fp8=torch.float8_e4m3fn, fp32_scale=False), "e4m3", F16),
}


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
    for attr in ("W_nbits", "group_size", "elements_per_sample", "data_contiguous", "meta_is_channelwise", "scaled_activations",
                 "W_group_mode", "channel_scale_mode"):
        assert getattr(a, attr) == getattr(b, attr), attr


@functools.lru_cache(maxsize=None)
def _layer_weight(dtype):
    W = planted_weights_rows(128, 512, dtype, seed=3)
    return torch.where(W.float().abs() > 64, torch.zeros_like(W), W)  # (the outputs below stay finite in fp16)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("name", list(PROCS))
def test_from_linear_equals_from_weights_of_the_restatement(name, bias):
    N, K = 128, 512
    make, fmt, dtype = PROCS[name]
    W = _layer_weight(dtype)
    codes, s = quantize_rows_spec(W, fmt, quant_utils.ROWS_SCALE_RULE)
    b = (torch.randn(N, generator=torch.Generator().manual_seed(1)) / 4).to(dtype).to(DEV) if bias else None
    lin = torch.nn.Linear(K, N, bias=bias, device=DEV, dtype=dtype)
    with torch.no_grad():
        lin.weight.copy_(W)
        if bias:
            lin.bias.copy_(b)
    layer = make().from_linear(lin, del_orig=False)
    assert lin.weight is not None
    want = make().from_weights(codes.view(FORMATS[fmt][1]).to(DEV), b, s.to(DEV))
    _same_layer(layer, want)
    assert layer.W_q.is_cuda and tuple(layer.W_q.shape) == (K, N) and layer.W_q.stride() == (1, K) and tuple(layer.scales.shape) == (1, N)
    assert torch.equal(layer.W_q.data.t().contiguous().view(torch.uint8).cpu(), codes)
    for M in (1, 16, 200):
        x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) / 10).to(dtype).to(DEV)
        y, y_want = layer(x), want(x)
        assert y.dtype == y_want.dtype and torch.isfinite(y).all() and torch.equal(y, y_want), f"M = {M}"
    code_f = codes.view(torch.int8).float() if fmt == "int8" else codes.view(FORMATS[fmt][1]).float()
    assert torch.equal(layer.dequantize(torch.float32).cpu(), code_f * layer.scales.data.cpu().float().view(N, 1))
    third = make().from_linear(lin)  # del_orig defaults to True: the float weight and bias are dropped
    assert lin.weight is None and lin.bias is None
    _same_layer(third, want)


def test_quantizer_dequantize_is_code_times_scale():
    W = weights(7, KW, "bf16")
    for fmt, (_, qdt, _, _) in FORMATS.items():
        wq = WeightQuantizerRows(qdt, dtype=torch.bfloat16, device=DEV, fp32_scale=False)
        q, s = wq.quantize(W.to(DEV))
        codes, want_s = quantize_rows_spec(W, fmt, quant_utils.ROWS_SCALE_RULE, torch.bfloat16)
        assert s.dtype == torch.bfloat16 and torch.equal(_bits(q).cpu(), codes) and torch.equal(_bits(s).cpu(), _bits(want_s))
        code_f = codes.view(torch.int8).float() if fmt == "int8" else codes.view(qdt).float()
        assert torch.equal(wq.dequantize(q, s, torch.float32).cpu(), code_f * want_s.float())
        assert torch.equal(wq.dequantize(q, s).cpu(), (code_f * want_s.float()).to(torch.bfloat16))


def test_cpu_weight_for_a_gpu_layer_and_a_strided_weight():
    W = _layer_weight(B16)
    codes, s = quantize_rows_spec(W, "int8", quant_utils.ROWS_SCALE_RULE)
    layer = helper.A8W8_int8_dynamic(device=DEV, dtype=B16).from_weights(W)  # moved in its own dtype, then the kernel
    assert layer.W_q.is_cuda and torch.equal(layer.W_q.data.t().contiguous().view(torch.uint8).cpu(), codes)
    assert torch.equal(_bits(layer.scales.data.view(-1, 1).cpu()), _bits(s))
    big = torch.zeros(128, 512 + 40, device=DEV, dtype=B16)
    big[:, 8:8 + 512].copy_(W)
    layer2 = helper.A16W8_INT8(device=DEV, dtype=B16).from_weights(big[:, 8:8 + 512])  # a row-strided view: read in place
    assert layer2.W_q.stride() == (1, 512) and torch.equal(layer2.W_q.data.t().contiguous().view(torch.uint8).cpu(), codes)


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
    helper.patch_model(net, DEV, helper.A8W8_int8_dynamic(dtype=torch.bfloat16))
    assert isinstance(net.body[0], GemLiteLinear) and isinstance(net.body[2], GemLiteLinear) and type(net.lm_head) is torch.nn.Linear
    for got, lin in zip((net.body[0], net.body[2]), copies):
        W = lin.weight.data.cpu()
        codes, s = quantize_rows_spec(W, "int8", quant_utils.ROWS_SCALE_RULE)
        _same_layer(got, helper.A8W8_int8_dynamic(device=DEV, dtype=torch.bfloat16).from_weights(codes.view(torch.int8).to(DEV), lin.bias.data, s.to(DEV)))
    assert net(torch.randn(3, 256, device=DEV, dtype=torch.bfloat16)).shape == (3, 32)


# ------------------------------------------------------------------------------------------------ G5: non-finite rows
NONFINITE_SHAPES = [(6, 200), (6, KW + 8), (4, KR + 8)]  # one per form


@pytest.mark.parametrize("dt", ["bf16", "fp32"])
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("N,K", NONFINITE_SHAPES, ids=[f"{n}x{k}" for n, k in NONFINITE_SHAPES])
def test_non_finite_rows_get_a_non_finite_scale(N, K, fmt, dt):
    W = planted_weights_rows(N, K, DTYPES[dt], seed=21).clone()
    W[1, K // 3], W[3, K - 1] = float("nan"), float("-inf")
    for rule in (0, 1):
        codes, s = quantize_rows_spec(W, fmt, rule)
        q, sc = run(W.to(DEV), fmt, rule)  # (the launch returned OK)
        torch.cuda.synchronize()
        q, sc = q.cpu(), sc.cpu()
        assert torch.isnan(sc[1]).all() and torch.isinf(sc[3]).all() and bool((sc[3] > 0).all())
        keep = torch.ones(N, dtype=torch.bool)
        keep[1] = keep[3] = False
        assert torch.isfinite(sc[keep]).all() and torch.equal(_bits(sc[keep]), _bits(s[keep])) and torch.equal(q[keep], codes[keep])


# ------------------------------------------------------------------------------------------------ G6: memory
@pytest.mark.parametrize("name", ["A8W8_int8_dynamic", "A16W8_FP8"])
def test_from_weights_allocates_the_layer_and_nothing_else(name):
    N, K = 512, 4096
    make = PROCS[name][0]
    small = torch.randn(32, 64, device=DEV, dtype=torch.bfloat16)
    make().from_weights(small)  # (the library and every lazy piece of torch are loaded before the measurement)
    W = (torch.randn(N, K, device=DEV) * 0.05).to(torch.bfloat16)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_stats()
    layer = make().from_weights(W)
    torch.cuda.synchronize()
    after = torch.cuda.memory_stats()
    # The bytes from_weights asked for.  (The allocator's own count, max_memory_allocated(), is that of the blocks it handed out: in a
    # process that has run other tests it may serve 2 MiB from a cached block up to 1 MiB larger without splitting it.)
    peak = after["requested_bytes.all.peak"] - before["requested_bytes.all.current"]
    blocks = after["allocated_bytes.all.peak"] - before["allocated_bytes.all.current"]
    print(f"{name}: peak {peak} bytes requested above the start (in blocks of {blocks}); N * K + 4 * N + 64 KiB = {N * K + 4 * N + 65536}; "
          f"the torch sequence needs >= {8 * N * K}")
    assert peak <= N * K + 4 * N + 65536
    assert tuple(layer.W_q.shape) == (K, N)


# ------------------------------------------------------------------------------------------------ G7: one launch, capturable
def _kernel_nodes(graph: torch.cuda.CUDAGraph) -> int:
    """Kernel nodes of a captured graph, asked of the HIP runtime this process already uses (hipGraphGetNodes / hipGraphNodeGetType)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    raw = C.c_void_p(int(graph.raw_cuda_graph()))
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    kinds = []
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        kinds.append(t.value)
    assert len(kinds) == sum(1 for t in kinds if t == 0), f"node types {kinds}"  # 0 = hipGraphNodeTypeKernel: nothing but kernels
    return len(kinds)


@pytest.mark.parametrize("N,K", [(7, KW), (3, KW + 8), (2, KR + 8)], ids=["wave", "resident", "reread"])
def test_quantizer_call_is_one_capturable_kernel(N, K):
    first, second = weights(N, K, "bf16"), planted_weights_rows(N, K, torch.bfloat16, seed=99)
    wq = WeightQuantizerRows(torch.float8_e4m3fn, device=DEV)
    buf = first.to(DEV)
    eager_q, eager_s = wq.quantize(buf)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        q, s = wq.quantize(buf)
    assert _kernel_nodes(graph) == 1
    buf.copy_(second.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    codes, want_s = quantize_rows_spec(second, "e4m3", quant_utils.ROWS_SCALE_RULE)
    assert torch.equal(_bits(q).cpu(), codes) and torch.equal(_bits(s).cpu(), _bits(want_s))
    codes1, want_s1 = quantize_rows_spec(first, "e4m3", quant_utils.ROWS_SCALE_RULE)
    assert torch.equal(_bits(eager_q).cpu(), codes1) and torch.equal(_bits(eager_s).cpu(), _bits(want_s1))
