"""Bias inside the launch on the GPU: the biased forms of gemv_w4_decode3_kernel (single and grouped) and gemm_w{4,2}_rows_kernel.
The reference of every comparison is this library's own unbiased launch followed by torch's `out += bias` (core.FUSE_BIAS = False), and
every comparison is BIT-EXACT: the kernels round the accumulator to the 16-bit type, add the bias in fp32 and round again, as the two
launches do."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from oracle import gemlite_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F16, B16 = torch.float16, torch.bfloat16
# nch_total = 2 (14 idle waves) | 1 chunk per wave | 2 per wave (the planner gives K = 8192 to another GEMV kernel today: skipped, loudly) |
# 43 chunks: 2 .. 3 per wave, the decode3 shape that does cover "more than one chunk" | 256 tiles
DECODE_SHAPES = [(256, 512), (512, 4096), (512, 8192), (512, 11008), (4096, 4096)]


@pytest.fixture(autouse=True)
def _switch_back():
    yield
    core.FUSE_BIAS = True
    core.TUNING_OVERRIDE = None


def _layer(N, K, tdt, seed, nbits=4, gs=128, mode="fma", bias=True, arrays=None):
    """mode: 'fma' = W_group_mode 4 | 'sub' = W_group_mode 3 | 'zscalar' = a scalar zero point"""
    W_q, scales, zeros = arrays if arrays is not None else O.gen_data(N, K, nbits, gs, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(nbits, gs, K, N, code, code)
    z = 2 ** (nbits - 1) if mode == "zscalar" else torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV)
    b = (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.5).to(tdt).to(DEV) if bias is True else bias
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV), z, b, fma_mode=(mode == "fma"))
    return lin


def _x(M, K, tdt, seed):
    return torch.from_numpy(O.gen_x(M, K, seed=seed)).to(tdt).to(DEV)


def _names(lin, x):
    """(kernel of the unbiased launch, kernel of the launch with the layer's bias) as the library plans them for layer(x)"""
    W_q, scales, zeros = lin.get_tensor_args()
    a = core._call_args(x, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, 0x1000, (W_q.shape[1], 1))
    ext = _hip.forward_ext(lin.bias.data_ptr(), gemlite_amd.dtypes.TORCH_TO_DTYPE[lin.bias.dtype].value)
    lib = _hip.load()
    return lib.gemlite_hip_kernel_name(C.byref(a)).decode(), lib.gemlite_hip_kernel_name_ex(C.byref(a), C.byref(ext)).decode()


def _python_path(lin, x, fuse):
    core.FUSE_BIAS = fuse
    try:
        y = core._forward_impl(x, lin.bias, lin.get_tensor_args(), lin.get_meta_args(), -1).clone()
    finally:
        core.FUSE_BIAS = True
    torch.cuda.synchronize()
    return y


def _need(name, prefix):
    if not name.startswith(prefix):
        pytest.skip(f"PLANNER ROUTES ELSEWHERE: {name} instead of {prefix}: this case checks nothing")


# ---- 1. M = 1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fma", "sub", "zscalar"])
@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N,K", DECODE_SHAPES)
def test_decode_fused_equals_matmul_then_add(N, K, tdt, mode):
    lin = _layer(N, K, tdt, seed=N + K, mode=mode)
    x = _x(1, K, tdt, seed=3)
    plain, biased = _names(lin, x)
    _need(plain, "gemv_w4_decode3_kernel<")
    assert biased == "gemv_w4_decode3_kernel<tile16,16w,bias>"
    want = _python_path(lin, x, False)
    got = _python_path(lin, x, True)
    assert torch.equal(got, want)
    assert not torch.equal(got, want - lin.bias), "the bias is in"


# ---- 2. special values and the double rounding ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
def test_special_bias_values_and_both_roundings(tdt):
    """x = (1, t, 0, ...), every column's first two codes 1, scale 1, zero 0: acc = 1 + t, with t HALF an ulp of 1 in the 16-bit type — a
    tie, rounded to 1.  bias = t / 2 in the tie columns: double rounding gives 1, one rounding of acc + bias gives 1 + ulp."""
    N, K = 256, 512
    t = 2.0 ** -11 if tdt == F16 else 2.0 ** -8
    W_q, scales, zeros = O.gen_data(N, K, 4, 128, seed=5, np_float=np.float16)
    W_q[:, :2] = 1
    scales[:] = 1
    zeros[:] = 0
    fin = torch.finfo(tdt)
    special = [0.0, -0.0, float("inf"), float("-inf"), float("nan"), fin.max, -fin.max, 2.0 ** -24, -(2.0 ** -24), 3 * 2.0 ** -25, 1.0 - 2.0 ** -24]
    bias = torch.full((N,), t / 2, dtype=torch.float32)
    bias[:len(special)] = torch.tensor(special)
    bias[N // 2:] = torch.randn(N // 2, generator=torch.Generator().manual_seed(1))
    bias = bias.to(tdt).to(DEV)
    lin = _layer(N, K, tdt, seed=5, bias=bias, arrays=(W_q, scales, zeros))
    x = torch.zeros(1, K, dtype=tdt, device=DEV)
    x[0, 0], x[0, 1] = 1.0, t
    # on the CPU, in float64: these inputs DO tell the two roundings apart
    acc = O.forward_packed(O.to_f64(x), lin.W_q.data.cpu().numpy(), O.to_f64(lin.scales.data), O.to_f64(lin.zeros.data), W_nbits=4,
                           group_size=128, W_group_mode=lin.W_group_mode)
    acc = torch.from_numpy(acc)
    b64 = bias.cpu().double()
    twice = (acc.to(tdt).float() + bias.cpu().float()).to(tdt)
    once = (acc + b64).to(tdt)
    differ = (twice != once) & ~torch.isnan(twice)
    assert differ.any(), "no column where one rounding of acc + bias differs from two: the inputs check nothing"
    plain, biased = _names(lin, x)
    _need(plain, "gemv_w4_decode3_kernel<")
    want = _python_path(lin, x, False)
    got = _python_path(lin, x, True)
    nan = torch.isnan(want)
    assert nan[0, 4] and int(nan.sum()) == 1 and torch.equal(torch.isnan(got), nan)
    assert torch.equal(got[~nan], want[~nan])
    assert torch.equal(got.cpu()[differ], twice[differ]) and not torch.equal(got.cpu()[differ], once[differ])
    assert torch.isinf(got[0, 2]) and torch.isinf(got[0, 3]) and got[0, 2] > 0 > got[0, 3]


# ---- 3. rows kernel -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbits", [4, 2])
@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N,K", [(272, 512), (272, 4096), (1024, 512), (1024, 4096)])
def test_rows_fused_equals_matmul_then_add(N, K, tdt, nbits):
    lin = _layer(N, K, tdt, seed=N + K + nbits, nbits=nbits)
    for M in (2, 16, 17, 64):
        x = _x(M, K, tdt, seed=M)
        prefix = f"gemm_w{nbits}_rows_kernel<"
        if not _names(lin, x)[0].startswith(prefix):
            core.TUNING_OVERRIDE = (9, 0, 0, 0)  # GEMLITE_T0_ROWS_KERNEL: 2 .. 4 rows default to the matrix-core GEMV
        plain, biased = _names(lin, x)
        _need(plain, prefix)
        assert biased == plain[:-1] + ",bias>"
        want = _python_path(lin, x, False)
        got = _python_path(lin, x, True)
        core.TUNING_OVERRIDE = None
        assert got.shape == (M, N) and torch.equal(got, want), f"M={M}"  # every row, the last partial row block included
        assert not torch.equal(got, want - lin.bias)


# ---- 4. capture -----------------------------------------------------------------------------------------------------------------------
def _stats():
    seen, joined = C.c_uint64(0), C.c_uint64(0)
    _hip.load().gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    return seen.value, joined.value


def _gmax():
    return _hip.load().gemlite_hip_capture_group_max()


def _capture(step):
    """Warm `step` up on a side stream, capture it there: (graph, what step() returned, decode launches seen, launches joined, kernel nodes)"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    seen0, joined0 = _stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        outs = step()
    seen1, joined1 = _stats()
    return g, outs, seen1 - seen0, joined1 - joined0


def _eager_unfused(lins, x):
    core.FUSE_BIAS = False
    try:
        ys = [lin(x).clone() for lin in lins]
    finally:
        core.FUSE_BIAS = True
    torch.cuda.synchronize()
    return ys


def _replay_and_compare(g, outs, want):
    for o in outs:
        o.zero_()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i}"


@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N", [512, 4096], ids=["grid_y>1", "grid_y=1"])
def test_four_independent_biased_layers_are_one_kernel_node(N, tdt):
    """Without the feature each layer is a matmul node and an add node (8 nodes) and nothing joins."""
    lins = [_layer(N, 4096, tdt, seed=10 + i) for i in range(4)]
    x = _x(1, 4096, tdt, seed=3)
    _need(_names(lins[0], x)[0], "gemv_w4_decode3_kernel<")
    want = _eager_unfused(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 4 and joined == min(4, _gmax()) - 1
    _replay_and_compare(g, outs, want)


def test_more_biased_layers_than_a_group_holds_split_like_unbiased_ones():
    n = _gmax() + 3
    lins = [_layer(512, 4096, F16, seed=30 + i) for i in range(n)]
    x = _x(1, 4096, F16, seed=4)
    want = _eager_unfused(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == n and joined == _gmax() + 1  # (GMAX - 1) + 2, the unbiased split
    _replay_and_compare(g, outs, want)


def test_a_layer_whose_bias_is_the_previous_output_does_not_join():
    lin1 = _layer(512, 4096, F16, seed=60)
    lin2 = _layer(512, 4096, F16, seed=61, bias=None)
    x = _x(1, 4096, F16, seed=7)

    def step():
        y1 = lin1(x)
        y2 = core._forward_impl(x, y1.view(-1), lin2.get_tensor_args(), lin2.get_meta_args(), -1)  # dependent THROUGH the bias
        return y1, y2

    core.FUSE_BIAS = False
    y1w, y2w = (y.clone() for y in step())
    core.FUSE_BIAS = True
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(step)
    assert seen == 2 and joined == 0
    _replay_and_compare(g, outs, [y1w, y2w])


def test_biased_unbiased_biased_neighbours_are_three_nodes():
    lins = [_layer(512, 4096, F16, seed=70), _layer(512, 4096, F16, seed=71, bias=None), _layer(512, 4096, F16, seed=72)]
    x = _x(1, 4096, F16, seed=8)
    want = _eager_unfused(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 3 and joined == 0
    _replay_and_compare(g, outs, want)


# ---- 5. guard band --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 256, 512), (1, 512, 4096), (17, 272, 512), (64, 1024, 512)])
def test_nothing_outside_the_output_window_is_written_and_the_bias_is_left_alone(M, N, K):
    lin = _layer(N, K, F16, seed=80 + M)
    x = _x(M, K, F16, seed=9)
    rs = N + 128
    off = 3 * rs + 64
    buf = torch.full(((3 + M + 64) * rs * 2,), 0xFF, dtype=torch.uint8, device=DEV).view(F16)
    out = buf.as_strided((M, N), (rs, 1), off)
    bias_before = lin.bias.clone()
    W_q, scales, zeros = lin.get_tensor_args()
    a = core._call_args(x, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, out.data_ptr(), (rs, 1))
    ext = _hip.forward_ext(lin.bias.data_ptr(), 1)
    lib = _hip.load()
    assert lib.gemlite_hip_bias_fused(C.byref(a), C.byref(ext)) == 1
    stream = _hip.current_stream_handle(x.device)
    ws = _hip.workspace(x.device, stream, 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    assert lib.gemlite_hip_forward_ex(C.byref(a), C.byref(ext), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _python_path(lin, x, False))
    mask = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)
    mask.as_strided((M, N), (rs, 1), off).fill_(False)
    assert bool((buf.view(torch.int16)[mask] == -1).all()), "a store outside [M, N]"
    assert torch.equal(lin.bias, bias_before)


def test_a_bias_the_library_does_not_add_is_reported_not_refused():
    lin = _layer(512, 1024, F16, seed=85)
    x = _x(1, 1024, F16, seed=10)
    bias32 = lin.bias.float()
    out = torch.empty(1, 512, dtype=F16, device=DEV)
    W_q, scales, zeros = lin.get_tensor_args()
    a = core._call_args(x, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, out.data_ptr(), (512, 1))
    ext = _hip.forward_ext(bias32.data_ptr(), 0)
    stream = _hip.current_stream_handle(x.device)
    ws = _hip.workspace(x.device, stream, 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    assert _hip.load().gemlite_hip_forward_ex(C.byref(a), C.byref(ext), stream) == _hip.BIAS_NOT_ADDED
    torch.cuda.synchronize()
    assert torch.equal(out + lin.bias, _python_path(lin, x, False))


# ---- 6. the C++ path against the Python path ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 16, 128])
def test_fast_path_and_python_path_agree_bit_for_bit(M):
    """M = 128: a tile kernel, the library answers "add it yourself" and the C++ path does."""
    if core._FAST is None:
        pytest.skip("gemlite_amd/_fast.so not built")
    lin = _layer(512, 4096, F16, seed=90 + M)
    x = _x(M, 4096, F16, seed=11)
    want = _python_path(lin, x, False)
    lin(x)                                              # the slow call installs the handle
    assert lin.__dict__.get("_fast") is not None
    seen_fast = []
    orig = core._FAST

    def spy(*args):
        y = orig.forward(*args)
        seen_fast.append(isinstance(y, torch.Tensor))
        return y

    try:
        core._FAST = type("SpyFast", (), {"forward": staticmethod(spy), "set_tuning": staticmethod(orig.set_tuning),
                                          "make": staticmethod(orig.make), "workspace": staticmethod(orig.workspace)})
        y_fast = lin(x)
        core.FUSE_BIAS = False
        y_fast_unfused = lin(x)
    finally:
        core._FAST = orig
        core.FUSE_BIAS = True
    torch.cuda.synchronize()
    assert sum(seen_fast) == 2 and seen_fast[-1], "both calls ran the C++ path (a False in between: the tuning of this M was looked up first)"
    assert torch.equal(y_fast, want) and torch.equal(y_fast_unfused, want) and torch.equal(_python_path(lin, x, True), want)
