"""gemlite_amd.GemLiteExperts / gemlite_hip_forward_experts on the MI355X: every valid slot is bit-identical to its expert's own decode
launch, invalid ids give zero rows and touch nothing, the ids are read when the graph REPLAYS, expert strides are 64-bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemlite_amd import DType, GemLiteExperts, GemLiteLinear, _hip, core, experts as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 256, 7.25
TUNING = (2, 1, 0, 0)  # the single-layer decode3 kernel at every shape below (asserted)
SHAPES = {"a": (48, 768), "b": (256, 4352), "c": (16, 256), "d": (768, 2048)}
E = 8


def make_experts(N, K, gs=128, dtype=torch.float16, zeros="tensor", bias=False, n=E, seed=0):
    g = torch.Generator().manual_seed(seed * 1000 + N + K + gs)
    dt = DType.FP16 if dtype == torch.float16 else DType.BF16
    layers = []
    for _ in range(n):
        W_q = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
        scales = (torch.rand(N * K // gs, 1, generator=g) * 0.02 + 0.005).to(dtype)
        z = (torch.rand(N * K // gs, 1, generator=g) * 4 + 6).to(dtype).to(DEV) if zeros == "tensor" else 8
        b = (torch.rand(N, generator=g) - 0.5).to(dtype).to(DEV) if bias else None
        layers.append(GemLiteLinear(4, gs, K, N, dt, dt).pack(W_q.to(DEV), scales.to(DEV), z, b))
    return GemLiteExperts.from_layers(layers, del_orig=True)


def rand_x(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5).to(dtype).to(DEV)


def oracle_slot(ex, e, x_row):
    """Expert e's own single-layer decode3 launch on one x row (+ the bias as `out += bias`)."""
    lin = ex.expert(e)
    x2 = x_row.reshape(1, -1)
    a = core._call_args(x2, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, TUNING, False, 0x1000, (lin.W_q.shape[1], 1))
    name = _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode()
    assert name.startswith("gemv_w4_decode3_kernel"), name
    y = core._hip_matmul(x2, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, TUNING)
    if lin.bias is not None:
        y += lin.bias
    return y[0]


def launch_guarded(ex, x, ids):
    """The C call on an output window with guard bands on both sides -> (out [slots, N], the whole buffer)."""
    N, K = ex.out_features, ex.in_features
    rows, spx = X._split(x, ids, K)
    slots = ids.numel()
    buf = torch.full((GUARD + slots * N + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    out = buf[GUARD:GUARD + slots * N]
    e = X._call_args(x.contiguous().view(rows, K), ids.contiguous(), out.data_ptr(), ex.bias, ex.get_tensor_args(), ex.get_meta_args(), spx)
    rc = _hip.load().gemlite_hip_forward_experts(C.byref(e), _hip.current_stream_handle(x.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    return out.view(slots, N), buf


def guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def check_slots(ex, x, ids, out):
    """Every valid slot equals its expert's own launch bit for bit; every invalid one is exactly zero."""
    K = ex.in_features
    rows, spx = X._split(x, ids, K)
    x2, flat = x.contiguous().view(rows, K), ids.reshape(-1).tolist()
    for s, e in enumerate(flat):
        if 0 <= e < ex.num_experts:
            want = oracle_slot(ex, e, x2[s // spx])
            assert torch.equal(out[s], want), (s, e, float((out[s].float() - want.float()).abs().max()))
        else:
            assert bool((out[s].view(torch.int16) == 0).all()), (s, e)


@pytest.mark.parametrize("case", list(SHAPES))
@pytest.mark.parametrize("dtype,gs,zeros,bias,ids_dtype", [
    (torch.float16, 128, "tensor", False, torch.int64),
    (torch.bfloat16, 32, "tensor", True, torch.int32),
    (torch.float16, 32, "int", True, torch.int64),
    (torch.bfloat16, 128, "int", False, torch.int32),
])
def test_every_slot_is_bit_identical_to_its_experts_own_decode_launch(case, dtype, gs, zeros, bias, ids_dtype):
    N, K = SHAPES[case]
    ex = make_experts(N, K, gs, dtype, zeros, bias)
    # shared x: 3 tokens, top_k = 2, ids with repeats
    ids = torch.tensor([[5, 2], [2, 7], [0, 5]], dtype=ids_dtype, device=DEV)
    x = rand_x((3, K), dtype, 1)
    out, buf = launch_guarded(ex, x, ids)
    check_slots(ex, x, ids, out)
    assert guards_intact(buf)
    assert torch.equal(ex(x, ids), out.view(3, 2, N))  # the module: same launch, its own output tensor
    # one row per slot (the down projection)
    xs = rand_x((3, 2, K), dtype, 2)
    out, buf = launch_guarded(ex, xs, ids)
    check_slots(ex, xs, ids, out)
    assert guards_intact(buf)
    assert torch.equal(ex(xs, ids), out.view(3, 2, N))
    # T = 1
    one = torch.tensor([[3]], dtype=ids_dtype, device=DEV)
    out, buf = launch_guarded(ex, x[:1], one)
    check_slots(ex, x[:1], one, out)
    assert guards_intact(buf)


def test_arithmetic_against_float64_where_no_single_layer_decode3_plan_exists():
    """N = 32, K = 14336 (56 chunks: four per wave; the single-layer planner stops at two).  Mean relative error against float64
    x @ dequantize(fp32).T below 4e-4 plus the output quantum — the project's one bound for decode kernels."""
    N, K = 32, 14336
    ex = make_experts(N, K, 128, torch.float16, "tensor", False, n=4)
    ids = torch.tensor([[1, 3], [0, 1]], dtype=torch.int64, device=DEV)
    x = rand_x((2, K), torch.float16, 3)
    out, buf = launch_guarded(ex, x, ids)
    assert guards_intact(buf)
    for s, e in enumerate(ids.reshape(-1).tolist()):
        W = ex.expert(e).dequantize(torch.float32).double().cpu().numpy()
        y_ref = x[s // 2].double().cpu().numpy() @ W.T
        rel = float(np.abs(out[s].double().cpu().numpy() - y_ref).mean() / np.abs(y_ref).mean())
        print(f"experts K=14336 slot {s} expert {e}: rel={rel:.3e}")
        assert rel < 4e-4 + 2.0 ** -25 / np.abs(y_ref).mean(), (s, e, rel)


def test_a_captured_graph_reads_the_ids_when_it_replays():
    N, K = SHAPES["d"]
    ex = make_experts(N, K, bias=True)
    x = rand_x((3, K), torch.float16, 4)
    ids = torch.tensor([[0, 1], [2, 3], [4, 5]], dtype=torch.int64, device=DEV)
    ex(x, ids)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ex(x, ids)
    for i, new_ids in enumerate(([[7, 7], [1, 0], [3, 6]], [[2, 5], [5, 2], [0, 0]], [[6, 4], [4, 1], [7, 3]])):
        ids.copy_(torch.tensor(new_ids, dtype=torch.int64, device=DEV))
        x.copy_(rand_x((3, K), torch.float16, 10 + i))
        graph.replay()
        torch.cuda.synchronize()
        check_slots(ex, x, ids, y.view(6, N))


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
def test_invalid_ids_give_zero_rows_and_touch_nothing_else(ids_dtype):
    N, K = SHAPES["a"]
    ex = make_experts(N, K, bias=True)
    bad = [-1, E, 2 ** 31 - 1] + ([(1 << 32) + 1, -(1 << 40)] if ids_dtype == torch.int64 else [-(2 ** 31)])
    flat = [4, bad[0], bad[1], 0, bad[2], 7] + bad[3:] + [1]
    if len(flat) % 2:
        flat.append(bad[0])
    ids = torch.tensor(flat, dtype=ids_dtype, device=DEV).view(-1, 2)
    x = rand_x((ids.shape[0], K), torch.float16, 5)
    out, buf = launch_guarded(ex, x, ids)
    check_slots(ex, x, ids, out)
    assert guards_intact(buf)


def test_expert_strides_are_64_bit():
    """Through the C ABI: two experts 4 GiB apart inside one buffer; expert 1 lives at the far offset."""
    N, K = SHAPES["a"]
    ex = make_experts(N, K, n=2)
    words = (K // 8) * N
    big = torch.empty((1 << 30) + words, dtype=torch.int32, device=DEV)  # 4 GiB + one expert
    big[:words].copy_(ex.W_q[0].reshape(-1))
    big[1 << 30:].copy_(ex.W_q[1].reshape(-1))
    ids = torch.tensor([[1, 0], [1, 1]], dtype=torch.int64, device=DEV)
    x = rand_x((2, K), torch.float16, 6)
    buf = torch.full((GUARD + 4 * N + GUARD,), SENTINEL, dtype=torch.float16, device=DEV)
    out = buf[GUARD:GUARD + 4 * N]
    e = X._call_args(x, ids, out.data_ptr(), None, ex.get_tensor_args(), ex.get_meta_args(), 2)
    e.layer.w_q = big.data_ptr()
    e.stride_expert_w = 1 << 32
    assert _hip.load().gemlite_hip_forward_experts(C.byref(e), _hip.current_stream_handle(x.device)) == 0
    torch.cuda.synchronize()
    check_slots(ex, x, ids, out.view(4, N))
    assert guards_intact(buf)


def test_an_experts_launch_between_two_layers_keeps_them_from_joining_one_group():
    from oracle import gemlite_oracle as O
    lib = _hip.load()
    lins = []
    for seed in (1, 2):
        W_q, scales, zeros = O.gen_data(4096, 4096, 4, 128, seed=seed)
        lins.append(GemLiteLinear(4, 128, 4096, 4096, DType.FP16, DType.FP16).pack(
            torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales).to(DEV), torch.from_numpy(zeros).to(DEV)))
    ex = make_experts(48, 4096, n=4)
    x = rand_x((1, 4096), torch.float16, 7)
    ids = torch.tensor([[2, 0]], dtype=torch.int64, device=DEV)
    want = [lins[0](x), ex(x, ids), lins[1](x)]
    torch.cuda.synchronize()

    def stats():
        s, j = C.c_uint64(0), C.c_uint64(0)
        lib.gemlite_hip_capture_group_stats(C.byref(s), C.byref(j))
        return s.value, j.value

    grouping = lib.gemlite_hip_capture_group_max() >= 2
    s0, j0 = stats()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        got = [lins[0](x), ex(x, ids), lins[1](x)]
    s1, j1 = stats()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        ctl = [lins[0](x), lins[1](x)]
    s2, j2 = stats()
    g1.replay()
    g2.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(ctl[0], want[0]) and torch.equal(ctl[1], want[2])
    if grouping:
        assert (s1 - s0, j1 - j0) == (2, 0), "the experts launch lies between the two layers: they must not join"
        assert (s2 - s1, j2 - j1) == (2, 1), "without it they join as before"
    else:
        assert (s2 - s0, j2 - j0) == (0, 0)


def test_opcheck_and_torch_compile_fullgraph():
    N, K = SHAPES["a"]
    ex = make_experts(N, K, bias=True)
    x = rand_x((3, K), torch.float16, 8)
    ids = torch.tensor([[5, 2], [2, 7], [0, 5]], dtype=torch.int64, device=DEV)
    torch.library.opcheck(torch.ops.gemlite.forward_experts.default, (x, ids, ex.bias, ex.get_tensor_args(), ex.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))

    class Block(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.experts = ex

        def forward(self, x, ids, w):
            return (self.experts(x, ids) * w.unsqueeze(-1)).sum(-2)

    block = Block()
    w = torch.rand(3, 2, device=DEV).to(torch.float16)
    eager = block(x, ids, w)
    compiled = torch.compile(block, fullgraph=True)(x, ids, w)
    torch.cuda.synchronize()
    assert torch.allclose(compiled.float(), eager.float(), rtol=2e-3, atol=2e-3)
    assert torch.equal(torch.compile(ex, fullgraph=True)(x, ids), ex(x, ids))
