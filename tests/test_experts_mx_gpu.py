"""MXFP4 experts on the MI355X (gemv_mxw4_experts_kernel): GemLiteExperts on A16W4_MXFP layers against the float64
product with the dequantised weights, under the bound of the block-scaled tests (tests/test_mx_gpu.py::_check, restated)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gemlite_amd import GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X, helper

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD, SENTINEL = 256, 7.25
REL_TOL = {torch.float16: 1.0e-3, torch.bfloat16: 4.0e-3}
E = 8
IDS = [[5, 2], [2, 7], [0, 5]]


def check(tag, y, ref, tdt):
    y = y.detach().float().cpu().numpy().astype(np.float64)
    ref = np.asarray(ref, np.float64).reshape(y.shape)
    err = np.abs(y - ref)
    scale = max(float(np.abs(ref).mean()), 1e-12)
    tol = REL_TOL[tdt]
    assert np.isfinite(y).all(), tag
    assert err.mean() / scale < tol, (tag, err.mean() / scale)
    viol = err > 10 * tol * scale + 4 * tol * np.abs(ref)
    assert int(viol.sum()) == 0, (tag, int(viol.sum()), float(err.max()), scale)


def make_layers(N, K, dtype, bias, n=E, seed=0, scale_lo=118, scale_hi=126):
    """A16W4_MXFP layers from random e2m1 codes and random e8m0 bytes in [scale_lo, scale_hi]."""
    g = torch.Generator().manual_seed(seed * 1000 + N + K)
    proc = helper.A16W4_MXFP(device=DEV, dtype=dtype)
    layers = []
    for _ in range(n):
        codes = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
        scales = torch.randint(scale_lo, scale_hi + 1, (N, K // 32), dtype=torch.uint8, generator=g)
        b = (torch.rand(N, generator=g) - 0.5).to(dtype) if bias else None
        layers.append(proc.from_weights(codes, scales, b))
    return layers


@functools.lru_cache(maxsize=None)
def experts_and_weights(N, K, dtype, bias, scale_lo=118, scale_hi=126):
    """-> (the experts, float64 [E, N, K] dequantised weights, float64 [E, N] bias or None); built once per shape."""
    ex = GemLiteExperts.from_layers(make_layers(N, K, dtype, bias, scale_lo=scale_lo, scale_hi=scale_hi), del_orig=True)
    W = torch.stack([ex.expert(e).dequantize(torch.float32).double() for e in range(E)])
    return ex, W, None if ex.bias is None else ex.bias.double()


def rand_x(shape, dtype, seed, amp=0.5):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * amp).to(dtype).to(DEV)


def reference(W, b, x, ids):
    """float64 [slots, N]: x row s / spx times expert ids[s]; an id outside [0, E) gives zeros."""
    flat = ids.reshape(-1).tolist()
    x2 = x.reshape(-1, x.shape[-1]).double()
    spx = len(flat) // x2.shape[0]
    rows = []
    for s, e in enumerate(flat):
        ok = 0 <= e < W.shape[0]
        rows.append((x2[s // spx] @ W[e].T + (0 if b is None else b[e])) if ok else torch.zeros(W.shape[1], dtype=torch.float64, device=DEV))
    return torch.stack(rows).cpu().numpy()


def launch_guarded(ex, x, ids):
    """The C call on an output window with guard bands on both sides -> out [slots, N]; asserts the bands are intact."""
    N, K = ex.out_features, ex.in_features
    rows, spx = X._split(x, ids, K)
    slots = ids.numel()
    buf = torch.full((GUARD + slots * N + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    out = buf[GUARD:GUARD + slots * N]
    e = X._call_args(x.contiguous().view(rows, K), ids.contiguous(), out.data_ptr(), ex.bias, ex.get_tensor_args(), ex.get_meta_args(), spx)
    rc = _hip.load().gemlite_hip_forward_experts(C.byref(e), _hip.current_stream_handle(x.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())
    return out.view(slots, N)


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64], ids=["i32", "i64"])
@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N,K", [(32, 256), (32, 768), (48, 2048), (32, 14336)])
def test_every_slot_matches_the_float64_product_with_its_experts_dequantised_weights(N, K, dtype, bias, ids_dtype):
    ex, W, b = experts_and_weights(N, K, dtype, bias)
    ids = torch.tensor(IDS, dtype=ids_dtype, device=DEV)
    for x in (rand_x((3, K), dtype, 1), rand_x((3, 2, K), dtype, 2)):  # shared per token; one row per slot
        out = launch_guarded(ex, x, ids)
        check((N, K, tuple(x.shape)), out, reference(W, b, x, ids), dtype)
        assert torch.equal(ex(x, ids), out.view(3, 2, N))  # the module: the same launch on its own output tensor
    x = rand_x((1, K), dtype, 3).expand(3, K).contiguous()
    out = ex(x, ids)
    assert torch.equal(out[0, 1], out[1, 0]) and torch.equal(out[0, 0], out[2, 1])  # the same expert on the same row: identical bits


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_scales_below_the_exponent_range_of_fp16_are_applied_exactly(dtype):
    N, K = 32, 768
    ex, W, b = experts_and_weights(N, K, dtype, True, 110, 130)
    ids = torch.tensor(IDS, dtype=torch.int64, device=DEV)
    x = rand_x((3, K), dtype, 4, amp=0.25)  # |y| stays near sqrt(K) * 6 * 2^3 * 0.25: far inside fp16
    ref = reference(W, b, x, ids)
    assert np.abs(ref).max() < 3.0e4
    check("scale range", ex(x, ids), ref, dtype)


def test_invalid_ids_give_zero_rows_and_their_neighbours_are_right():
    N, K, dtype = 32, 768, torch.float16
    ex, W, b = experts_and_weights(N, K, dtype, True)
    x = rand_x((3, K), dtype, 5)
    for ids in (torch.tensor([[-1, 2], [3, E], [1 << 32, 1]], dtype=torch.int64, device=DEV),
                torch.tensor([[-1, 2], [3, E], [E + 1, 1]], dtype=torch.int32, device=DEV)):
        out = launch_guarded(ex, x, ids)
        for s in (0, 3, 4):
            assert bool((out[s].view(torch.int16) == 0).all()), s
        check("neighbours", out, reference(W, b, x, ids), dtype)


def ordered(t):
    """The 16-bit patterns as integers that ascend with the value (one unit in the last place = 1)."""
    i = t.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("inter,K", [(16, 256), (32, 768)])
def test_the_glu_launch_is_silu_gate_times_up_of_the_plain_launch(inter, K, dtype, bias):
    gate, up = make_layers(inter, K, dtype, bias, seed=1), make_layers(inter, K, dtype, bias, seed=2)
    ex = GemLiteExperts.from_gate_up(gate, up)
    ids = torch.tensor([[5, 2], [-1, 7], [0, 5]], dtype=torch.int64, device=DEV)
    x = rand_x((3, K), dtype, 6, amp=0.05)
    y = ex(x, ids).double()
    ref = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(dtype)
    out = ex.forward_glu(x, ids)
    assert tuple(out.shape) == (3, 2, inter) and float(y.abs().max()) > 0.1
    assert int((ordered(out) - ordered(ref)).abs().max()) <= 1
    assert bool((out[1, 0].view(torch.int16) == 0).all())


def test_a_captured_launch_reads_the_ids_of_every_replay():
    N, K, dtype = 32, 768, torch.bfloat16
    ex, W, b = experts_and_weights(N, K, dtype, True)
    x = rand_x((3, K), dtype, 7)
    ids = torch.tensor(IDS, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ex(x, ids)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ex(x, ids)
    for other in (IDS, [[1, 1], [6, -1], [4, 3]], [[7, 0], [0, 7], [2, 2]]):
        ids.copy_(torch.tensor(other, dtype=torch.int32, device=DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ex(x, ids)), other


def test_the_mlp_on_mx_stacks_is_the_glu_launch_the_down_launch_and_the_combine_launch():
    """Hidden 256, intermediate 256 (the down launch needs K % 256 == 0, so 256 is the smallest intermediate size), 4 experts, top_k 2."""
    hidden, inter, n, dtype = 256, 256, 4, torch.float16
    mlp = GemLiteExpertsMLP.from_layers(make_layers(inter, hidden, dtype, True, n, 1), make_layers(inter, hidden, dtype, True, n, 2),
                                        make_layers(hidden, inter, dtype, True, n, 3))
    x = rand_x((3, hidden), dtype, 8, amp=0.05)
    ids = torch.tensor([[3, 1], [0, 2], [1, -1]], dtype=torch.int64, device=DEV)
    w = torch.rand((3, 2), generator=torch.Generator().manual_seed(9)).to(DEV)
    want = mlp.down.combine_batched(mlp.down(mlp.gate_up.forward_glu(x, ids), ids), ids, w)
    got = mlp(x, ids, w)
    assert tuple(got.shape) == (3, hidden) and torch.equal(got, want) and float(got.float().abs().max()) > 0
    for refused in (lambda: mlp.forward_batched(x, ids, w), lambda: mlp.forward_batched_fused(x, ids, w),
                    lambda: mlp.down.forward_combine(x, ids, w), lambda: mlp.down.route(ids)):
        with pytest.raises(NotImplementedError, match="MXFP4"):
            refused()
