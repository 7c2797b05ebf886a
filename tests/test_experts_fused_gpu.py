"""gemlite_hip_forward_experts_fused, GemLiteExperts.forward_glu / forward_combine and GemLiteExpertsMLP on the MI355X.  The reference is
always the unfused launch ``ex(x, ids)`` (tests/test_experts_gpu.py: every slot bit-identical to its expert's own decode launch) plus
float64 arithmetic on the host; outputs are written into a window with sentinel bands on both sides.

Bounds.  GLU: |out - ref| <= 1 ulp of the output type at |ref| — the fp32 evaluation of silu(g) * u is a few 2^-24 relative, far below
the output's half-ulp (2^-11 fp16, 2^-8 bf16), so it can turn a rounding at a near-tie and never move a value by two.  COMBINE:
|out - ref| <= 1 ulp_out(|ref|) + top_k * 2^-23 * sum_k |w_k y_k| — the final rounding plus the fp32 accumulation of top_k rounded products."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gemlite_amd import GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X
from tests.test_experts_gpu import DEV, GUARD, SENTINEL, E, guards_intact, make_experts, rand_x

pytestmark = pytest.mark.gpu
GLU, COMBINE = _hip.EXPERTS_GLU, _hip.EXPERTS_COMBINE
ROWS = [  # (dtype, group, zeros, bias, ids dtype): the rows of test_experts_gpu.py
    (torch.float16, 128, "tensor", False, torch.int64),
    (torch.bfloat16, 32, "tensor", True, torch.int32),
    (torch.float16, 32, "int", True, torch.int64),
    (torch.bfloat16, 128, "int", False, torch.int32),
]
GLU_SHAPES = [(32, 256), (96, 768), (512, 4352), (1536, 2048)]
COMBINE_SHAPES = [(16, 256), (48, 768), (256, 4352), (2048, 768)]


@functools.lru_cache(maxsize=None)
def experts(N, K, row, n=E):
    dtype, gs, zeros, bias, _ = ROWS[row]
    return make_experts(N, K, gs, dtype, zeros, bias, n=n)


def launch_fused(ex, epilogue, x, ids, w=None):
    """The C call on an output window with guard bands on both sides -> (out [rows, width], the whole buffer)."""
    N, K = ex.out_features, ex.in_features
    rows_x, spx = X._split(x, ids, K)
    top_k = ids.shape[-1]
    rows, width = (ids.numel(), N // 2) if epilogue == GLU else (ids.numel() // top_k, N)
    buf = torch.full((GUARD + rows * width + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    out = buf[GUARD:GUARD + rows * width]
    e = X._call_args(x.contiguous().view(rows_x, K), ids.contiguous(), out.data_ptr(), ex.bias, ex.get_tensor_args(), ex.get_meta_args(), spx)
    e.stride_out_slot = width
    if epilogue == GLU:
        f = X._fused_args(e, GLU)
    else:
        w = w.contiguous()
        f = X._fused_args(e, COMBINE, w.data_ptr(), X.TORCH_TO_DTYPE[w.dtype].value, top_k)
    rc = _hip.load().gemlite_hip_forward_experts_fused(C.byref(f), _hip.current_stream_handle(x.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    return out.view(rows, width), buf


def ulp(ref, dtype):
    """The spacing of `dtype` at |ref| (float64 arrays); the subnormal spacing below the smallest normal."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    a = np.abs(ref)
    ex = np.floor(np.log2(np.maximum(a, 2.0 ** emin)))
    return 2.0 ** (ex - mant)


def f64(t):
    return t.double().cpu().numpy()


def glu_ref(y):
    """silu(gate) * up in float64 on the unfused launch's rounded outputs y [..., 2 I]."""
    y = f64(y)
    half = y.shape[-1] // 2
    g, u = y[..., :half], y[..., half:]
    return g / (1.0 + np.exp(-g)) * u


def check_glu(out, y, dtype, what):
    ref = glu_ref(y).reshape(out.shape)
    got = f64(out)
    assert np.isfinite(got).all(), what
    err, tol = np.abs(got - ref), ulp(ref, dtype)
    worst = float((err / tol).max())
    print(f"glu {what}: worst |out - ref| = {worst:.3f} ulp")
    assert (err <= tol).all(), (what, worst)


def check_combine(out, y, w, dtype, what):
    """y [T, top_k, N] from the unfused launch, w [T, top_k]"""
    prod = f64(w)[..., None] * f64(y)
    ref, mag = prod.sum(-2), np.abs(prod).sum(-2)
    got = f64(out)
    assert np.isfinite(got).all(), what
    err, tol = np.abs(got - ref), ulp(ref, dtype) + y.shape[-2] * 2.0 ** -23 * mag
    worst = float((err / tol).max())
    print(f"combine {what}: worst |out - ref| / bound = {worst:.3f}")
    assert (err <= tol).all(), (what, worst)


def routing(T, top_k, dtype, seed, signs=False):
    """(ids [T, top_k] with repeats allowed, weights [T, top_k] positive and normalised, or of mixed signs)"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(0, E, (T, top_k), generator=g)
    w = torch.rand(T, top_k, generator=g) + 0.05
    w = w / w.sum(-1, keepdim=True)
    if signs:
        w = w * (torch.randint(0, 2, (T, top_k), generator=g) * 2 - 1) * 1.5
    return ids, w.to(dtype).to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------------- GLU
@pytest.mark.parametrize("shape", GLU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_glu_is_silu_gate_times_up_of_the_unfused_launch(shape, row):
    N, K = shape
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    ids = torch.tensor([[5, 2], [2, 7], [0, 5]], dtype=ids_dtype, device=DEV)
    for what, x, i in (("shared x", rand_x((3, K), dtype, 1), ids), ("x per slot", rand_x((3, 2, K), dtype, 2), ids),
                       ("T = 1", rand_x((1, K), dtype, 3), torch.tensor([[3]], dtype=ids_dtype, device=DEV))):
        out, buf = launch_fused(ex, GLU, x, i)
        assert guards_intact(buf), what
        check_glu(out, ex(x, i), dtype, f"{N}x{K} row {row} {what}")
        assert torch.equal(ex.forward_glu(x, i), out.view(tuple(i.shape) + (N // 2,))), what  # the module: same launch, its own output


@pytest.mark.parametrize("row", [0, 1])
def test_glu_stays_finite_where_the_gate_reaches_plus_and_minus_60(row):
    N, K = 96, 768
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    ids = torch.tensor([[5, 2], [2, 7]], dtype=ids_dtype, device=DEV)
    x = rand_x((2, K), dtype, 4)
    gate = ex(x[1:], ids[1:])[0, 0, :N // 2].float()
    x[1] *= float(64.0 / min(gate.max(), -gate.min()))  # token 1's first expert: both ends of its gate values beyond 60
    y = ex(x, ids)
    gate = y[1, 0, :N // 2].float()
    assert float(gate.max()) >= 60 and float(gate.min()) <= -60 and bool(torch.isfinite(y).all())
    out, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    check_glu(out, y, dtype, f"gate beyond +-60 row {row}")


# ------------------------------------------------------------------------------------------------------------------------------ COMBINE
@pytest.mark.parametrize("shape", COMBINE_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("top_k", [1, 2, 3, 8, 10, 16])
def test_combine_is_the_weighted_sum_of_the_unfused_launch(shape, top_k):
    N, K = shape
    row = (COMBINE_SHAPES.index(shape) + top_k) % len(ROWS)
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    for T in (1, 3):
        for wdt, signs in ((torch.float32, False), (dtype, False), (torch.float32, True)):
            ids, w = routing(T, top_k, wdt, 100 * top_k + T, signs)
            ids = ids.to(ids_dtype).to(DEV)
            x = rand_x((T, top_k, K), dtype, 5 + T)  # one row per slot, as the down projection takes it
            what = f"{N}x{K} top_k {top_k} T {T} weights {wdt} signs {signs}"
            out, buf = launch_fused(ex, COMBINE, x, ids, w)
            assert guards_intact(buf), what
            check_combine(out, ex(x, ids), w, dtype, what)
            assert torch.equal(ex.forward_combine(x, ids, w), out), what
    # one x row per token
    ids, w = routing(3, top_k, torch.float32, 7)
    ids, x = ids.to(ids_dtype).to(DEV), rand_x((3, K), dtype, 8)
    out, buf = launch_fused(ex, COMBINE, x, ids, w)
    assert guards_intact(buf)
    check_combine(out, ex(x, ids), w, dtype, f"{N}x{K} top_k {top_k} shared x")


@pytest.mark.parametrize("top_k", [1, 3, 8, 16])
@pytest.mark.parametrize("row", [1, 2])
def test_a_one_hot_weight_gives_that_members_unfused_output_bit_for_bit(top_k, row):
    """Every member of a block is rounded exactly as its own slot of the unfused launch: 0.f + 1 * y == y, the others add 0 * y_k."""
    N, K = 256, 4352
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    ids, _ = routing(3, top_k, torch.float32, 11 + top_k)
    ids, x = ids.to(ids_dtype).to(DEV), rand_x((3, top_k, K), dtype, 12)
    y = ex(x, ids)
    for k0 in sorted({0, top_k - 1}):
        for wdt in (torch.float32, dtype):
            w = torch.zeros(3, top_k, dtype=wdt, device=DEV)
            w[:, k0] = 1
            out, buf = launch_fused(ex, COMBINE, x, ids, w)
            assert guards_intact(buf)
            assert torch.equal(out, y[:, k0, :]), (k0, wdt, float((out.float() - y[:, k0, :].float()).abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------- long K
def decode_bound(got, ref, factor=1.0):
    """The project's one bound for decode kernels: mean relative error below 4e-4 plus the output quantum."""
    rel = float(np.abs(got - ref).mean() / np.abs(ref).mean())
    return rel, factor * (4e-4 + 2.0 ** -25 / np.abs(ref).mean())


def test_long_k_against_float64():
    """K = 14336: 56 chunks, four per virtual wave, where no single-layer decode3 plan exists — against float64 x @ dequantize().T."""
    K = 14336
    ex = make_experts(64, K, 128, torch.float16, "tensor", False, n=4)
    ids = torch.tensor([[1, 3], [0, 1]], dtype=torch.int64, device=DEV)
    x = rand_x((2, K), torch.float16, 3)
    W = [f64(ex.expert(e).dequantize(torch.float32)) for e in range(4)]
    proj = np.stack([np.stack([f64(x[t]) @ W[e].T for e in row]) for t, row in enumerate(ids.tolist())])  # [2, 2, 64]
    # the members themselves, through a one-hot combine: the gate half and the up half
    for k0 in (0, 1):
        w = torch.zeros(2, 2, device=DEV)
        w[:, k0] = 1
        out, buf = launch_fused(ex, COMBINE, x, ids, w)
        assert guards_intact(buf)
        for name, cols in (("gate", slice(0, 32)), ("up", slice(32, 64))):
            rel, bound = decode_bound(f64(out)[:, cols], proj[:, k0, cols])
            print(f"K=14336 member {k0} {name}: rel={rel:.3e} bound={bound:.3e}")
            assert rel < bound, (k0, name, rel)
    # GLU against the float64 projections: the bound doubled for the product of two bounded factors
    out, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    g, u = proj[..., :32], proj[..., 32:]
    rel, bound = decode_bound(f64(out).reshape(2, 2, 32), g / (1.0 + np.exp(-g)) * u, 2.0)
    print(f"K=14336 GLU: rel={rel:.3e} bound={bound:.3e}")
    assert rel < bound, rel
    # COMBINE, N = 32, top_k = 2
    ex = make_experts(32, K, 128, torch.float16, "tensor", False, n=4)
    W = [f64(ex.expert(e).dequantize(torch.float32)) for e in range(4)]
    _, w = routing(2, 2, torch.float32, 13)
    out, buf = launch_fused(ex, COMBINE, x, ids, w)
    assert guards_intact(buf)
    ref = np.stack([sum(float(w[t, k]) * (f64(x[t]) @ W[e].T) for k, e in enumerate(row)) for t, row in enumerate(ids.tolist())])
    rel, bound = decode_bound(f64(out), ref)
    print(f"K=14336 COMBINE: rel={rel:.3e} bound={bound:.3e}")
    assert rel < bound, rel


# --------------------------------------------------------------------------------------------------------------------------- invalid ids
def bad_ids(ids_dtype):
    return [-1, E, 2 ** 31 - 1] + ([(1 << 32) + 1, -(1 << 40)] if ids_dtype == torch.int64 else [-(2 ** 31)])


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
def test_glu_gives_zero_rows_for_invalid_ids_and_touches_nothing_else(ids_dtype):
    N, K = 96, 768
    ex = make_experts(N, K, bias=True)
    bad = bad_ids(ids_dtype)
    flat = [4, bad[0], bad[1], 0, bad[2], 7] + bad[3:] + [1]
    if len(flat) % 2:
        flat.append(bad[0])
    ids = torch.tensor(flat, dtype=ids_dtype, device=DEV).view(-1, 2)
    x = rand_x((ids.shape[0], K), torch.float16, 5)
    out, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    valid = torch.tensor([0 <= e < E for e in flat], device=DEV)
    assert bool((out[~valid].view(torch.int16) == 0).all())
    y = ex(x, ids).view(-1, N)
    check_glu(out[valid], y[valid], torch.float16, f"valid slots among invalid ones, {ids_dtype}")


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
def test_combine_adds_exactly_nothing_for_an_invalid_id(ids_dtype):
    N, K = 48, 768
    ex = make_experts(N, K, bias=True)
    bad = bad_ids(ids_dtype)
    top_k, T = 3, len(bad) + 1
    ids, w = routing(T, top_k, torch.float32, 17)
    x = rand_x((T, top_k, K), torch.float16, 6)
    broken, zeroed = ids.clone(), w.clone()
    for t, b in enumerate(bad):  # token t: slot t % top_k is invalid; the last token: every slot
        broken[t, t % top_k] = b
        zeroed[t, t % top_k] = 0
    broken[T - 1] = torch.tensor([bad[i % len(bad)] for i in range(top_k)])
    out, buf = launch_fused(ex, COMBINE, x, broken.to(ids_dtype).to(DEV), w)
    assert guards_intact(buf)
    # the same call with the id valid and the weight 0
    want, buf2 = launch_fused(ex, COMBINE, x, ids.to(ids_dtype).to(DEV), zeroed)
    assert guards_intact(buf2)
    assert torch.equal(out[:T - 1].view(torch.int16), want[:T - 1].view(torch.int16))
    assert bool((out[T - 1].view(torch.int16) == 0).all()), "a token without a valid id is a row of zeros"
    check_combine(want[:T - 1], ex(x, ids.to(ids_dtype).to(DEV))[:T - 1], zeroed[:T - 1], torch.float16, f"weight 0, {ids_dtype}")


# ------------------------------------------------------------------------------------------------------------------------ the whole MLP
def make_mlp(H=768, I=256, dtype=torch.float16, bias=True):
    gate_up = make_experts(2 * I, H, 128, dtype, "tensor", bias, seed=1)
    down = make_experts(H, I, 128, dtype, "tensor", bias, seed=2)
    return GemLiteExpertsMLP(gate_up, down)


def check_mlp(mlp, x, ids, w, out, what):
    """out against the unfused pipeline, stage by stage: GLU of gate_up's launch, then the weighted sum of down's launch on that h."""
    h = mlp.gate_up.forward_glu(x, ids)
    check_glu(h, mlp.gate_up(x, ids), x.dtype, what)
    check_combine(out, mlp.down(h, ids), w, x.dtype, what)


def test_a_captured_mlp_reads_ids_weights_and_x_when_it_replays():
    mlp = make_mlp()
    T, top_k, H = 3, 2, 768
    x = rand_x((T, H), torch.float16, 4)
    ids, w = routing(T, top_k, torch.float32, 20)
    ids = ids.to(DEV)
    mlp(x, ids, w)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = mlp(x, ids, w)
    for i in range(3):
        new_ids, new_w = routing(T, top_k, torch.float32, 21 + i, signs=i == 2)
        ids.copy_(new_ids.to(DEV))
        w.copy_(new_w)
        x.copy_(rand_x((T, H), torch.float16, 30 + i))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, mlp(x, ids, w)), i
        check_mlp(mlp, x, ids, w, y, f"replay {i}")


def test_expert_strides_are_64_bit():
    """Through the C ABI: two experts 4 GiB apart inside one buffer; expert 1 lives at the far offset."""
    N, K = 48, 768
    ex = make_experts(N, K, n=2)
    words = (K // 8) * N
    big = torch.empty((1 << 30) + words, dtype=torch.int32, device=DEV)  # 4 GiB + one expert
    big[:words].copy_(ex.W_q[0].reshape(-1))
    big[1 << 30:].copy_(ex.W_q[1].reshape(-1))
    ids = torch.tensor([[1, 0], [1, 1]], dtype=torch.int64, device=DEV)
    x = rand_x((2, K), torch.float16, 6)
    _, w = routing(2, 2, torch.float32, 23)
    buf = torch.full((GUARD + 2 * N + GUARD,), SENTINEL, dtype=torch.float16, device=DEV)
    out = buf[GUARD:GUARD + 2 * N]
    e = X._call_args(x, ids, out.data_ptr(), None, ex.get_tensor_args(), ex.get_meta_args(), 2)
    e.layer.w_q = big.data_ptr()
    e.stride_expert_w = 1 << 32
    f = X._fused_args(e, COMBINE, w.data_ptr(), X.TORCH_TO_DTYPE[w.dtype].value, 2)
    assert _hip.load().gemlite_hip_forward_experts_fused(C.byref(f), _hip.current_stream_handle(x.device)) == 0
    torch.cuda.synchronize()
    assert guards_intact(buf)
    check_combine(out.view(2, N), ex(x, ids), w, torch.float16, "experts 4 GiB apart")
    onehot = torch.tensor([[1.0, 0.0], [0.0, 1.0]], device=DEV)
    f = X._fused_args(e, COMBINE, onehot.data_ptr(), X.TORCH_TO_DTYPE[onehot.dtype].value, 2)
    assert _hip.load().gemlite_hip_forward_experts_fused(C.byref(f), _hip.current_stream_handle(x.device)) == 0
    torch.cuda.synchronize()
    y = ex(x, ids)
    assert torch.equal(out.view(2, N), torch.stack([y[0, 0], y[1, 1]])) and guards_intact(buf)


def test_opcheck_and_torch_compile_fullgraph():
    mlp = make_mlp()
    x = rand_x((3, 768), torch.float16, 8)
    ids, w = routing(3, 2, torch.float32, 24)
    ids = ids.to(DEV)
    g, d = mlp.gate_up, mlp.down
    torch.library.opcheck(torch.ops.gemlite.forward_experts_glu.default, (x, ids, g.bias, g.get_tensor_args(), g.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))
    h = g.forward_glu(x, ids)
    torch.library.opcheck(torch.ops.gemlite.forward_experts_combine.default, (h, ids, w, d.bias, d.get_tensor_args(), d.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))
    eager = mlp(x, ids, w)
    compiled = torch.compile(mlp, fullgraph=True)(x, ids, w)
    torch.cuda.synchronize()
    assert torch.equal(compiled, eager)
    check_mlp(mlp, x, ids, w, eager, "eager")
