"""gemlite_hip_forward_experts_rows_glu / gemlite_hip_experts_combine and GemLiteExpertsMLP.forward_batched_fused on the MI355X: the GLU
launch is silu(gate) * up of the unfused rows launch at the same R within the 1-ulp bound of tests/test_experts_fused_gpu.py, the combine
launch is the fp32 loop of torch bit for bit (and the decode kernel's combine on the same y), the fused MLP is its own composition bit
for bit and lies within the §4 gate of forward_batched, and a captured MLP follows the ids and weights of every replay.  Out-of-range
ids are a defined input with a defined result; no test here provokes a fault."""
import ctypes as C
import functools

import pytest
import torch

from gemlite_amd import GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X
from tests.test_experts_fused_gpu import check_combine, check_glu, ulp  # noqa: F401 (ulp: the bound check_glu applies)
from tests.test_experts_gpu import DEV, GUARD, SENTINEL, E, guards_intact, make_experts, rand_x

pytestmark = pytest.mark.gpu
ROWS = [  # (dtype, group, zeros, bias, ids dtype)
    (torch.float16, 128, "tensor", False, torch.int64),
    (torch.bfloat16, 64, "tensor", True, torch.int32),
    (torch.float16, 128, "int", True, torch.int64),
    (torch.bfloat16, 128, "int", False, torch.int32),
]
GLU_SHAPES = [(32, 256), (96, 768), (512, 4352), (1536, 2048)]  # one tile pair, one chunk | three pairs | 17 chunks | many tiles
HIGH = (1 << 32) + 1  # an int64 id whose low dword is a valid expert


def rs_of(gs):
    return (16, 32, 48, 64) if gs >= 128 else (16, 32)


@functools.lru_cache(maxsize=None)
def experts(N, K, row):
    dtype, gs, zeros, bias, _ = ROWS[row]
    return make_experts(N, K, gs, dtype, zeros, bias)


def batch_ids(R, ids_dtype):
    """[T, 2] with R + 14 slots (never a multiple of 16): expert 3 holds R + 5 of them — two work blocks, the second with 5 rows —
    experts 4 and 7 none, three slots are invalid (-1, E, and a high dword or the most negative id); shuffled, so tokens mix experts."""
    bad = [-1, E, HIGH if ids_dtype == torch.int64 else -(2 ** 31)]
    flat = [3] * (R + 5) + [0, 1, 2, 5, 6, 5] + bad
    perm = torch.randperm(len(flat), generator=torch.Generator().manual_seed(R)).tolist()
    return torch.tensor([flat[i] for i in perm], dtype=ids_dtype, device=DEV).view(-1, 2)


def glu_guarded(ex, x, ids, routing, pad=0):
    """The C call on an output window with guard bands on both sides and rows `pad` elements apart -> out [slots, I]."""
    N, K = ex.out_features, ex.in_features
    I = N // 2
    rows, spx = X._split(x, ids, K)
    n, stride = ids.numel(), I + pad
    buf = torch.full((GUARD + n * stride + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    out = buf[GUARD:GUARD + n * stride].view(n, stride)
    e = X._call_args(x.contiguous().view(rows, K), ids.contiguous(), out.data_ptr(), ex.bias, ex.get_tensor_args(), ex.get_meta_args(), spx)
    e.stride_out_slot = stride
    g = X._glu_rows_args(X._rows_args(e, routing.rows_per_block, routing.workspace))
    rc = _hip.load().gemlite_hip_forward_experts_rows_glu(C.byref(g), _hip.current_stream_handle(x.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    assert guards_intact(buf) and bool((out[:, I:] == SENTINEL).all()), "written outside the rows of the output"
    return out[:, :I]


def valid_slots(ids, n_experts=E):
    flat = ids.reshape(-1)
    return (flat >= 0) & (flat < n_experts)


GLU_CASES = [(shape, row, R) for shape in GLU_SHAPES for row in range(len(ROWS)) for R in rs_of(ROWS[row][1])]


@pytest.mark.parametrize("shape,row,R", GLU_CASES, ids=[f"{s[0]}x{s[1]}-row{r}-R{R}" for s, r, R in GLU_CASES])
def test_glu_is_silu_gate_times_up_of_the_unfused_rows_launch_at_the_same_block_size(shape, row, R):
    N, K = shape
    I = N // 2
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    assert ex.rows_per_block(1, R, glu=True) == R
    ids = batch_ids(R, ids_dtype)
    T = ids.shape[0]
    one = torch.tensor([[6]], dtype=ids_dtype, device=DEV)
    for what, x, i, pad in (("shared x", rand_x((T, K), dtype, 1), ids, 0), ("x per slot", rand_x((T, 2, K), dtype, 2), ids, 16),
                            ("T = 1", rand_x((1, K), dtype, 3), one, 0)):
        routing = ex.route(i, R)
        out = glu_guarded(ex, x, i, routing, pad)
        ok = valid_slots(i)
        assert bool((out[~ok].view(torch.int16) == 0).all()), f"{what}: an invalid slot is not a row of zeros"
        y = ex.forward_batched(x, i, routing)
        check_glu(out[ok], y.reshape(-1, N)[ok], dtype, f"{N}x{K} row {row} R {R} {what}")
        h = ex.forward_batched_glu(x, i, routing)  # the module: the same launch, its own output tensor
        assert tuple(h.shape) == tuple(i.shape) + (I,) and torch.equal(h.reshape(-1, I), out), what
    own = ex.forward_batched_glu(x, one)  # ... and its own routing: the default block size of one slot is 16
    assert tuple(own.shape) == (1, 1, I) and (R != 16 or torch.equal(own, h))


@pytest.mark.parametrize("row", [0, 1])
def test_glu_stays_finite_where_the_gate_reaches_plus_and_minus_60(row):
    N, K = 96, 768
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    ex = experts(N, K, row)
    ids = torch.tensor([[5, 2], [2, 7]], dtype=ids_dtype, device=DEV)
    x = rand_x((2, K), dtype, 4)
    routing = ex.route(ids, 16)
    gate = ex.forward_batched(x[1:], ids[1:])[0, 0, :N // 2].float()
    x[1] *= float(64.0 / min(gate.max(), -gate.min()))  # token 1's first expert: both ends of its gate values beyond 60
    y = ex.forward_batched(x, ids, routing)
    gate = y[1, 0, :N // 2].float()
    assert float(gate.max()) >= 60 and float(gate.min()) <= -60 and bool(torch.isfinite(y).all())
    out = glu_guarded(ex, x, ids, routing)
    check_glu(out, y, dtype, f"gate beyond +-60 row {row}")


def test_a_nan_row_reaches_only_its_own_slots():
    N, K = 96, 768
    ex = experts(N, K, 2)
    ids = torch.tensor([[2, 5], [2, 2], [5, 0], [2, 7]], dtype=torch.int64, device=DEV)  # expert 2's block holds tokens 0, 1, 1, 3
    x = rand_x((4, K), torch.float16, 9)
    clean = ex.forward_batched_glu(x, ids)
    x[1, 300] = float("nan")
    h = ex.forward_batched_glu(x, ids)
    torch.cuda.synchronize()
    assert bool(torch.isnan(h[1]).all()), "every output of the token with the NaN is NaN"
    for t in (0, 2, 3):
        assert torch.equal(h[t], clean[t]) and bool(torch.isfinite(h[t]).all()), t
    xs = rand_x((4, 2, K), torch.float16, 10)  # one row per slot: only that slot
    clean = ex.forward_batched_glu(xs, ids)
    xs[1, 0, 7] = float("nan")
    h = ex.forward_batched_glu(xs, ids)
    torch.cuda.synchronize()
    keep = torch.ones(4, 2, dtype=torch.bool, device=DEV)
    keep[1, 0] = False
    assert bool(torch.isnan(h[1, 0]).all()) and torch.equal(h[keep], clean[keep])


# ------------------------------------------------------------------------------------------------------------------------------ COMBINE
@functools.lru_cache(maxsize=None)
def small_experts(dtype):
    return make_experts(48, 768, 128, dtype, "tensor", True)


def combine_ref(y, ids, w, n_experts=E):
    """The fp32 loop: one multiply, one add per slot in ascending k from zeros, one rounding; slots with an invalid id are skipped."""
    T, top_k, N = y.shape
    acc = torch.zeros(T, N, dtype=torch.float32, device=y.device)
    ok = (ids >= 0) & (ids < n_experts)
    for k in range(top_k):
        term = acc + w[:, k, None].float() * y[:, k].float()
        acc = torch.where(ok[:, k, None], term, acc)
    return acc.to(y.dtype)


def combine_inputs(T, top_k, N, dtype, weights, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(T, top_k, N, generator=g).to(dtype).to(DEV)
    ids = torch.randint(0, E, (T, top_k), generator=g).to(DEV)
    w = torch.rand(T, top_k, generator=g) + 0.05
    w = w / w.sum(-1, keepdim=True)
    if weights == "mixed signs":
        w = w * (torch.randint(0, 2, (T, top_k), generator=g) * 2 - 1) * 1.5
    return y, ids, w.to(dtype if weights == "16-bit" else torch.float32).to(DEV)


def combine_guarded(y2, ids, w, T, n_experts=E, pad=0):
    """The C call on an output window with guard bands on both sides and rows `pad` apart -> out [T, N]; y2 [slots, N] as it lies."""
    N, top_k = y2.shape[1], ids.numel() // T
    stride = N + pad
    buf = torch.full((GUARD + T * stride + GUARD,), SENTINEL, dtype=y2.dtype, device=DEV)
    out = buf[GUARD:GUARD + T * stride].view(T, stride)
    c = X._combine_args(y2, ids.contiguous(), w.contiguous(), out, n_experts, top_k)
    rc = _hip.load().gemlite_hip_experts_combine(C.byref(c), _hip.current_stream_handle(y2.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    assert guards_intact(buf) and bool((out[:, N:] == SENTINEL).all()), "written outside the rows of the output"
    return out[:, :N]


@pytest.mark.parametrize("weights", ["fp32", "16-bit", "mixed signs"])
@pytest.mark.parametrize("top_k", [1, 2, 3, 8, 16, 17, 64])
def test_combine_is_the_fp32_loop_bit_for_bit(top_k, weights):
    seed = 0
    for dtype in (torch.float16, torch.bfloat16):
        ex = small_experts(dtype)
        for T in (1, 3, 40):
            for N in (16, 48, 2048):
                seed += 1
                y, ids, w = combine_inputs(T, top_k, N, dtype, weights, seed)
                want = combine_ref(y, ids, w)
                out = ex.combine_batched(y, ids, w)
                assert tuple(out.shape) == (T, N) and out.dtype == dtype
                assert torch.equal(out, want), (dtype, T, N, float((out.float() - want.float()).abs().max()))
                check_combine(out, y, w, dtype, f"{dtype} T {T} top_k {top_k} N {N} {weights}")
                # int32 ids, the C call into a guarded window with padded rows
                assert torch.equal(combine_guarded(y.view(-1, N), ids.int(), w, T, pad=16 if N == 48 else 0), want)


@pytest.mark.parametrize("top_k", [1, 3, 8, 16])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_combine_of_the_decode_launch_is_the_decode_kernels_own_combine(dtype, top_k):
    ex = small_experts(dtype)
    g = torch.Generator().manual_seed(top_k)
    ids = torch.randint(0, E, (5, top_k), generator=g).to(DEV)
    ids[2, 0] = -1
    w = torch.softmax(torch.randn(5, top_k, generator=g), -1).to(DEV)
    for x in (rand_x((5, 768), dtype, 3), rand_x((5, top_k, 768), dtype, 4)):
        for wt in (w, w.to(dtype)):
            assert torch.equal(ex.combine_batched(ex(x, ids), ids, wt), ex.forward_combine(x, ids, wt))


@pytest.mark.parametrize("ids_dtype", [torch.int32, torch.int64])
def test_invalid_ids_add_exactly_nothing_and_a_token_without_a_valid_id_is_plus_zero(ids_dtype):
    dtype, T, top_k, N = torch.float16, 4, 3, 48
    ex = small_experts(dtype)
    y, ids, w = combine_inputs(T, top_k, N, dtype, "fp32", 11)
    bad = [-1, E, HIGH if ids_dtype == torch.int64 else -(2 ** 31)]
    ids = ids.to(ids_dtype)
    ids[0, 1], ids[1, 0], ids[1, 2] = bad[0], bad[1], bad[2]
    ids[2] = torch.tensor(bad, dtype=ids_dtype)
    want = combine_ref(y, ids.long().clamp(-1, E), w)
    # what an invalid slot holds is never read: NaN / Inf in its y row and its weight change nothing
    y2, w2 = y.clone(), w.clone()
    y2[0, 1], y2[1, 0], y2[2] = float("nan"), float("inf"), float("nan")
    w2[0, 1], w2[1, 2], w2[2] = float("nan"), float("-inf"), float("inf")
    for yy, ww in ((y, w), (y2, w2), (y2, w2.to(dtype))):
        out = ex.combine_batched(yy, ids, ww)
        assert bool(torch.isfinite(out).all()) and bool((out[2].view(torch.int16) == 0).all()), "a token without a valid id is +0"
        if ww.dtype == torch.float32:
            assert torch.equal(out, want)
        else:
            assert torch.equal(out, combine_ref(y, ids.long().clamp(-1, E), w.to(dtype)))


def test_a_view_that_is_only_4_byte_aligned_gives_the_bits_of_the_aligned_call():
    for dtype in (torch.float16, torch.bfloat16):
        ex = small_experts(dtype)
        for T, top_k, N in ((3, 2, 48), (40, 8, 2048)):
            y, ids, w = combine_inputs(T, top_k, N, dtype, "fp32", 5)
            want = ex.combine_batched(y, ids, w)
            wide = torch.zeros(T, top_k, N + 16, dtype=dtype, device=DEV)
            view = wide[..., 2:2 + N]
            view.copy_(y)
            assert view.data_ptr() % 16 == 4 and torch.equal(ex.combine_batched(view, ids, w), want)
            assert torch.equal(combine_guarded(view.view(-1, N), ids, w, T, pad=2), want)  # and 4-byte aligned output rows
            # a slice of a forward_batched output: the [gate; up] halves of y are views with the row stride of the whole
            assert torch.equal(ex.combine_batched(wide[..., 16:], ids, w), ex.combine_batched(wide[..., 16:].contiguous(), ids, w))


# ---------------------------------------------------------------------------------------------------------------------------------- MLP
@functools.lru_cache(maxsize=None)
def make_mlp(gs_gate, gs_down, n=E, hidden=256, inter=256, dtype=torch.float16):
    gate = make_experts(inter, hidden, gs_gate, dtype, "tensor", False, n=n, seed=1)
    up = make_experts(inter, hidden, gs_gate, dtype, "tensor", False, n=n, seed=2)
    return GemLiteExpertsMLP(GemLiteExperts.from_gate_up([gate.expert(e) for e in range(n)], [up.expert(e) for e in range(n)]),
                             make_experts(hidden, inter, gs_down, dtype, "tensor", False, n=n, seed=3))


def mlp_inputs(n, T, top_k, hidden, seed=7):
    g = torch.Generator().manual_seed(seed)
    ids = torch.stack([torch.randperm(n, generator=g)[:top_k] for _ in range(T)]).to(DEV)
    w = torch.softmax(torch.randn(T, top_k, generator=g), -1).to(DEV)
    return rand_x((T, hidden), torch.float16, seed + 1), ids, w


def check_gate(out, ref, what):
    """The §4 gate as tests/test_experts_rows_gpu.py::test_the_mlp_routes_once_and_equals_the_composition applies it."""
    ref = ref.double()
    err, scale, tol = (out.double() - ref).abs(), float(ref.abs().mean()), 1e-3
    print(f"{what}: rel={float(err.mean()) / scale:.3e} max={float(err.max()):.3e}")
    assert float(err.mean()) / scale < tol and bool((err <= 10 * tol * scale + 4 * tol * ref.abs()).all()), what


@pytest.mark.parametrize("gs_gate,gs_down,n,T,top_k,R", [(128, 128, E, 140, 2, 48), (128, 32, E, 140, 2, 32), (64, 64, 128, 40, 8, 16)])
def test_the_fused_mlp_is_its_composition_and_lies_within_the_gate_of_forward_batched(gs_gate, gs_down, n, T, top_k, R):
    """The settings of tests/test_experts_rows_gpu.py::test_the_mlp_routes_once_and_equals_the_composition (R = 48 shared; down in groups
    of 32 forcing 32) and 128 experts in groups of 64.  Like that test, the comparison with the composition spans two route launches: the
    bits of a slot depend on the row the route gives it, and on these ids the route repeats its order."""
    mlp = make_mlp(gs_gate, gs_down, n)
    x, ids, w = mlp_inputs(n, T, top_k, mlp.hidden_size)
    assert mlp.glu_fused() and mlp.rows_per_block_fused(ids.numel()) == R
    mlp.forward_batched_fused(x, ids, w)  # (warm-up, as in front of a capture: every route below finds the ids where the first left them)
    out = mlp.forward_batched_fused(x, ids, w)
    routing = mlp.gate_up.route(ids, R)
    h = mlp.gate_up.forward_batched_glu(x, ids, routing)
    want = mlp.down.combine_batched(mlp.down.forward_batched(h, ids, routing), ids, w)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (T, mlp.hidden_size) and torch.equal(out, want)
    check_gate(out, mlp.forward_batched(x, ids, w), f"fused MLP vs forward_batched g{gs_gate}/g{gs_down} E {n}")
    # the 16-bit weights a router may hand over, and int32 ids
    assert torch.equal(mlp.forward_batched_fused(x, ids.int(), w.half()),
                       mlp.down.combine_batched(mlp.down.forward_batched(h, ids, routing), ids, w.half()))


def test_gate_up_in_groups_of_32_takes_the_torch_glu_and_still_the_combine_launch():
    mlp = make_mlp(32, 128)
    x, ids, w = mlp_inputs(E, 140, 2, mlp.hidden_size)
    assert not mlp.glu_fused() and mlp.rows_per_block_fused(ids.numel()) == mlp.rows_per_block(ids.numel()) == 32
    out = mlp.forward_batched_fused(x, ids, w)
    routing = mlp.gate_up.route(ids, 32)
    y = mlp.gate_up.forward_batched(x, ids, routing).float()
    inter = mlp.intermediate_size
    h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(x.dtype)
    want = mlp.down.combine_batched(mlp.down.forward_batched(h, ids, routing), ids, w)
    assert torch.equal(out, want)
    check_gate(out, mlp.forward_batched(x, ids, w), "fallback MLP vs forward_batched")
    with pytest.raises(NotImplementedError, match="groups of 32 have no GLU form"):
        mlp.gate_up.forward_batched_glu(x, ids, routing)


def test_a_captured_fused_mlp_follows_the_ids_and_weights_of_every_replay():
    mlp = make_mlp(128, 128)
    T, top_k = 18, 2
    x, ids, w = mlp_inputs(E, T, top_k, mlp.hidden_size, seed=20)
    mlp.forward_batched_fused(x, ids, w)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = mlp.forward_batched_fused(x, ids, w)
    for i in range(3):
        nx, nids, nw = mlp_inputs(E, T, top_k, mlp.hidden_size, seed=30 + i)
        if i == 1:
            nids[4, 1], nids[9, 0] = -1, E
        if i == 2:
            nids[:] = 5  # one expert, 36 slots: three work blocks of 16
        x.copy_(nx), ids.copy_(nids), w.copy_(nw)
        graph.replay()
        torch.cuda.synchronize()
        eager = mlp.forward_batched_fused(x, ids, w)
        assert torch.equal(out, eager), i
        check_gate(out, mlp.forward_batched(x, ids, w), f"replay {i}")


def test_opcheck_of_the_two_ops():
    ex = experts(96, 768, 2)
    ids = torch.tensor([[5, 2], [2, 7], [0, 5]], dtype=torch.int64, device=DEV)
    x = rand_x((3, 768), torch.float16, 8)
    ws = ex.route(ids, 16).workspace
    torch.library.opcheck(torch.ops.gemlite.forward_experts_rows_glu.default, (x, ids, ws, 16, ex.bias, ex.get_tensor_args(), ex.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))
    y, w = ex.forward_batched(x, ids), torch.rand(3, 2, device=DEV)
    torch.library.opcheck(torch.ops.gemlite.experts_combine.default, (y, ids, w, E), test_utils=("test_schema", "test_faketensor"))
