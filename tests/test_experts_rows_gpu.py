"""gemlite_hip_experts_route + gemlite_hip_forward_experts_rows / GemLiteExperts.forward_batched on the MI355X: the routed work table keeps
its contract (tests/test_experts_rows_cpu.py::check_table), every valid slot is bit-identical to its row of the expert's own forced
gemm_w4_rows_kernel launch of the same (MT, SPG) form, invalid slots are zero rows, nothing else is touched, and a captured route +
forward follows the ids of every replay.  Out-of-range ids are a defined input with a defined result; no test here provokes a fault."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from gemlite_amd import ExpertsRouting, GemLiteExperts, GemLiteExpertsMLP, _hip, core, experts as X
from tests.test_experts_gpu import DEV, E, GUARD, SENTINEL, guards_intact, make_experts, rand_x
from tests.test_experts_rows_cpu import HEADER, blocks_max, blocks_used, buckets_of, check_table

pytestmark = pytest.mark.gpu
SHAPES = {"one tile, one chunk": (16, 256), "three tiles, five waves idle": (48, 768), "paired tiles, 17 chunks": (256, 4352)}
FORCED = (9, 1, 0, 0)  # gemm_w4_rows_kernel at any M, one column tile per block
TABLE_GUARD, TABLE_SENTINEL = 64, -7
HIGH = (1 << 32) + 1  # an int64 id whose low dword is a valid expert


@functools.lru_cache(maxsize=None)
def experts_of(N, K, gs, dtype, zeros, bias):
    return make_experts(N, K, gs, dtype, zeros, bias)


def id_patterns(R, ids_dtype):
    """name -> ids [..., top_k] (as lists): all slots on one expert with c = R - 1, R, R + 1, 2 R + 1 (one token whose top_k is c: the
    shared-row layout then has ONE x row for all of them); a batch with an expert without a slot, repeats inside a token and the invalid
    ids; a single slot."""
    bad = [-1, E] + ([HIGH] if ids_dtype == torch.int64 else [-(2 ** 31)])
    mixed = [[5, 5, 2], [2, bad[0], 7], [0, 5, bad[1]], [bad[2], 1, 1], [7, 7, 7], [4, 0, 5]]  # (experts 3 and 6 have no slot)
    pats = {f"one expert, c = {c}": [3] * c for c in (R - 1, R, R + 1, 2 * R + 1)}
    pats["mixed"] = mixed
    pats["one slot"] = [[6]]
    return pats


def route_guarded(ex, ids, R):
    """The C call on a workspace with a guard band behind it -> (routing, the whole int32 buffer, the entries the table may use)."""
    n = ids.numel()
    need = X.rows_workspace_ints(n, ex.num_experts, R)
    buf = torch.full((need + TABLE_GUARD,), TABLE_SENTINEL, dtype=torch.int32, device=DEV)
    e = X._stand_in_args(ex.bias, ex.get_tensor_args(), ex.get_meta_args(), n)
    e.ids, e.ids_dtype = ids.data_ptr(), X.TORCH_TO_DTYPE[ids.dtype].value
    r = X._rows_args(e, R, buf[:need])
    rc = _hip.load().gemlite_hip_experts_route(C.byref(r), _hip.current_stream_handle(ids.device))
    assert rc == 0, _hip.status_string(rc)
    return ExpertsRouting(buf[:need], R, n, ex.num_experts), buf, need


def check_routing(buf, need, ids, R, E=E):
    """The table against the restated contract; nothing written behind the table, nor into the entries beyond the used count."""
    table = buf.cpu().numpy()
    flat = ids.reshape(-1).cpu().numpy()
    used = check_table(table[:need], flat, E, R)
    bmax = blocks_max(len(flat), E, R)
    assert (table[need:] == TABLE_SENTINEL).all(), "written behind the table"
    assert (table[HEADER + used:HEADER + bmax] == TABLE_SENTINEL).all() and (table[HEADER + bmax + used * R:need] == TABLE_SENTINEL).all()
    return used


def forward_guarded(ex, x, ids, routing, pad=0):
    """The C call on an output window with guard bands on both sides and rows `pad` elements apart -> (out [slots, N], the buffer)."""
    N, K = ex.out_features, ex.in_features
    rows, spx = X._split(x, ids, K)
    n, stride = ids.numel(), N + pad
    buf = torch.full((GUARD + n * stride + GUARD,), SENTINEL, dtype=x.dtype, device=DEV)
    out = buf[GUARD:GUARD + n * stride].view(n, stride)
    e = X._call_args(x.contiguous().view(rows, K), ids.contiguous(), out.data_ptr(), ex.bias, ex.get_tensor_args(), ex.get_meta_args(), spx)
    e.stride_out_slot = stride
    r = X._rows_args(e, routing.rows_per_block, routing.workspace)
    rc = _hip.load().gemlite_hip_forward_experts_rows(C.byref(r), _hip.current_stream_handle(x.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    assert guards_intact(buf) and bool((out[:, N:] == SENTINEL).all()), "written outside the rows of the output"
    return out[:, :N], buf


_named = set()


def oracle_rows(ex, x, ids, R):
    """[slots, N]: every valid slot from its expert's own forced gemm_w4_rows_kernel launch with R / 16 row tiles, on a matrix of R rows
    that holds the slot's x row (+ the bias as `out += bias`: two roundings); invalid slots zero."""
    N, K = ex.out_features, ex.in_features
    rows, spx = X._split(x, ids, K)
    x2, flat = x.contiguous().view(rows, K), ids.reshape(-1).tolist()
    want = torch.zeros((len(flat), N), dtype=x.dtype, device=DEV)
    for e in range(ex.num_experts):
        slots = [s for s, v in enumerate(flat) if v == e]
        lin = ex.expert(e)
        for i in range(0, len(slots), R):
            part = slots[i:i + R]
            xm = x2[[s // spx for s in part] + [part[0] // spx] * (R - len(part))].contiguous()
            key = (id(ex), R)
            if key not in _named:
                a = core._call_args(xm, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, FORCED, False, 0x1000, (N, 1))
                name = _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode()
                assert name == f"gemm_w4_rows_kernel<{R}x16>", name
                _named.add(key)
            y = core._hip_matmul(xm, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, FORCED)
            if lin.bias is not None:
                y += lin.bias
            want[part] = y[:len(part)]
    return want


def check_outputs(ex, x, ids, out, R):
    want = oracle_rows(ex, x, ids, R)
    valid = torch.from_numpy(buckets_of(ids.reshape(-1).cpu().numpy(), ex.num_experts) < ex.num_experts).to(DEV)
    assert bool((out[~valid].view(torch.int16) == 0).all()), "an invalid slot is not a row of zeros"
    same = (out.view(torch.int16) == want.view(torch.int16)).all(dim=1)
    assert bool(same.all()), ("slots that differ from their expert's own rows launch", (~same).nonzero().flatten().tolist()[:8])


CASES = [(shape, gs, dtype, zeros, bias, idt, R)
         for shape, gs, dtype, zeros, bias, idt, R in itertools.product(SHAPES, (32, 64, 128, 256), (torch.float16, torch.bfloat16),
                                                                         ("tensor", "int"), (False, True), (torch.int32, torch.int64), (16, 32, 48, 64))
         if (R <= 32 or gs > 32)            # groups of 32: 16 / 32 rows per block (the registers of the kernel)
         and gs < SHAPES[shape][1]]         # a group that spans K (256 at K = 256) is packed as CHANNEL scales, which GemLiteExperts.from_layers
                                            # has always refused (W_group_mode 1..4, channel_scale_mode 0): not an experts layer at all


@pytest.mark.parametrize("shape,gs,dtype,zeros,bias,ids_dtype,R", CASES,
                         ids=[f"{SHAPES[c[0]][0]}x{SHAPES[c[0]][1]}-g{c[1]}-{str(c[2])[6:]}-z{c[3]}-b{int(c[4])}-{str(c[5])[6:]}-R{c[6]}" for c in CASES])
def test_the_table_keeps_its_contract_and_every_slot_is_its_experts_own_rows_launch(shape, gs, dtype, zeros, bias, ids_dtype, R):
    N, K = SHAPES[shape]
    ex = experts_of(N, K, gs, dtype, zeros, bias)
    assert ex.rows_per_block(1, R) == R
    for name, pattern in id_patterns(R, ids_dtype).items():
        ids = torch.tensor(pattern, dtype=ids_dtype, device=DEV)
        routing, buf, need = route_guarded(ex, ids, R)
        torch.cuda.synchronize()
        check_routing(buf, need, ids, R)
        lead, top_k = tuple(ids.shape[:-1]), ids.shape[-1]
        # one x row per token, shared by its slots — and one row per slot (the down projection)
        for x in (rand_x(lead + (K,), dtype, 1), rand_x(lead + (top_k, K), dtype, 2)):
            out, _ = forward_guarded(ex, x, ids, routing, pad=16 if name == "mixed" else 0)
            check_outputs(ex, x, ids, out, R)
        if name == "mixed":  # the module: its own route, its own output tensor
            y = ex.forward_batched(x, ids, ex.route(ids, R))
            assert tuple(y.shape) == tuple(ids.shape) + (N,) and torch.equal(y.reshape(-1, N), out)


def test_the_default_block_size_and_empty_ids():
    N, K = SHAPES["three tiles, five waves idle"]
    ex = experts_of(N, K, 128, torch.float16, "tensor", True)
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(0, E, (70, 2), generator=g).to(DEV)  # 140 slots over 8 experts: a mean of 17, 21 with its quarter -> blocks of 32
    x = rand_x((70, K), torch.float16, 6)
    routing = ex.route(ids)
    assert routing.rows_per_block == 32 == ex.rows_per_block(140) and routing.workspace.numel() == X.rows_workspace_ints(140, E, 32)
    y = ex.forward_batched(x, ids)
    torch.cuda.synchronize()
    check_table(routing.workspace.cpu().numpy(), ids.reshape(-1).cpu().numpy(), E, 32)
    check_outputs(ex, x, ids, y.reshape(-1, N), 32)
    none = torch.empty((0, 2), dtype=torch.int64, device=DEV)
    assert tuple(ex.forward_batched(x[:0], none).shape) == (0, 2, N) and int(ex.route(none).workspace[0]) == 0
    assert tuple(ex(x[:0], none).shape) == (0, 2, N)  # as forward handles them


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 1e-3), (torch.bfloat16, 4e-3)])
def test_arithmetic_against_float64(dtype, tol):
    """The rows-kernel gate of DESIGN §4: mean|err| / mean|y| < tol and |err| <= 10 tol mean|y| + 4 tol |y| against float64
    x @ dequantize(fp32).T.  (No K of the experts domain is refused by the forced single-layer form — plan_gemm_wn_rows has no K limit
    below the shared 32-bit extents — so every shape is ALSO pinned bit for bit above; this is the one check that does not lean on it.)"""
    N, K = SHAPES["paired tiles, 17 chunks"]
    ex = experts_of(N, K, 64, dtype, "tensor", False)
    ids = torch.tensor([[1, 3], [0, 1], [7, 1]], dtype=torch.int64, device=DEV)
    x = rand_x((3, K), dtype, 3)
    y = ex.forward_batched(x, ids).reshape(-1, N).double().cpu().numpy()
    for s, e in enumerate(ids.reshape(-1).tolist()):
        W = ex.expert(e).dequantize(torch.float32).double().cpu().numpy()
        ref = x[s // 2].double().cpu().numpy() @ W.T
        err, scale = np.abs(y[s] - ref), np.abs(ref).mean()
        print(f"forward_batched {dtype} slot {s} expert {e}: rel={err.mean() / scale:.3e} max={err.max():.3e}")
        assert err.mean() / scale < tol and (err <= 10 * tol * scale + 4 * tol * np.abs(ref)).all(), (s, e)


def test_a_captured_route_and_forward_follow_the_ids_of_every_replay():
    N, K = SHAPES["three tiles, five waves idle"]
    ex = experts_of(N, K, 128, torch.float16, "tensor", True)
    R = 16
    first = [[0, 1]] * 9 + [[2, 3]] * 9                      # 4 experts with 9 slots each: 4 blocks
    others = ([[5, 5]] * 18,                                 # one expert, 36 slots: 3 blocks (down)
              [[e, (e + 1) % E] for e in range(E)] * 2 + [[-1, E], [0, 0]],  # all 8 experts + the invalid bucket: 9 blocks (up)
              [[7, 7]] * 8 + [[6, 4]] * 10)                  # 16 + 10 + 10: 3 blocks, one exactly full
    ids = torch.tensor(first, dtype=torch.int64, device=DEV)
    x = rand_x((18, K), torch.float16, 4)
    ex.forward_batched(x, ids, ex.route(ids, R))  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        routing = ex.route(ids, R)
        y = ex.forward_batched(x, ids, routing)
    seen = []
    for i, new_ids in enumerate((first,) + others):
        ids.copy_(torch.tensor(new_ids, dtype=torch.int64, device=DEV))
        x.copy_(rand_x((18, K), torch.float16, 10 + i))
        graph.replay()
        torch.cuda.synchronize()
        seen.append(check_table(routing.workspace.cpu().numpy(), ids.reshape(-1).cpu().numpy(), E, R))
        eager = ex.forward_batched(x, ids, ex.route(ids, R))
        assert torch.equal(y, eager)
        check_outputs(ex, x, ids, y.reshape(-1, N), R)
    assert seen == [4, 3, 9, 3] == [blocks_used(np.array(p), E, R) for p in (first,) + others]


@pytest.mark.parametrize("gs_down,shared", [(128, True), (32, False)])
def test_the_mlp_routes_once_and_equals_the_composition(gs_down, shared):
    """gate_up (groups of 128) and down (groups of 128: both resolve the same R and share it; groups of 32: down caps at 32 and the MLP
    picks 32 for both).  Bit for bit the two forward_batched calls with the torch ops between; within the §4 gate of
    GemLiteExpertsMLP.forward, whose decode kernels sum K in another order."""
    dtype, hidden, inter = torch.float16, 256, 256
    gate = make_experts(inter, hidden, 128, dtype, "tensor", False, seed=1)
    up = make_experts(inter, hidden, 128, dtype, "tensor", False, seed=2)
    mlp = GemLiteExpertsMLP(GemLiteExperts.from_gate_up([gate.expert(e) for e in range(E)], [up.expert(e) for e in range(E)]),
                            make_experts(hidden, inter, gs_down, dtype, "tensor", False, seed=3))
    g = torch.Generator().manual_seed(7)
    T, top_k = 140, 2  # 280 slots over 8 experts: a mean of 35, 43 with its quarter -> blocks of 48, which groups of 32 do not take
    ids = torch.stack([torch.randperm(E, generator=g)[:top_k] for _ in range(T)]).to(DEV)
    w = torch.softmax(torch.randn(T, top_k, generator=g), -1).to(DEV)
    x = rand_x((T, hidden), dtype, 8)
    n = ids.numel()
    assert mlp.gate_up.rows_per_block(n) == 48 and mlp.down.rows_per_block(n) == (48 if shared else 32)
    R = mlp.rows_per_block(n)
    assert R == (48 if shared else 32)
    out = mlp.forward_batched(x, ids, w)
    routing = mlp.gate_up.route(ids, R)
    y = mlp.gate_up.forward_batched(x, ids, routing).float()
    h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(dtype)
    d = mlp.down.forward_batched(h, ids, routing).float()
    want = (d * w.unsqueeze(-1)).sum(-2).to(dtype)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    check_outputs(mlp.down, h, ids, mlp.down.forward_batched(h, ids, routing).reshape(-1, hidden), R)
    ref = mlp(x, ids, w).double()
    err, scale, tol = (out.double() - ref).abs(), float(ref.abs().mean()), 1e-3
    print(f"MLP forward_batched vs forward: rel={float(err.mean()) / scale:.3e} max={float(err.max()):.3e}")
    assert float(err.mean()) / scale < tol and bool((err <= 10 * tol * scale + 4 * tol * ref.abs()).all())


def test_a_nan_row_reaches_only_its_own_slots():
    N, K = SHAPES["three tiles, five waves idle"]
    ex = experts_of(N, K, 128, torch.float16, "tensor", True)
    ids = torch.tensor([[2, 5], [2, 2], [5, 0], [2, 7]], dtype=torch.int64, device=DEV)  # expert 2's block holds tokens 0, 1, 1, 3
    x = rand_x((4, K), torch.float16, 9)
    clean = ex.forward_batched(x, ids)
    x[1, 300] = float("nan")
    y = ex.forward_batched(x, ids)
    torch.cuda.synchronize()
    assert bool(torch.isnan(y[1]).all()), "every output of the token with the NaN is NaN"
    for t in (0, 2, 3):
        assert torch.equal(y[t], clean[t]) and bool(torch.isfinite(y[t]).all()), t
    # one row per slot: only that slot
    xs = rand_x((4, 2, K), torch.float16, 10)
    clean = ex.forward_batched(xs, ids)
    xs[1, 0, 7] = float("inf")
    xs[1, 0, 8] = float("-inf")
    y = ex.forward_batched(xs, ids)
    torch.cuda.synchronize()
    keep = torch.ones(4, 2, dtype=torch.bool, device=DEV)
    keep[1, 0] = False
    assert not bool(torch.isfinite(y[1, 0]).any()) and torch.equal(y[keep], clean[keep])


def test_opcheck_of_the_two_ops():
    N, K = SHAPES["three tiles, five waves idle"]
    ex = experts_of(N, K, 128, torch.float16, "tensor", True)
    ids = torch.tensor([[5, 2], [2, 7], [0, 5]], dtype=torch.int64, device=DEV)
    x = rand_x((3, K), torch.float16, 8)
    torch.library.opcheck(torch.ops.gemlite.experts_route.default, (ids, 16, ex.bias, ex.get_tensor_args(), ex.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))
    ws = ex.route(ids, 16).workspace
    torch.library.opcheck(torch.ops.gemlite.forward_experts_rows.default, (x, ids, ws, 16, ex.bias, ex.get_tensor_args(), ex.get_meta_args()),
                          test_utils=("test_schema", "test_faketensor"))
