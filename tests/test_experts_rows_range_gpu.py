"""gemlite_hip_experts_route + gemlite_hip_forward_experts_rows at scale and at the edges of their domain (run on a real MI355X via
`pytest -m gpu`); builders, id patterns and bookkeeping live in tests/test_experts_rows_range_cpu.py with their self-tests.

  part 1  the routing contract (tests/test_experts_rows_cpu.py::check_table, the sentinels of test_experts_rows_gpu.check_routing) for
          128 .. 4096 experts and up to 65535 slots: the prefix sum across waves, the second pass of the per-bucket and per-slot loops;
  part 2  forward at the same scale: every valid slot bit-identical to its row of the expert's own forced gemm_w4_rows_kernel launch
          (oracle_rows_fast, the twin of test_experts_rows_gpu.oracle_rows over ONE argsort), one x row per slot / per 8 slots / for all
          slots, a float64 check that does not lean on the forced launch, the MLP over 128 experts;
  part 3  strides and padding against the dense call, every 64-bit product at 4 GiB, the in-expert 32-bit offsets and the x extent at
          the largest values experts_rows_plan admits — bit for bit, every moved operand in 0xFF bytes that are unchanged afterwards
          (the layout rules of tests/test_addressing_limits_gpu.py::_place).
Out-of-range ids are a defined input with a defined result; no test here provokes a fault."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gemlite_amd import GemLiteExpertsMLP, _hip, core, experts as X
from tests import test_experts_rows_range_cpu as RR
from tests.test_addressing_limits_gpu import _all_ff, _check_and_clear, _ints
from tests.test_experts_gpu import DEV, GUARD, SENTINEL, guards_intact, make_experts, rand_x
from tests.test_experts_range_gpu import bits, place, strided
from tests.test_experts_rows_cpu import buckets_of
from tests.test_experts_rows_gpu import FORCED, check_outputs, check_routing, experts_of, forward_guarded, route_guarded

pytestmark = pytest.mark.gpu
F16, B16 = RR.F16, RR.B16
I32, I64 = torch.int32, torch.int64
TOL = {F16: 1e-3, B16: 4e-3}  # the rows-kernel gate of DESIGN §4 (test_experts_rows_gpu.test_arithmetic_against_float64)


@functools.lru_cache(maxsize=None)
def stack(E, dtype, zeros, bias, gs=RR.SMALL["gs"], N=RR.SMALL["N"], K=RR.SMALL["K"], seed=0):
    return RR.big_stack(E, N, K, gs, dtype, zeros, bias, seed, device=DEV)


def routed(ex, flat, ids_dtype, R):
    """route the flat ids on a guarded workspace and hold the table against the contract -> (ids [n], routing)"""
    ids = RR.ids_tensor(flat, ids_dtype, DEV)
    routing, buf, need = route_guarded(ex, ids, R)
    torch.cuda.synchronize()
    check_routing(buf, need, ids, R, ex.num_experts)
    return ids, routing


# ================================================================================================ part 1: the routing contract at scale
@pytest.mark.parametrize("ids_dtype", [I32, I64], ids=["int32", "int64"])
@pytest.mark.parametrize("R", RR.SCALE_R)
@pytest.mark.parametrize("E", RR.SCALE_E)
def test_the_routing_contract_at_scale(E, R, ids_dtype):
    ex = stack(E, F16, "int", False)
    ids64 = ids_dtype == I64
    pats = RR.patterns_for(E, R, ids64)
    pats.update({f"random, n = {n}": RR.random_ids(E, n, ids64) for n in RR.RANDOM_N})
    for name, flat in pats.items():
        try:
            routed(ex, flat, ids_dtype, R)
        except AssertionError as err:
            raise AssertionError(f"part 1, E = {E}, R = {R}, {name} ({len(flat)} slots): {err}") from err


# ================================================================================================ part 2: forward at scale
LAST = [None]  # the request of the last call, as sent
_named = set()


def launch_rows(ex, x2, ids, spx, routing, out_ptr, stride_out, targs=None, bias="own"):
    """one C call (the rows twin of test_experts_range_gpu.run): every stride is what the tensors' own strides say, slots_per_x_row and
    the output window are the caller's"""
    e = X._call_args(x2, ids, out_ptr, ex.bias if isinstance(bias, str) else bias, list(targs or ex.get_tensor_args()), ex.get_meta_args(), spx)
    e.stride_out_slot = stride_out
    r = X._rows_args(e, routing.rows_per_block, routing.workspace)
    rc = _hip.load().gemlite_hip_forward_experts_rows(C.byref(r), _hip.current_stream_handle(ids.device))
    assert rc == 0, _hip.status_string(rc)
    torch.cuda.synchronize()
    LAST[0] = r.experts
    return r.experts


def windowed_rows(ex, x2, ids, spx, routing, pad=0, targs=None, bias="own"):
    """the call into a window whose rows are `pad` elements apart beyond N, sentinels in the gaps and on both sides -> out [slots, N]
    (the rows twin of test_experts_range_gpu.windowed)"""
    n, N = ids.numel(), ex.out_features
    stride = N + pad
    buf = torch.full((GUARD + n * stride + GUARD,), SENTINEL, dtype=x2.dtype, device=DEV)
    launch_rows(ex, x2, ids, spx, routing, buf[GUARD:].data_ptr(), stride, targs, bias)
    v = buf[GUARD:GUARD + n * stride].view(n, stride)
    assert guards_intact(buf) and bool((v[:, N:] == SENTINEL).all()), "a store outside the output rows"
    return v[:, :N]


def oracle_rows_fast(ex, x2, row_of_slot, flat, R):
    """[slots, N] as test_experts_rows_gpu.oracle_rows gives it — every chunk of R slots of a populated expert through that expert's OWN
    forced gemm_w4_rows_kernel<R x16> launch on a matrix of R rows (+ the bias as `out += bias`: two roundings), invalid slots zero —
    with the slots grouped by ONE stable argsort (test_experts_rows_range_cpu.chunks_of) and one gather / one scatter for all chunks."""
    E, N = ex.num_experts, ex.out_features
    chunks = [(e, slots) for e, slots in RR.chunks_of(flat, E, R) if e < E]
    want = torch.zeros((len(flat), N), dtype=x2.dtype, device=DEV)
    if not chunks:
        return want
    slot_of = np.full((len(chunks), R), -1, dtype=np.int64)
    for i, (_, slots) in enumerate(chunks):
        slot_of[i, :len(slots)] = slots
    rows = np.asarray(row_of_slot)[np.where(slot_of >= 0, slot_of, slot_of[:, :1])]  # (a chunk's first row fills its empty rows)
    xm_all = x2[torch.from_numpy(rows.reshape(-1)).to(DEV)].view(len(chunks), R, -1)
    y_all = torch.empty((len(chunks), R, N), dtype=x2.dtype, device=DEV)
    for i, (e, _) in enumerate(chunks):
        lin = ex.expert(e)
        if (id(ex), R) not in _named:
            a = core._call_args(xm_all[i], lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, FORCED, False, 0x1000, (N, 1))
            name = _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode()
            assert name == f"gemm_w4_rows_kernel<{R}x16>", name
            _named.add((id(ex), R))
        y_all[i] = core._hip_matmul(xm_all[i], lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, FORCED)
    if ex.bias is not None:
        y_all += ex.bias[torch.tensor([e for e, _ in chunks], device=DEV)].unsqueeze(1)
    keep = torch.from_numpy(slot_of >= 0).to(DEV)
    want[torch.from_numpy(slot_of[slot_of >= 0]).to(DEV)] = y_all[keep]
    return want


def same_rows(out, want, flat, E, what):
    valid = torch.from_numpy(buckets_of(flat, E) < E).to(DEV)
    assert bool((out[~valid].view(torch.int16) == 0).all()), f"{what}: an invalid slot is not a row of zeros"
    same = (out.view(torch.int16) == want.view(torch.int16)).all(dim=1)
    assert bool(same.all()), (f"part 2, {what}: slots that differ from their expert's own rows launch", (~same).nonzero().flatten().tolist()[:8])


def float64_gate(ex, x2, row_of_slot, flat, out, slots, what):
    """DESIGN §4 per slot against float64 x @ dequantize(fp32).T (+ bias), which leans on no launch of the rows kernel:
    mean|err| / mean|y| < tol and |err| <= 10 tol mean|y| + 4 tol |y| -> the worst ratio to either form of the gate"""
    tol, worst = TOL[x2.dtype], 0.0
    for s in slots:
        e = int(flat[s])
        ref = x2[int(row_of_slot[s])].double() @ ex.expert(e).dequantize(torch.float32).double().T
        if ex.bias is not None:
            ref = ref + ex.bias[e].double()
        ref, y = ref.cpu().numpy(), out[s].double().cpu().numpy()
        err, scale = np.abs(y - ref), np.abs(ref).mean()
        ratio = max(err.mean() / scale / tol, float((err / (10 * tol * scale + 4 * tol * np.abs(ref))).max()))
        worst = max(worst, ratio)
        assert err.mean() / scale < tol and (err <= 10 * tol * scale + 4 * tol * np.abs(ref)).all(), (what, s, e, ratio)
    print(f"{what}: {len(slots)} slots against float64, worst ratio to the gate of DESIGN §4 = {worst:.3f}")
    return worst


SCALE_CASES = [  # (E, n, R, dtype, group, zeros, bias, ids dtype)
    (320, 1025, 16, F16, 64, "tensor", False, I64),
    (320, 1025, 32, B16, 32, "int", True, I32),      # groups of 32 with their largest block
    (1024, 4097, 32, B16, 64, "tensor", False, I32),
    (4096, 65535, 16, F16, 64, "tensor", True, I64),
    (4096, 65535, 64, F16, 64, "tensor", True, I32),
]


@pytest.mark.parametrize("E,n,R,dtype,gs,zeros,bias,ids_dtype", SCALE_CASES,
                         ids=[f"E{c[0]}-n{c[1]}-R{c[2]}-{str(c[3])[6:]}-g{c[4]}-z{c[5]}-b{int(c[6])}-{str(c[7])[6:]}" for c in SCALE_CASES])
def test_forward_at_scale_is_every_experts_own_rows_launch(E, n, R, dtype, gs, zeros, bias, ids_dtype):
    ex = stack(E, dtype, zeros, bias, gs)
    N, K = ex.out_features, ex.in_features
    flat = RR.random_ids(E, n, ids_dtype == I64, seed=1)
    ids, routing = routed(ex, flat, ids_dtype, R)
    x = rand_x((n, K), dtype, 11)  # every row differs: a slot that reads another slot's row shows
    what = f"E = {E}, n = {n}, R = {R}"
    # one x row per 8 slots (the planner takes the first ceil(n / 8) rows of x; n is no multiple of 8: through the C call)
    tok = np.arange(n) // 8
    want = oracle_rows_fast(ex, x, tok, flat, R)
    out = windowed_rows(ex, x, ids, 8, routing, pad=8)
    assert LAST[0].slots_per_x_row == 8 and LAST[0].n_slots == n and LAST[0].n_experts == E
    same_rows(out, want, flat, E, what + ", one x row per 8 slots")
    # one x row per slot, holding the same values: the same outputs
    xs = x[torch.from_numpy(tok).to(DEV)].contiguous()
    out, _ = forward_guarded(ex, xs, ids.view(n, 1), routing, pad=8)
    same_rows(out, want, flat, E, what + ", one x row per slot")
    if (E, R) == (4096, 16):
        # low, middle and highest expert ids among 64 slots across the launch
        valid = np.nonzero(buckets_of(flat, E) < E)[0]
        by_id = valid[np.argsort(flat[valid], kind="stable")]
        picks = sorted(set(by_id[np.linspace(0, len(by_id) - 1, 64).astype(int)].tolist()))
        assert len(picks) == 64 and flat[picks].min() == flat[valid].min() <= 1 and flat[picks].max() == flat[valid].max() >= E - 2
        float64_gate(ex, xs, np.arange(n), flat, out, picks, what)
        # ONE x row for everything: E + 1 distinct rows, indexed by bucket
        per_bucket = torch.cat((oracle_rows_fast(ex, x[:1], np.zeros(E, dtype=np.int64), np.arange(E), R), torch.zeros((1, N), dtype=dtype, device=DEV)))
        assert len(np.unique(bits(per_bucket), axis=0)) == E + 1
        want1 = per_bucket[torch.from_numpy(buckets_of(flat, E)).to(DEV)]
        for spx in (65535, 1 << 40):
            out = windowed_rows(ex, x, ids, spx, routing)
            assert LAST[0].slots_per_x_row == spx
            same_rows(out, want1, flat, E, what + f", slots_per_x_row = {spx}")


def test_the_mlp_over_128_experts():
    """GemLiteExpertsMLP.forward_batched, E = 128, top_k = 8, T = 40: bit for bit the two forward_batched calls with the torch ops between,
    and within the §4 gate of GemLiteExpertsMLP.forward (whose decode kernels sum K in another order)."""
    E, T, top_k, hidden, inter, dtype = 128, 40, 8, 256, 256, F16
    mlp = GemLiteExpertsMLP(stack(E, dtype, "tensor", False, 64, 2 * inter, hidden, seed=1), stack(E, dtype, "tensor", False, 64, hidden, inter, seed=2))
    g = torch.Generator().manual_seed(7)
    ids = torch.stack([torch.randperm(E, generator=g)[:top_k] for _ in range(T)]).to(DEV)
    w = torch.softmax(torch.randn(T, top_k, generator=g), -1).to(DEV)
    x = rand_x((T, hidden), dtype, 8)
    out = mlp.forward_batched(x, ids, w)
    R = mlp.rows_per_block(ids.numel())
    routing = mlp.gate_up.route(ids, R)
    y = mlp.gate_up.forward_batched(x, ids, routing).float()
    h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(dtype)
    d = mlp.down.forward_batched(h, ids, routing)
    want = (d.float() * w.unsqueeze(-1)).sum(-2).to(dtype)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    flat = ids.reshape(-1).cpu().numpy()
    same_rows(d.reshape(-1, hidden), oracle_rows_fast(mlp.down, h.reshape(-1, inter), np.arange(T * top_k), flat, R), flat, E, "MLP down")
    ref = mlp(x, ids, w).double()
    err, scale, tol = (out.double() - ref).abs(), float(ref.abs().mean()), TOL[dtype]
    print(f"MLP forward_batched vs forward, E = {E}: rel={float(err.mean()) / scale:.3e} max={float(err.max()):.3e} "
          f"(ratio to the gate {max(float(err.mean()) / scale / tol, float((err / (10 * tol * scale + 4 * tol * ref.abs())).max())):.3f})")
    assert float(err.mean()) / scale < tol and bool((err <= 10 * tol * scale + 4 * tol * ref.abs()).all())


# ================================================================================================ part 3: strides, padding, addressing edges
def mixed_ids(E, ids_dtype):
    """12 slots, top_k = 2: repeats inside a token and across tokens, experts without a slot, every kind of invalid id"""
    bad = RR.invalid_ids(3, E, ids_dtype == I64).tolist()
    return torch.tensor([[5, 2], [2, bad[0]], [0, 5], [bad[1], 1], [2, 2], [7, bad[2]]], dtype=ids_dtype, device=DEV)


@pytest.mark.parametrize("dtype,gs,ids_dtype", [(F16, 64, I64), (B16, 32, I32)], ids=["fp16-g64-int64", "bf16-g32-int32"])
def test_rows_strides_and_padding_give_the_dense_result_bit_for_bit(dtype, gs, ids_dtype):
    N, K, R = 256, 768, 16
    ex = experts_of(N, K, gs, dtype, "tensor", True)
    ids = mixed_ids(ex.num_experts, ids_dtype)
    _, routing = routed(ex, ids.reshape(-1).cpu().numpy(), ids_dtype, R)
    W_q, sc, zr = ex.get_tensor_args()
    R8, G = K // 8, K // gs
    for shared in (False, True):
        x = rand_x((6, K) if shared else (12, K), dtype, 81 + shared)
        spx = 2 if shared else 1
        dense_out = windowed_rows(ex, x, ids, spx, routing)
        check_outputs(ex, x if shared else x.view(6, 2, K), ids, dense_out, R)
        dense = bits(dense_out)
        what = f"part 3, {dtype} shared x {shared}"
        assert np.array_equal(bits(windowed_rows(ex, x, ids, spx, routing, pad=24)), dense), f"{what}: stride_out_slot = N + 24"
        assert LAST[0].stride_out_slot == N + 24
        for j in (1, 3):  # stride_x_row = K + 8 j, NaN between the rows
            xv, xbuf = strided(x, (K + 8 * j, 1))
            before = xbuf.clone()
            got = bits(windowed_rows(ex, xv, ids, spx, routing))
            assert LAST[0].stride_x_row == K + 8 * j
            assert np.array_equal(got, dense) and torch.equal(xbuf, before), f"{what}: stride_x_row = K + {8 * j}"
        for j in (1, 2):  # padding between experts: 16 j bytes (W), 8 j bytes (metadata), 2 j bytes (bias)
            Wv, wbuf = strided(W_q, (R8 * N + 4 * j, N, 1))
            sv, sbuf = strided(sc, (G * N + 4 * j, N, 1))
            zv, zbuf = strided(zr, (G * N + 4 * j, N, 1))
            bv, bbuf = strided(ex.bias, (N + j, 1))
            before = [b.clone() for b in (wbuf, sbuf, zbuf, bbuf)]
            got = bits(windowed_rows(ex, x, ids, spx, routing, targs=(Wv, sv, zv), bias=bv))
            sent = LAST[0]
            assert (sent.stride_expert_w, sent.stride_expert_meta, sent.stride_expert_bias) == (R8 * N * 4 + 16 * j, G * N * 2 + 8 * j, N * 2 + 2 * j)
            assert np.array_equal(got, dense), f"{what}: experts {j} steps of padding apart"
            assert all(torch.equal(a, b) for a, b in zip(before, (wbuf, sbuf, zbuf, bbuf)))
        # rows of the weights and of the metadata wider than N
        Wv, wbuf = strided(W_q, (R8 * (N + 8), N + 8, 1))
        sv, sbuf = strided(sc, (G * (N + 12), N + 12, 1))
        zv, zbuf = strided(zr, (G * (N + 12), N + 12, 1))
        before = [b.clone() for b in (wbuf, sbuf, zbuf)]
        got = bits(windowed_rows(ex, x, ids, spx, routing, targs=(Wv, sv, zv)))
        assert (LAST[0].layer.stride_wk, LAST[0].layer.stride_meta_g) == (N + 8, N + 12)
        assert np.array_equal(got, dense), f"{what}: stride_wk = N + 8, stride_meta_g = N + 12"
        assert all(torch.equal(a, b) for a, b in zip(before, (wbuf, sbuf, zbuf)))
    # stride_x_row = 0: every slot reads row 0
    x = rand_x((1, K), dtype, 83)
    dense = bits(windowed_rows(ex, x.expand(12, K).contiguous(), ids, 1, routing))
    for spx in (1, 2):
        xv = x.expand(12 // spx, K)
        assert xv.stride(0) == 0
        got = bits(windowed_rows(ex, xv, ids, spx, routing))
        assert LAST[0].stride_x_row == 0 and np.array_equal(got, dense), f"part 3, {dtype}: stride_x_row = 0, {spx} slots per row"


FAR = ["stride_expert_w", "stride_expert_meta", "stride_expert_bias", "stride_out_slot", "stride_wk", "stride_meta_g"]


@pytest.mark.parametrize("field", FAR)
def test_rows_every_64_bit_stride_at_4_gib_and_the_in_expert_32_bit_edge(field):
    """Two experts 4 GiB apart (weights, metadata, bias: the 64-bit products `expert * stride`), three output rows 2^32 - 4 bytes apart
    (`slot * stride_out_slot`: the third row lies beyond 2^32 bytes), and rows of the weights / of the metadata at the largest stride
    experts_rows_plan admits (the 32-bit offsets inside an expert; the two experts interleave).  One allocation per case."""
    N, K, gs, R, dtype = RR.ROWS_EDGE_N, RR.ROWS_EDGE_K, RR.ROWS_EDGE_GS, 16, F16
    ex = experts_of_two(N, K, gs, dtype)
    W_q, sc, zr = ex.get_tensor_args()
    out_stride = (1 << 31) - 2
    moved = {"stride_expert_w": (W_q, (1 << 30, N, 1)), "stride_expert_meta": (sc, (1 << 31, N, 1)), "stride_expert_bias": (ex.bias, (1 << 31, 1)),
             "stride_wk": (W_q, (N, RR.rows_edge_stride_wk(), 1)), "stride_meta_g": (sc, (N, RR.rows_edge_stride_meta_g(), 1))}
    expect = {"stride_expert_w": 1 << 32, "stride_expert_meta": 1 << 32, "stride_expert_bias": 1 << 32, "stride_out_slot": out_stride,
              "stride_wk": RR.rows_edge_stride_wk(), "stride_meta_g": RR.rows_edge_stride_meta_g()}[field]
    three = field == "stride_out_slot"
    ids = torch.tensor([[1], [0], [1]] if three else [[1, 0], [1, 1]], device=DEV)
    spx = ids.shape[-1]
    x = rand_x((3 if three else 2, K), dtype, 100)
    _, routing = routed(ex, ids.reshape(-1).cpu().numpy(), I64, R)
    dense_out = windowed_rows(ex, x, ids, spx, routing)
    check_outputs(ex, x, ids, dense_out, R)
    dense = bits(dense_out)
    assert len(np.unique(dense, axis=0)) == 3  # (two slots of expert 1 on one x row agree; nothing else does)
    torch.cuda.empty_cache()
    v = big = None
    try:
        if three:
            v, big = place(torch.empty((3, N), dtype=dtype, device=DEV), (out_stride, 1))
            _ints(v).fill_(-1)
            launch_rows(ex, x, ids, spx, routing, v.data_ptr(), out_stride)
            got = bits(v)
            _ints(v).fill_(-1)
            assert _all_ff(big), "part 3: a store outside the three output rows"
        else:
            targs = [W_q, sc, zr]
            v, big = place(*moved[field])
            if field in ("stride_expert_w", "stride_wk"):
                targs[0] = v
            elif field in ("stride_expert_meta", "stride_meta_g"):
                targs[1] = v
            got = bits(windowed_rows(ex, x, ids, spx, routing, targs=targs, bias=v if field == "stride_expert_bias" else ex.bias))
        sent = LAST[0].layer if field in ("stride_wk", "stride_meta_g") else LAST[0]
        assert getattr(sent, field) == expect, (field, getattr(sent, field), expect)
        assert np.array_equal(got, dense), f"part 3: {field} = {expect}"
        if not three:
            _check_and_clear(v, big, moved[field][0], field)
    finally:
        v = big = None
        torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def experts_of_two(N, K, gs, dtype):
    return make_experts(N, K, gs, dtype, "int", True, n=2)


def test_rows_the_x_extent_just_below_2_gib():
    """513 x rows (2^21 - 8) elements apart, K = 2048: an extent of 2^31 - 4096 bytes, the largest request
    test_experts_rows_cpu.test_the_edges_of_the_domain_are_inside accepts.  Every row is live; slots read row 0, row 256 and row 512."""
    N, K, gs, R, dtype = 16, 2048, 128, 16, F16
    n, spx, stride = 2 * 512 + 1, 2, (1 << 21) - 8
    ex = experts_of(N, K, gs, dtype, "tensor", False)
    E = ex.num_experts
    flat = RR.random_ids(E, n, True, seed=2)
    flat[[0, 1, 512, 513, 1024]] = [3, 6, 0, 7, 5]  # rows 0, 256 and 512 each have a valid slot
    ids, routing = routed(ex, flat, I64, R)
    x = rand_x((513, K), dtype, 110)
    assert (512 * stride + K) * 2 == (1 << 31) - 4096
    dense_out = windowed_rows(ex, x, ids, spx, routing)
    same_rows(dense_out, oracle_rows_fast(ex, x, np.arange(n) // spx, flat, R), flat, E, "the x extent, dense")
    dense = bits(dense_out)
    torch.cuda.empty_cache()
    xv = xbuf = None
    try:
        xv, xbuf = strided(x, (stride, 1))
        assert xbuf.numel() == (1 << 31) - 4096
        got = bits(windowed_rows(ex, xv, ids, spx, routing))
        sent = LAST[0]
        assert (sent.stride_x_row, sent.slots_per_x_row, sent.n_slots, sent.layer.K) == (stride, spx, n, K)
        bad = np.nonzero((got != dense).any(1))[0]
        assert bad.size == 0, ("part 3, the x extent: slots that differ from the dense call", bad[:8], (bad[:8] // spx))
        _check_and_clear(xv, xbuf, x, "x at its largest extent")
    finally:
        xv = xbuf = None
        torch.cuda.empty_cache()
