"""The experts launches across magnitudes, non-finite inputs, strides and the corners of their domain (run on a real MI355X via
`pytest -m gpu`): gemlite_hip_forward_experts and gemlite_hip_forward_experts_fused with the GLU and COMBINE epilogues, which no sweep over
tests/test_abi_bounds_cpu.py::CASES reaches.  Tables, builders and gates live in tests/test_experts_range_cpu.py with their self-tests.

Every numeric check has two stages, and neither takes its expectation from the code under test:
  members    the unfused launch, slot by slot, against float64 x @ W.T (+ bias) rebuilt from the codes, scales and zeros kept on the CPU:
             test_magnitude_range_gpu.row_gate with the decode kernels' tolerance; where the single-layer planner names
             gemv_w4_decode3_kernel for the expert, the slot is also bit-identical to that launch (test_experts_gpu.oracle_slot);
  epilogues  the fused launch against float64 arithmetic on the unfused launch's rounded outputs: |out - ref| <= 1 ulp (GLU),
             <= 1 ulp + top_k 2^-23 sum |w y| (COMBINE), the bounds derived in tests/test_experts_fused_gpu.py, elementwise.
Layout checks (strides, padding, 64-bit strides, the in-expert 32-bit edge) are bit-identical to the dense call of the same request, with
sentinels around every output row and 0xFF around every moved input (the layout rules of tests/test_addressing_limits_gpu.py::_place)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, core, experts as X
from tests import test_experts_range_cpu as R
from tests import test_magnitude_range_gpu as MR
from tests import test_nonfinite_cpu as NF
from tests.test_addressing_limits_gpu import BASE, MAX_ALLOC, REACH, TAIL, _all_ff, _check_and_clear, _ints
from tests.test_experts_fused_gpu import COMBINE, GLU, ROWS, check_combine, check_glu, f64, launch_fused, ulp
from tests.test_experts_gpu import DEV, GUARD, SENTINEL, TUNING, guards_intact, launch_guarded, oracle_slot

pytestmark = pytest.mark.gpu
E, F16, B16 = R.E, R.F16, R.B16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "experts_glu_deep_gates.npz")


@functools.lru_cache(maxsize=None)
def built(N, K, gs, dtype, zeros="tensor", bias=False, n=E, factor=1.0, scales=True, fma=True):
    """(the experts' numbers on the CPU, the GemLiteExperts on the GPU), built once per process and never changed"""
    h = R.host_experts(N, K, gs, dtype, zeros, bias, n=n, factor=factor, scales=scales, fma=fma)
    return h, R.to_experts(h, DEV)


def built_row(N, K, row, **kw):
    dtype, gs, zeros, bias, _ = ROWS[row]
    return built(N, K, gs, dtype, zeros, bias, **kw)


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def flat(ids):
    return ids.reshape(-1).tolist()


def rand_x(shape, dtype, seed, amp=0.5):
    return (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * amp).to(dtype).to(DEV)


def single_layer(ex, e, x_row):
    """expert e's own decode3 launch on x_row, or None where the single-layer planner names another kernel for it"""
    lin = ex.expert(e)
    x2 = x_row.reshape(1, -1)
    a = core._call_args(x2, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, TUNING, False, 0x1000, (lin.W_q.shape[1], 1))
    if not _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode().startswith("gemv_w4_decode3_kernel"):
        return None
    return oracle_slot(ex, e, x_row)


def check_members(h, ex, x2, ids, spx, y, what, limit=MR.Y_LIMIT, identity=False):
    """Stage 1 on y [slots, N] of the unfused launch; -> the number of slots compared with their own single-layer launch."""
    y_ref = R.ref_slots(h, x2, ids, spx)
    assert np.isfinite(y_ref).all() and float(np.abs(y_ref).max()) < limit, (what, float(np.abs(y_ref).max()))
    code, tol = R.OUT_CODE[h.dtype], R.tol_for(h.dtype)
    recs = MR.row_gate(f64(y), y_ref, code, tol)
    worst = max((r["rel_mean"] / (tol + MR.QUANTUM[code] / r["mean_abs_ref"]) for r in recs if r["rel_mean"] is not None), default=0.0)
    print(f"members {what}: worst mean relative error / bound = {worst:.3f}")
    bad = [dict(r, id=ids[r["row"]]) for r in recs if not r["ok"]]
    assert not bad, (what, bad[:4])
    same = 0
    if identity:
        for s, e in enumerate(ids):
            want = single_layer(ex, e, x2[s // spx]) if 0 <= e < h.n else None
            if want is not None:
                assert np.array_equal(bits(y[s]), bits(want)), (what, s, e)
                same += 1
    return same


# ================================================================================================ part 1: magnitudes per slot
@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_every_slot_of_the_unfused_launch_holds_its_own_activation_profile(shape, row):
    N, K = shape
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    ids = torch.tensor(R.MAG_IDS, dtype=ids_dtype, device=DEV)
    same = 0
    for li, rows in enumerate(R.mag_launches(ids.numel(), dtype)):
        x = R.profile_x(rows, K, dtype, 10 + li).to(DEV)
        y, buf = launch_guarded(ex, x.view(3, 2, K), ids)
        assert guards_intact(buf)
        same += check_members(h, ex, x, flat(ids), 1, y, f"{N}x{K} row {row} launch {li} {rows}", identity=True)
    assert same == 2 * ids.numel() or shape == R.SHAPES[3], same  # (32 x 4352 is the one shape the existing suite does not pin to decode3)


@pytest.mark.parametrize("shape", R.GLU_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("row", range(len(ROWS)))
def test_glu_holds_one_ulp_for_every_profile(shape, row):
    N, K = shape
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    ids = torch.tensor(R.MAG_IDS, dtype=ids_dtype, device=DEV)
    for li, rows in enumerate(R.mag_launches(ids.numel(), dtype)):
        x = R.profile_x(rows, K, dtype, 10 + li).to(DEV)
        y, buf = launch_guarded(ex, x.view(3, 2, K), ids)
        assert guards_intact(buf)
        check_members(h, ex, x, flat(ids), 1, y, f"GLU {N}x{K} row {row} launch {li}")
        out, buf = launch_fused(ex, GLU, x.view(3, 2, K), ids)
        assert guards_intact(buf)
        check_glu(out, y, dtype, f"{N}x{K} row {row} launch {li} {rows}")


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("top_k", R.COMBINE_TOP_KS)
def test_combine_holds_its_bound_where_amplitudes_1e_4_and_10_share_a_block(shape, top_k):
    N, K = shape
    row = (R.SHAPES.index(shape) + top_k) % len(ROWS)
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    T = 2 if top_k == 3 else 1
    ids = R.combine_ids(top_k, T, 40 + top_k).to(ids_dtype).to(DEV)
    for li, rows in enumerate(R.mag_launches(T * top_k, dtype)):
        x = R.profile_x(rows, K, dtype, 30 + li).to(DEV)
        y, buf = launch_guarded(ex, x.view(T, top_k, K), ids)
        assert guards_intact(buf)
        check_members(h, ex, x, flat(ids), 1, y, f"COMBINE {N}x{K} top_k {top_k} launch {li}")
        y = y.view(T, top_k, N)
        for wdt in (torch.float32, dtype):
            w = R.combine_weights(T, top_k, 50 + li).to(wdt).to(DEV)
            out, buf = launch_fused(ex, COMBINE, x.view(T, top_k, K), ids, w)
            assert guards_intact(buf)
            check_combine(out, y, w, dtype, f"{N}x{K} top_k {top_k} launch {li} weights {wdt}")
        # a one-hot weight on the smallest and on the largest member: that member's rounded output, whatever shares the block with it
        for name in ("amp1e-4", "amp10"):
            k0 = rows.index(name) % top_k
            t0 = rows.index(name) // top_k
            w = torch.zeros(T, top_k, device=DEV)
            w[:, k0] = 1
            out, buf = launch_fused(ex, COMBINE, x.view(T, top_k, K), ids, w)
            assert guards_intact(buf) and torch.equal(out, y[:, k0, :]), (name, k0)
            assert float(out[t0].float().abs().max()) > 0


@pytest.mark.parametrize("which", ["small", "large"])
@pytest.mark.parametrize("row", [0, 1])
def test_all_three_kernels_hold_across_weight_scales(row, which):
    N, K = R.SCALE_SHAPE
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    factor = MR.scale_factors(dtype)[which == "large"]
    h, ex = built_row(N, K, row, factor=factor)
    ids = torch.tensor(R.MAG_IDS, dtype=ids_dtype, device=DEV)
    rows, = R.mag_launches(6, dtype, MR.SCALE_PROFILES)
    x = R.profile_x(rows, K, dtype, 20).to(DEV)
    y, buf = launch_guarded(ex, x.view(3, 2, K), ids)
    assert guards_intact(buf)
    same = check_members(h, ex, x, flat(ids), 1, y, f"scales x {factor:g} row {row}", identity=True)
    assert same == 6
    glu_rows = R.glu_scale_slots(dtype, which)
    xg, idg = x[glu_rows].view(-1, 1, K), ids.view(-1, 1)[glu_rows]
    out, buf = launch_fused(ex, GLU, xg, idg)
    assert guards_intact(buf)
    with np.errstate(over="ignore"):  # (exp(-gate) of the float64 reference: gates reach -780 under the large factor)
        check_glu(out, y[glu_rows], dtype, f"scales x {factor:g} row {row}")
    w = R.combine_weights(2, 3, 21).to(DEV)
    out, buf = launch_fused(ex, COMBINE, x.view(2, 3, K), ids.view(2, 3), w)
    assert guards_intact(buf)
    check_combine(out, y.view(2, 3, N), w, dtype, f"scales x {factor:g} row {row}")


# ================================================================================================ part 2: deep gates
@pytest.mark.parametrize("row", R.DEEP_ROWS)
def test_glu_holds_one_ulp_where_the_gate_lies_below_minus_89(row):
    """silu(g) for g in [-97, -89] is a bf16 number (normal down to about -92) although exp(-g) is +Inf in fp32: the epilogue switches to
    g exp(g / 2) exp(g / 2) below -88 (gemv_decode.hip).  bf16 before that change, on an MI355X: worst |out - ref| = 254.7 ulp, at exactly
    these gates (the result was -0); 0.500 ulp after it.  Every output whose gate is above -88 is bit-identical to the recording made before it
    (tests/golden/experts_glu_deep_gates.npz), and so is the unfused launch."""
    N, K = R.DEEP_SHAPE
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    x = R.deep_x(h).to(DEV)
    ids = torch.tensor(R.DEEP_IDS, dtype=ids_dtype, device=DEV)
    y, buf = launch_guarded(ex, x, ids)
    assert guards_intact(buf)
    check_members(h, ex, x, flat(ids), 2, y, f"deep gates row {row}")
    gate = f64(y)[:, :N // 2]
    print(f"deep gates row {row}: {R.deep_count(gate)} gate values of the unfused launch in [-97, -89]")
    assert R.deep_count(gate) >= 8 and gate[0].max() >= 100 and gate[0].min() <= -100
    out, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    rec = np.load(GOLDEN)
    assert np.array_equal(bits(y), rec[f"y{row}"]), "the unfused launch differs from the recording"
    keep = gate > -88.0
    assert keep.sum() > gate.size // 2 and np.array_equal(bits(out)[keep], rec[f"out{row}"][keep]), "an output whose gate is above -88 changed"
    check_glu(out, y, dtype, f"deep gates row {row}")


# ================================================================================================ part 3: non-finite inputs
@functools.lru_cache(maxsize=None)
def _poisoned(row):
    """the clean launch and one launch per poisoned slot of all three kernels (x per slot, 6 slots, top_k = 2 for COMBINE), run once"""
    N, K = R.NONFINITE_SHAPE
    dtype, gs, _, _, ids_dtype = ROWS[row]
    h, ex = built_row(N, K, row)
    ids = torch.tensor(R.MAG_IDS, dtype=ids_dtype, device=DEV)
    w = R.combine_weights(3, 2, 60).to(DEV)
    x = rand_x((6, K), dtype, 61)

    def three(xs, i=ids, ww=w):
        xs = xs.view(3, 2, K)
        return dict(plain=launch_guarded(ex, xs, i), glu=launch_fused(ex, GLU, xs, i), combine=launch_fused(ex, COMBINE, xs, i, ww))

    def keep(res):
        assert all(guards_intact(buf) for _, buf in res.values())
        return {k: (bits(out), f64(out)) for k, (out, _) in res.items()}

    out = dict(clean=keep(three(x)), runs=[], dtype=dtype)
    for li, (r, kind) in enumerate(NF.launches(6)):
        xp, ks = NF.poison(x, r, kind, gs, seed=600 + li)
        run = dict(r=r, kind=kind, res=keep(three(xp)))
        # COMBINE with the poisoned slot's id invalid, against the clean x with that weight 0
        broken, zeroed = ids.clone(), w.clone()
        broken.view(-1)[r], zeroed.view(-1)[r] = -1, 0
        run["invalid"] = keep(three(xp, broken))["combine"][0]
        run["weight0"] = keep(three(x, ids, zeroed))["combine"][0]
        out["runs"].append(run)
    return out


@pytest.mark.parametrize("row", [1, 2])
def test_a_poisoned_slot_leaves_every_other_slot_and_token_bit_identical(row):
    L = _poisoned(row)
    for run in L["runs"]:
        r = run["r"]
        for kind, rr in (("plain", r), ("glu", r), ("combine", r // 2)):
            changed = NF.isolation_gate(run["res"][kind][0], L["clean"][kind][0], rr)
            assert changed == [], (kind, run["kind"], r, changed)


@pytest.mark.parametrize("row", [1, 2])
def test_a_poisoned_slot_comes_back_non_finite_and_an_invalid_id_hides_it_exactly(row):
    L = _poisoned(row)
    for run in L["runs"]:
        r = run["r"]
        for kind, rr in (("plain", r), ("glu", r), ("combine", r // 2)):
            assert NF.visible_gate(run["res"][kind][1][rr]) == 0, (kind, run["kind"], r, NF.visible_gate(run["res"][kind][1][rr]))
        assert np.array_equal(run["invalid"], run["weight0"]), (run["kind"], r)
        assert np.isfinite(run["invalid"].view(np.float16) if L["dtype"] == F16 else run["invalid"].astype(np.int32) << 16).all()


@pytest.mark.parametrize("dtype", [F16, B16], ids=["fp16", "bf16"])
def test_glu_of_an_infinite_gate(dtype):
    """gate +Inf: sign(up) Inf, NaN where up = 0; gate -Inf: NaN (-Inf / (1 + Inf), what include/gemlite_hip.h's formula and torch's
    silu give).  The gate and up values are hand-made (test_experts_range_cpu.glu_class_experts) and asserted on the unfused launch."""
    h = R.glu_class_experts(dtype)
    ex = R.to_experts(h, DEV)
    x = torch.full((1, 256), R.GLU_CLASS[dtype]["c"]).to(dtype).to(DEV)
    ids = torch.tensor([[0]], device=DEV)
    y, buf = launch_guarded(ex, x, ids)
    assert guards_intact(buf)
    g, u = f64(y)[0, :16], f64(y)[0, 16:]
    assert np.array_equal(g, np.where(np.arange(16) % 2 == 0, np.inf, -np.inf)), g
    assert np.array_equal(u, np.array([1.5, -2.25, 0.0])[np.arange(16) % 3]), u
    out, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    want, got = R.glu_class_expected(g, u), f64(out)[0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(want)], want[~np.isnan(want)]), (got, want)
    assert np.isnan(want).sum() == 8 + 3 and (want == np.inf).sum() == 3 and (want == -np.inf).sum() == 2


@pytest.mark.parametrize("kind", ["combine", "glu"])
def test_fp16_epilogue_outputs_overflow_to_inf_and_stay_finite_below(kind):
    N, K = R.OVERFLOW_SHAPE
    h, ex = built_row(N, K, 0)
    x = R.overflow_x(kind, K).to(DEV)
    ids = torch.tensor(R.OVERFLOW_IDS, device=DEV)
    y, buf = launch_guarded(ex, x, ids)
    assert guards_intact(buf) and bool(torch.isfinite(y).all())
    check_members(h, ex, x.view(6, K), flat(ids), 1, y, f"overflow {kind}", limit=NF.F16_MAX)
    if kind == "glu":
        out, buf = launch_fused(ex, GLU, x, ids)
        ref = R.glu_f64(f64(y))
        bound = ulp(ref, F16)
    else:
        w = torch.tensor([R.OVERFLOW_W] * 2, dtype=torch.float16, device=DEV)
        out, buf = launch_fused(ex, COMBINE, x, ids, w)
        prod = np.asarray(R.OVERFLOW_W)[None, :, None] * f64(y).reshape(2, 3, N)
        ref = prod.sum(1)
        bound = ulp(ref, F16) + 3 * 2.0 ** -23 * np.abs(prod).sum(1)
    assert guards_intact(buf)
    shares = NF.overflow_shares(ref, R.OVERFLOW_TOL)
    assert NF.shares_ok(shares), shares  # the reference first: every row straddles the threshold
    recs = R.epilogue_overflow_gate(f64(out), ref, bound)
    print(f"overflow {kind}: " + ", ".join(f"row {r['row']}: {r['over']} over / {r['under']} under" for r in recs))
    assert all(r["ok"] for r in recs), [r for r in recs if not r["ok"]]


def test_bf16_slots_of_amplitude_2_to_the_40_and_minus_40_share_a_combine_block():
    N, K = R.SHAPES[1]
    h, ex = built_row(N, K, 1)
    x = NF.make_wide_x(NF.WIDE_PROFILES * 2, K, 7).to(DEV)
    ids = torch.tensor([[5, 2, 6], [1, 7, 0]], dtype=torch.int32, device=DEV)
    y, buf = launch_guarded(ex, x.view(2, 3, K), ids)
    assert guards_intact(buf)
    check_members(h, ex, x, flat(ids), 1, y, "wide", limit=NF.WIDE_Y_LIMIT)
    y = y.view(2, 3, N)
    w = R.combine_weights(2, 3, 70).to(DEV)
    out, buf = launch_fused(ex, COMBINE, x.view(2, 3, K), ids, w)
    assert guards_intact(buf)
    check_combine(out, y, w, B16, "wide")
    for k0 in range(3):  # each member on its own: the 2^-40 one is not lost beside the 2^40 one
        w = torch.zeros(2, 3, device=DEV)
        w[:, k0] = 1
        out, buf = launch_fused(ex, COMBINE, x.view(2, 3, K), ids, w)
        assert guards_intact(buf) and torch.equal(out, y[:, k0, :]) and float(out.float().abs().max()) > 0, k0


# ================================================================================================ part 4: strides and padding
KINDS = ("plain", "glu", "combine")
LAST = [None]  # the request of the last call, as sent


def run(kind, targs, bias, meta, x2, ids, spx, out_ptr, stride_out, w=None):
    """one C call: every stride is what the tensors' own strides say (experts._call_args), the output goes where the caller says"""
    e = X._call_args(x2, ids, out_ptr, bias, list(targs), meta, spx)
    e.stride_out_slot = stride_out
    lib, st = _hip.load(), _hip.current_stream_handle(ids.device)
    if kind == "plain":
        rc = lib.gemlite_hip_forward_experts(C.byref(e), st)
    else:
        f = X._fused_args(e, GLU) if kind == "glu" else X._fused_args(e, COMBINE, w.data_ptr(), X.TORCH_TO_DTYPE[w.dtype].value, ids.shape[-1])
        rc = lib.gemlite_hip_forward_experts_fused(C.byref(f), st)
    assert rc == 0, (kind, _hip.status_string(rc))
    torch.cuda.synchronize()
    LAST[0] = e
    return e


def out_shape(kind, ids, N):
    return (ids.numel(), N // 2) if kind == "glu" else ((ids.numel(), N) if kind == "plain" else (ids.numel() // ids.shape[-1], N))


def windowed(kind, ex, x2, ids, spx, w, targs=None, bias="own", pad=0):
    """the call into a window whose rows are `pad` elements apart beyond their width, sentinels in the gaps and on both sides -> bits"""
    rows, width = out_shape(kind, ids, ex.out_features)
    stride = width + pad
    buf = torch.full((GUARD + rows * stride + GUARD,), SENTINEL, dtype=x2.dtype, device=DEV)
    run(kind, targs or ex.get_tensor_args(), ex.bias if isinstance(bias, str) else bias, ex.get_meta_args(), x2, ids, spx,
        buf[GUARD:].data_ptr(), stride, w)
    v = buf[GUARD:GUARD + rows * stride].view(rows, stride)
    assert guards_intact(buf) and bool((v[:, width:] == SENTINEL).all()), f"{kind}: a store outside the output rows"
    return bits(v[:, :width])


def strided(t, strides):
    """(a view of t's values with `strides` (elements) inside a buffer of 0xFF bytes, the buffer)"""
    n = sum((d - 1) * s for d, s in zip(t.shape, strides)) + 1
    buf = torch.full((n * t.element_size(),), 0xFF, dtype=torch.uint8, device=DEV)
    v = buf.view(t.dtype).as_strided(tuple(t.shape), tuple(strides))
    _ints(v).copy_(_ints(t))
    return v, buf


@pytest.mark.parametrize("row", [1, 2])
def test_strides_and_padding_give_the_dense_result_bit_for_bit(row):
    N, K = 256, 768
    dtype, gs, zeros, _, ids_dtype = ROWS[row]
    h, ex = built_row(N, K, row)
    ids = torch.tensor(R.MAG_IDS, dtype=ids_dtype, device=DEV)
    w = R.combine_weights(3, 2, 80).to(DEV)
    W_q, sc, zr = ex.get_tensor_args()
    R8, G = K // 8, K // gs
    for shared in (False, True):
        x = rand_x((3, K) if shared else (6, K), dtype, 81 + shared)
        spx = 2 if shared else 1
        for kind in KINDS:
            dense = windowed(kind, ex, x, ids, spx, w)
            what = f"{kind} row {row} shared x {shared}"
            assert np.array_equal(windowed(kind, ex, x, ids, spx, w, pad=24), dense), f"{what}: stride_out_slot = width + 24"
            for j in (1, 3):  # stride_x_row = K + 8 j, NaN between the rows
                xv, xbuf = strided(x, (K + 8 * j, 1))
                before = xbuf.clone()
                assert np.array_equal(windowed(kind, ex, xv, ids, spx, w), dense) and torch.equal(xbuf, before), f"{what}: stride_x_row = K + {8 * j}"
            for j in (1, 2):  # padding between experts: stride_expert_w + 16 j, stride_expert_meta + 8 j, stride_expert_bias + 2 j bytes
                Wv, wbuf = strided(W_q, (R8 * N + 4 * j, N, 1))
                sv, sbuf = strided(sc, (G * N + 4 * j, N, 1))
                zv, zbuf = strided(zr, (G * N + 4 * j, N, 1)) if zr.dim() == 3 else (zr, zr)
                bv, bbuf = strided(ex.bias, (N + j, 1))
                before = [b.clone() for b in (wbuf, sbuf, zbuf, bbuf)]
                got = windowed(kind, ex, x, ids, spx, w, targs=(Wv, sv, zv), bias=bv)
                assert np.array_equal(got, dense), f"{what}: experts {j} steps of padding apart"
                assert all(torch.equal(a, b) for a, b in zip(before, (wbuf, sbuf, zbuf, bbuf)))
            # rows of the weights and of the metadata wider than N
            Wv, wbuf = strided(W_q, (R8 * (N + 8), N + 8, 1))
            sv, sbuf = strided(sc, (G * (N + 12), N + 12, 1))
            zv, zbuf = strided(zr, (G * (N + 12), N + 12, 1)) if zr.dim() == 3 else (zr, zr)
            got = windowed(kind, ex, x, ids, spx, w, targs=(Wv, sv, zv))
            assert np.array_equal(got, dense), f"{what}: stride_wk = N + 8, stride_meta_g = N + 12"
    # stride_x_row = 0: every slot reads row 0
    x = rand_x((1, K), dtype, 83)
    for kind in KINDS:
        dense = windowed(kind, ex, x.expand(6, K).contiguous(), ids, 1, w)
        for spx in (1, 2):
            xv = x.expand(6 // spx, K)
            assert xv.stride(0) == 0
            assert np.array_equal(windowed(kind, ex, xv, ids, spx, w), dense), f"{kind}: stride_x_row = 0, {spx} slots per row"


# ================================================================================================ part 5: domain corners
CORNERS = [  # (N, K, gs, dtype, zeros, bias, scales, fma) -> W_group_mode
    ((256, 768, 64, F16, "tensor", True, True, True), 4),
    ((256, 768, 256, B16, "tensor", False, True, False), 3),
    ((32, 256, 256, F16, "int", True, True, True), 3),        # one K-long group
    ((32, 256, 256, B16, "tensor", False, True, False), 3),   # one K-long group, tensor zeros
    ((256, 768, 128, F16, "none", False, True, True), 2),
    ((32, 256, 256, B16, "none", True, True, True), 2),       # one K-long group, scales only
    ((256, 768, 128, B16, "tensor", True, False, True), 1),
    ((32, 4352, 64, F16, "int", False, False, True), 1),
]


@pytest.mark.parametrize("corner,mode", CORNERS, ids=[f"{c[0]}x{c[1]}-g{c[2]}-mode{m}-{c[4]}-{'fp16' if c[3] == F16 else 'bf16'}" for c, m in CORNERS])
def test_group_sizes_and_group_modes_against_float64(corner, mode):
    N, K, gs, dtype, zeros, bias, scales, fma = corner
    h, ex = built(N, K, gs, dtype, zeros, bias, scales=scales, fma=fma)
    assert h.mode == mode and ex.get_meta_args()[10] == mode and ex.get_meta_args()[2] == gs
    ids = torch.tensor(R.MAG_IDS, device=DEV)
    for shared in (False, True):
        x = rand_x((3, K) if shared else (6, K), dtype, 90 + shared, amp=0.5 if scales else 0.02)  # (W = q - z is 60 times larger)
        xs = x if shared else x.view(3, 2, K)
        y, buf = launch_guarded(ex, xs, ids)
        assert guards_intact(buf)
        check_members(h, ex, x, flat(ids), 2 if shared else 1, y, f"{corner} shared {shared}", identity=True)
        out, buf = launch_fused(ex, GLU, xs, ids)
        assert guards_intact(buf)
        check_glu(out, y, dtype, f"{corner} shared {shared}")
        w = R.combine_weights(3, 2, 91).to(DEV)
        out, buf = launch_fused(ex, COMBINE, xs, ids, w)
        assert guards_intact(buf)
        check_combine(out, y.view(3, 2, N), w, dtype, f"{corner} shared {shared}")


def _cycled_ids(n, ids_dtype):
    """ids cycling through the experts with invalid ones mixed in (every 7th: -1 or E) -> (tensor [n], index into the 9 expected rows)"""
    i = np.arange(n)
    ids = np.where(i % 7 == 3, np.where(i % 2 == 0, -1, E), (i * 5) % E)
    return torch.from_numpy(ids).to(ids_dtype).to(DEV), np.where((ids < 0) | (ids >= E), E, ids)


@pytest.mark.parametrize("spx", [65535, 1 << 40], ids=["spx65535", "spx2^40"])
@pytest.mark.parametrize("kind", ["plain", "glu"])
def test_65535_slots_on_one_shared_x_row(kind, spx):
    N, K, row = (16, 256, 2) if kind == "plain" else (32, 256, 1)
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    x = rand_x((1, K), dtype, 95)
    nine = torch.tensor(list(range(E)) + [-1], dtype=ids_dtype, device=DEV)
    y9, buf = launch_guarded(ex, x, nine.view(1, 9))
    assert guards_intact(buf)
    check_members(h, ex, x, flat(nine), 9, y9, f"nine rows {kind}", identity=True)
    want = bits(y9)
    if kind == "glu":
        out9, buf = launch_fused(ex, GLU, x, nine.view(1, 9))
        assert guards_intact(buf)
        check_glu(out9[:E], y9[:E], dtype, "nine rows")
        want = bits(out9)
    assert not want[E].any()
    ids, idx = _cycled_ids(65535, ids_dtype)
    rows, width = out_shape(kind, ids.view(1, -1), N)
    buf = torch.full((GUARD + rows * width + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    e = run(kind, ex.get_tensor_args(), ex.bias, ex.get_meta_args(), x, ids.view(1, -1), spx, buf[GUARD:].data_ptr(), width)
    assert e.n_slots == 65535 and e.slots_per_x_row == spx and guards_intact(buf)
    got = bits(buf[GUARD:GUARD + rows * width].view(rows, width))
    assert np.array_equal(got, want[idx]), np.nonzero((got != want[idx]).any(1))[0][:8]


def test_combine_with_4095_tokens_of_16_slots():
    N, K, row = 16, 256, 1
    dtype, ids_dtype = ROWS[row][0], ROWS[row][4]
    h, ex = built_row(N, K, row)
    T, top_k = 4095, 16
    x = rand_x((1, K), dtype, 96)
    nine = torch.tensor(list(range(E)) + [-1], dtype=ids_dtype, device=DEV)
    y9, _ = launch_guarded(ex, x, nine.view(1, 9))
    check_members(h, ex, x, flat(nine), 9, y9, "nine rows combine")
    ids, idx = _cycled_ids(T * top_k, ids_dtype)
    ids = ids.view(T, top_k)
    w = (R.combine_weights(T, top_k, 97) * (torch.randint(0, 2, (T, top_k), generator=torch.Generator().manual_seed(98)) * 2 - 1)).to(DEV)
    buf = torch.full((GUARD + T * N + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    run("combine", ex.get_tensor_args(), ex.bias, ex.get_meta_args(), x, ids, T * top_k, buf[GUARD:].data_ptr(), N, w)
    assert guards_intact(buf)
    y = y9[torch.from_numpy(idx).to(DEV)].view(T, top_k, N)  # every slot is one of the nine rows (test_65535_slots_...: bit for bit)
    check_combine(buf[GUARD:GUARD + T * N].view(T, N), y, w, dtype, "4095 tokens x 16")


# ================================================================================================ part 6: every 64-bit stride at 4 GiB
def place(t, strides):
    """tests/test_addressing_limits_gpu.py::_place for any number of dimensions: the view's base 2 GiB into ONE allocation of 0xFF bytes
    that reaches max(extent, 4 GiB) + 64 MiB beyond it"""
    es = t.element_size()
    ext = (sum((d - 1) * s for d, s in zip(t.shape, strides)) + 1) * es
    nbytes = (BASE + max(ext, REACH) + TAIL + 7) // 8 * 8
    assert nbytes <= MAX_ALLOC, (nbytes, tuple(t.shape), strides)
    buf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    v = buf.view(t.dtype).as_strided(tuple(t.shape), tuple(strides), BASE // es)
    _ints(v).copy_(_ints(t))
    return v, buf


FAR = ["stride_expert_meta", "stride_expert_bias", "stride_x_row", "stride_out_slot", "stride_wk", "stride_meta_g"]


@pytest.mark.parametrize("field", FAR)
def test_every_64_bit_stride_at_4_gib_and_the_in_expert_32_bit_edge(field):
    """Two experts / x rows / output rows 4 GiB apart (the 64-bit products of the kernels), and rows of the weights / of the metadata at
    the largest stride experts_plan admits (the 32-bit offsets inside an expert; the two experts interleave).  One allocation per case."""
    N, K, gs = R.EDGE_N, R.EDGE_K, R.EDGE_GS
    dtype = F16
    h, ex = built(N, K, gs, dtype, "int", True, n=2)
    W_q, sc, zr = ex.get_tensor_args()
    w = R.combine_weights(2, 2, 99).to(DEV)
    x = rand_x((2, K), dtype, 100)
    moved = {"stride_expert_meta": (sc, (1 << 31, N, 1)), "stride_expert_bias": (ex.bias, (1 << 31, 1)), "stride_x_row": (x, (1 << 31, 1)),
             "stride_wk": (W_q, (N, R.edge_stride_wk(), 1)), "stride_meta_g": (sc, (N, R.edge_stride_meta_g(), 1))}
    expect = {"stride_expert_meta": 1 << 32, "stride_expert_bias": 1 << 32, "stride_x_row": 1 << 31, "stride_out_slot": 1 << 31,
              "stride_wk": R.edge_stride_wk(), "stride_meta_g": R.edge_stride_meta_g()}[field]
    torch.cuda.empty_cache()
    v = big = win = None
    try:
        if field != "stride_out_slot":
            v, big = place(*moved[field])
        for kind in KINDS:
            ids = torch.tensor([[1], [0]] if field == "stride_out_slot" and kind != "combine" else [[1, 0], [1, 1]], device=DEV)
            spx = ids.shape[-1]
            dense = windowed(kind, ex, x, ids, spx, w)
            if field == "stride_out_slot":
                win, big = place(torch.empty(out_shape(kind, ids, N), dtype=dtype, device=DEV), (1 << 31, 1))
                _ints(win).fill_(-1)
                run(kind, ex.get_tensor_args(), ex.bias, ex.get_meta_args(), x, ids, spx, win.data_ptr(), 1 << 31, w)
                got = bits(win)
                _ints(win).fill_(-1)
                assert _all_ff(big), f"{kind}: a store outside the two output rows"
                win = big = None
                torch.cuda.empty_cache()
            else:
                targs = [v if field == "stride_wk" else W_q, v if field in ("stride_expert_meta", "stride_meta_g") else sc, zr]
                got = windowed(kind, ex, v if field == "stride_x_row" else x, ids, spx, w, targs=targs,
                               bias=v if field == "stride_expert_bias" else ex.bias)
            sent = LAST[0].layer if field in ("stride_wk", "stride_meta_g") else LAST[0]
            assert getattr(sent, field) == expect, (field, getattr(sent, field), expect)
            assert np.array_equal(got, dense), f"{kind}: {field}"
        if field != "stride_out_slot":
            _check_and_clear(v, big, moved[field][0], field)
    finally:
        v = big = win = None
        torch.cuda.empty_cache()
