"""The column gate, the profiles and the case lists of tests/test_weight_domain_gpu.py, without a GPU.

The gate exists for the column-side twin of the blind spot test_magnitude_range_cpu.py describes for rows: _compare normalises by
the whole output and row_gate by one row over all N columns, so a block of output channels whose weights are 1000 times smaller
than their neighbours' can come back zeroed, or 1 % off, and pass both.  These tests pin that the column gate rejects such a block
while the other two accept it; that its rounding allowance (twice the CPU model's distance from the exact result) covers a second
legitimate rounding order with margin on every committed profile; that the sweep is every launch site of CASES; that every profile
reaches at least 64 columns of every case that can carry it and really holds what it names; that the planner keeps each case's kernel
after the edit; and which kernels the planner gives layers with an integer zero point."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemlite_amd import _hip
from oracle import gemlite_oracle as O
from oracle import mx_oracle as MX
from tests import test_magnitude_range_gpu as MR
from tests import test_weight_domain_gpu as WD
from tests.test_abi_bounds_cpu import CASES, case_id, kernel_name, plan_args
from tests.test_gpu_parity import REL_TOL
from tests.test_magnitude_range_cpu import _compare_accepts

FP16, BF16 = 1, 2


# ------------------------------------------------------------------------------------------------ the gate
def _output(M=8, N=512, seed=0):
    """an ordinary output whose columns 64 .. 127 belong to channels 1000 times smaller than the rest"""
    rng = np.random.default_rng(seed)
    y_ref = rng.standard_normal((M, N))
    y_ref[:, 64:128] *= 1e-3
    y = (y_ref * (1 + rng.standard_normal((M, N)) * 1e-4)).astype(np.float16).astype(np.float64)
    return y, y_ref, {"normal": np.r_[0:64, 128:N], "small": np.arange(64, 128)}


@pytest.mark.parametrize("how", ["zeroed", "one_percent_off"])
def test_column_gate_rejects_a_small_block_that_the_whole_output_and_row_gates_accept(how):
    y, y_ref, cols = _output()
    tol = REL_TOL[FP16]
    assert all(r["ok"] for r in WD.column_gate(y, y_ref, None, cols, FP16, tol))
    y[:, 64:128] = 0.0 if how == "zeroed" else y_ref[:, 64:128] * 1.01
    assert _compare_accepts(y, y_ref, tol), "the whole-output gate is expected to miss this block"
    assert all(r["ok"] for r in MR.row_gate(y, y_ref, FP16, tol)), "the row gate is expected to miss this block"
    recs = WD.column_gate(y, y_ref, None, cols, FP16, tol)
    assert {(r["profile"], r["ok"]) for r in recs} == {("normal", True), ("small", False)}
    assert sum(not r["ok"] for r in recs) == y.shape[0]  # every row of the block


def test_column_gate_zero_sets_must_be_exactly_zero_and_accept_minus_zero():
    y_ref = np.zeros((2, 128))
    y_ref[0, :64] = 1.0
    cols = {"a": np.arange(64), "dead": np.arange(64, 128)}
    y = y_ref.copy()
    y[:, 64:] = -0.0
    assert all(r["ok"] for r in WD.column_gate(y, y_ref, None, cols, FP16, 1e-3))
    y[1, 70] = 2.0 ** -24
    assert [(r["row"], r["profile"]) for r in WD.column_gate(y, y_ref, None, cols, FP16, 1e-3) if not r["ok"]] == [(1, "dead")]
    y[1, 70] = np.nan
    assert [(r["row"], r["profile"]) for r in WD.column_gate(y, y_ref, None, cols, FP16, 1e-3) if not r["ok"]] == [(1, "dead")]


def test_column_gate_allowance_is_twice_the_model_distance_and_nothing_more():
    rng = np.random.default_rng(2)
    y_ref = rng.standard_normal((1, 64))
    d = rng.standard_normal((1, 64)) * 0.05
    cols = {"p": np.arange(64)}
    assert WD.column_gate(y_ref + d, y_ref, d, cols, BF16, 4e-3)[0]["ok"]       # the model itself
    assert WD.column_gate(y_ref - d, y_ref, d, cols, BF16, 4e-3)[0]["ok"]       # the other side of the exact value
    assert not WD.column_gate(y_ref + d, y_ref, None, cols, BF16, 4e-3)[0]["ok"]  # no allowance without a model
    assert not WD.column_gate(y_ref + 4 * d, y_ref, d, cols, BF16, 4e-3)[0]["ok"]
    assert not WD.column_gate(np.where(np.arange(64) == 9, np.inf, y_ref), y_ref, d, cols, BF16, 4e-3)[0]["ok"]


# ------------------------------------------------------------------------------------------------ emulation against emulation
EMU_N, EMU_K, EMU_GS = 640, 512, 128


@pytest.mark.parametrize("fma", [True, False], ids=["mode4", "mode3"])
@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nbits", [1, 2, 4, 8])
def test_two_rounding_orders_stay_under_0_8_of_the_bound_on_the_committed_profiles(nbits, tdt, fma):
    """The model (bf16: one rounding of the exact weight; fp16: the reference's chained fp16 arithmetic) gives d; the other order
    (bf16: chained; fp16: one rounding) plays the kernel.  Its error against the exact result must stay below 0.8 of the bound on
    every committed integer profile and activation row: a profile that cannot is narrowed here, not on the GPU."""
    r = dict(kind="wn", N=EMU_N, K=EMU_K, nbits=nbits, gs=EMU_GS, tdt=tdt)
    meta = FP16 if tdt == torch.float16 else BF16
    (pas,) = WD.passes_of(WD.INT_PROFILES, EMU_N)
    q, s, z = WD.int_profile_values(r, pas)
    s16, z16 = torch.from_numpy(s).to(tdt), torch.from_numpy(z).to(tdt)
    wgm = 4 if fma else 3
    if fma:
        z16 = (-z16.float() * s16.float()).to(tdt)
    s_gn, z_gn, q_kn = O.to_f64(s16).T, O.to_f64(z16).T, q.T.astype(np.float64)
    W_exact = O.dequantize(q_kn, s_gn, z_gn, EMU_GS, wgm)
    W_model = WD.model_weights(q_kn, s_gn, z_gn, EMU_GS, wgm, False, meta)
    if meta == FP16:
        W_other = O.round_to_dtype(W_exact, FP16)
    else:
        W_other = O.dequantize(q_kn, s_gn, z_gn, EMU_GS, wgm, meta_code=BF16)
    rows = WD.rows_for(tdt)
    x = O.to_f64(MR.make_x(list(rows), EMU_K, tdt, 5))
    y_exact = x @ W_exact
    assert np.abs(y_exact).max() < MR.Y_LIMIT
    recs = WD.column_gate(x @ W_other, y_exact, x @ W_model - y_exact, WD.columns_of(pas, EMU_N), meta, REL_TOL[meta])
    worst = max((r_["ratio"] for r_ in recs if r_["ratio"] is not None), default=0.0)
    assert all(r_["ok"] for r_ in recs) and worst < 0.8, sorted(((r_["ratio"] or 0), r_["profile"], rows[r_["row"]]) for r_ in recs)[-4:]
    dead = [r_ for r_ in recs if r_["profile"] == "dead" or rows[r_["row"]] == "zeros"]
    assert dead and all(r_["ratio"] is None for r_ in dead)  # exactly zero on both sides


# ------------------------------------------------------------------------------------------------ the sweep and its profiles
def test_the_sweep_is_exactly_the_abi_case_table():
    assert WD.SKIP == {}  # nothing is left out; a skip would need its reason here
    assert WD.SWEEP == CASES
    kinds = {c["recipe"]["kind"] for c in CASES}
    assert kinds == set(WD.INT_KINDS) | set(WD.CHANNEL_KINDS) | set(WD.MX_KINDS) | {"nv"}
    assert [cf for cf in WD.PROFILE_RUNS if not cf[1]] == [(c, False) for c in CASES if c["recipe"]["kind"] == "wn" and c["recipe"]["gs"] != c["recipe"]["K"]]


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_profile_reaches_64_columns_and_a_tile_holds_four(case):
    N = case["recipe"]["N"]
    profs = WD.profiles_of(case)
    passes = WD.passes_of(profs, N)
    assert [p for pas in passes for p in pas] == list(profs)
    for pas in passes:
        cols = WD.columns_of(pas, N)
        assert sorted(np.concatenate(list(cols.values())).tolist()) == list(range(N))
        assert all(len(c) >= 64 for c in cols.values()), {p: len(c) for p, c in cols.items()}
        if len(pas) >= 4:
            assert len({p for p, c in cols.items() if ((c >= 16) & (c < 32)).any()}) == 4
    assert len(passes) == (2 if N < 640 and len(profs) > 8 else 1)


EXERCISED = {  # kind -> the profiles its layers really carry (no kind of CASES lacks the tensor a profile edits: no fall-back to base)
    **{k: WD.INT_PROFILES for k in WD.INT_KINDS}, **{k: WD.CHANNEL_PROFILES for k in WD.CHANNEL_KINDS},
    **{k: tuple(f"rung{i}" for i in range(WD.MX_STEPS)) + ("dead",) for k in WD.MX_KINDS}, "nv": WD.NV_PROFILES}


def _edited(case, fma, pas):
    lin = WD.build(case["recipe"], "cpu", fma)
    before = [t.data.clone() for t in (lin.W_q, lin.scales, lin.zeros)]
    cols = WD.edit_layer(lin, case, pas)
    return lin, before, cols


@pytest.mark.parametrize("case,fma", WD.PROFILE_RUNS, ids=[WD.run_id(cf) for cf in WD.PROFILE_RUNS])
def test_edited_layers_keep_their_kernel_and_hold_the_profiles_they_name(case, fma):
    r = case["recipe"]
    kind = r["kind"]
    assert WD.profiles_of(case) == EXERCISED[kind]
    for pas in WD.passes_of(WD.profiles_of(case), r["N"]):
        lin, before, cols = _edited(case, fma, pas)
        a = plan_args(lin, case["M"], case["tuning"], case["fused"])
        assert _hip.load().gemlite_hip_query(C.byref(a)) == 0
        assert kernel_name(a) == case["name"], (case_id(case), fma)
        if kind == "wn":  # (one group per column is channel-wise: the scale moves to the epilogue, the zero stays as it is)
            assert lin.W_group_mode == (1 if r["gs"] == r["K"] else 4 if fma else 3)
        changed = lambda t, b, c: t.numel() > 1 and not torch.equal(t.data[..., c].float(), b[..., c].float())  # noqa: E731
        block = kind not in WD.INT_KINDS and kind not in WD.CHANNEL_KINDS  # (their `base` keeps the scale range, with the format's codes)
        for p, c in cols.items():
            s = lin.scales.data
            if p == "base" and not block:
                assert not changed(lin.scales, before[1], c) and not changed(lin.zeros, before[2], c) and not changed(lin.W_q, before[0], c)
            elif not block:
                sc, zc = s[..., c].float(), (lin.zeros.data[..., c].float() if lin.zeros.numel() > 1 else None)
                s0 = before[1][..., c].float()
                top = 2 ** lin.W_nbits - 1
                zraw = None if zc is None or lin.W_group_mode == 4 else zc  # mode 4 stores -z s
                if p == "dead":
                    assert not sc.any() and (zc is None or not zc.any())
                elif p == "neg":
                    assert torch.equal(sc, -s0) and (sc < 0).all()
                elif p == "large":
                    assert (sc >= 3.9 * s0).all()
                elif p == "small":
                    assert (sc <= s0 / 15.9).all() and (sc > 0).all()
                    if kind in WD.INT_KINDS and r.get("tdt", torch.float16) == torch.float16:
                        assert sc.min() >= 2.0 ** -14  # with integer zeros every non-zero |(q - z) s| stays normal
                        assert zc is None or lin.W_group_mode == 4 or torch.equal(zc, zc.round())
                elif p == "altsign":
                    G = sc.shape[0]
                    want = torch.tensor([0.0 if g % 4 == 3 else (1.0 if g % 2 == 0 else -1.0) for g in range(G)])[:, None]
                    assert torch.equal(torch.sign(sc), want.expand_as(sc))
                    assert lin.W_group_mode != 4 or not zc[3::4].any()  # fma mode: the stored zero term of a pruned group is 0 too
                elif zraw is not None:
                    if p == "zbelow":
                        assert (zraw >= -(top + 1)).all() and (zraw < 0).all() and (zraw != zraw.round()).any()
                    elif p == "zabove":
                        assert (zraw > top).all() and (zraw <= 2 * top + 1).all() and (zraw != zraw.round()).any()
                    elif p == "zfar":
                        assert (zraw.abs() == (2 if lin.W_nbits == 8 else 4) * (top + 1)).all()
                        assert zraw.shape[0] == 1 or ((zraw[0] > 0).all() and (zraw[1] < 0).all())
                    elif p == "zedge":
                        assert ((zraw == 0) | (zraw == top)).all()
                else:
                    assert changed(lin.zeros, before[2], c), p
            else:  # block-scaled: every code of the format in every column, the ladder's byte in every block
                wv, sb = _weights(lin)
                if p == "dead":
                    assert not wv[c].any()
                else:
                    n_codes = 254 if kind in WD.FP8_WEIGHT_KINDS else 16
                    assert all(len(np.unique(_codes(lin)[n])) == n_codes for n in c[:8])
                if p.startswith("rung"):
                    assert (sb[c] == WD.mx_ladder(kind, case["name"], r.get("tdt", torch.float16))[int(p[4:])]).all()
                elif p == "sub":
                    assert all(set(sb[n].tolist()) == set(range(8)) for n in c)
                elif p == "top":
                    assert all((sb[n] == 0x7E).sum() == sb.shape[1] // 8 for n in c)


def _codes(lin):
    """[N, K] codes of a block-scaled layer: e4m3 bytes, or e2m1 codes"""
    wb = WD._w_bytes(lin).t().contiguous().cpu().numpy()
    if lin.W_q.dtype != torch.uint8:
        return wb
    return np.stack([wb & 15, wb >> 4], axis=-1).reshape(wb.shape[0], -1)


def _weights(lin):
    from tests.test_mx_gpu import _weights_nk
    return _weights_nk(lin)


def test_mx_ladders_span_what_they_state():
    assert WD.mx_ladder("mx44", "mx_rows_a4w4_kernel<32x16>", torch.float16) == (107, 111, 116, 120, 124, 129, 133)
    assert WD.mx_ladder("mx88", "mx_rows_a8w8_kernel<64x16>", torch.bfloat16)[::6] == (107, 127)
    lo, hi = MR.FP16_E4M3_EXACT_BAND
    for name in MR.FP16_E4M3_ROUNDING:
        assert set(WD.mx_ladder("mx16w8", name + "<x>", torch.float16)) == set(range(lo, hi + 1))
        assert WD.mx_ladder("mx16w8", name + "<x>", torch.bfloat16)[0] == 107
    v = MX.fp8_e4m3_decode(np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)).astype(np.float64)
    assert 90 < np.sqrt((v ** 2).mean()) < 110  # the rms the e4m3 ladder's upper end is reasoned from


def test_every_case_has_a_poison_and_block_positions_cover_start_middle_and_end():
    for c in CASES:
        labels = [l for l, _ in WD.poisons_of(c)]
        kind = c["recipe"]["kind"]
        assert labels, case_id(c)
        assert ("code_0x7f" in labels) == (kind in WD.FP8_WEIGHT_KINDS)
        assert ("zero_nan" in labels) == (kind in WD.INT_KINDS)
        pos = WD.block_positions(c["recipe"]["N"])
        assert pos["tile_start"] % 16 == 0 and 0 < pos["mid_tile"] % 16 <= 16 - WD.BLOCK_COLS and pos["last"] + WD.BLOCK_COLS == c["recipe"]["N"]
    assert 0 < WD.POISON_COL % 16 < 15 and WD.POISON_COL % 4


def test_an_inf_weight_has_no_finite_e4m3_value():
    """what part 3 holds the fp8-activation families to, which cast the dequantised weight to e4m3 before the product: the format has
    no Inf, and the cast of +-Inf (a finite code times an Inf scale) is its NaN code, not +-448"""
    w = torch.tensor([float("inf"), -float("inf"), float("nan"), 448.0, 1e6]).to(torch.float8_e4m3fn)
    assert w.view(torch.uint8).tolist()[:3] == [0x7F, 0xFF, 0x7F]
    assert torch.isnan(w.float()[:3]).all() and w.float()[3] == 448.0


# ------------------------------------------------------------------------------------------------ scalar zero points
# what the planner gives a 1024 x 512 layer with an integer zero point, one M per distinct kernel: (bits, activations, M, kernel)
SCALAR_ADMISSIONS = [
    (1, "fp16", 1, "gemv_wn_kernel<tile64>"),
    (1, "fp16", 65, "gemm_w1_mma_kernel<128x128>"),
    (1, "bf16", 1, "gemv_wn_kernel<tile64>"),
    (1, "bf16", 65, "gemm_w1_mma_kernel<128x128>"),
    (1, "int8", 1, "generic_matmul_kernel"),
    (1, "fp8", 1, "generic_matmul_kernel"),
    (2, "fp16", 1, "gemv_w2_mfma_kernel<tile16>"),
    (2, "fp16", 33, "gemm_w2_rows_kernel<48x16>"),
    (2, "fp16", 255, "gemm_w2_mma_kernel<64x128>"),
    (2, "bf16", 1, "gemv_w2_mfma_kernel<tile16>"),
    (2, "bf16", 33, "gemm_w2_rows_kernel<48x16>"),
    (2, "bf16", 255, "gemm_w2_mma_kernel<64x128>"),
    (2, "int8", 1, "gemv_a8w2_kernel<tile16,16w>"),
    (2, "int8", 17, "a8w2_rows_kernel<32x16>"),
    (2, "int8", 64, "a8w2_rows_kernel<64x16>"),
    (2, "int8", 65, "gemm_a8w2_mma_kernel<128x128>"),
    (2, "int8", 129, "gemm_a8w2_mma_kernel<256x128>"),
    (2, "fp8", 1, "gemv_a8w2_kernel<tile16,16w>"),
    (2, "fp8", 17, "a8w2_rows_kernel<32x16>"),
    (2, "fp8", 64, "a8w2_rows_kernel<64x16>"),
    (2, "fp8", 65, "gemm_a8w2_mma_kernel<128x128>"),
    (2, "fp8", 129, "gemm_a8w2_mma_kernel<256x128>"),
    (4, "fp16", 2, "gemv_mfma_kernel<tile16,rows4>"),
    (4, "fp16", 4, "gemm_w4_rows_kernel<16x16>"),
    (4, "fp16", 17, "gemm_w4_rows_kernel<32x16>"),
    (4, "fp16", 64, "gemm_w4_rows_kernel<64x16>"),
    (4, "fp16", 129, "gemm_w4_mma_kernel<64x128>"),
    (4, "bf16", 1, "gemv_w4_decode3_kernel<tile16,16w>"),
    (4, "bf16", 2, "gemv_mfma_kernel<tile16,rows4>"),
    (4, "bf16", 17, "gemm_w4_rows_kernel<32x16>"),
    (4, "bf16", 33, "gemm_w4_rows_kernel<48x16>"),
    (4, "int8", 1, "gemv_a8w4_kernel<tile16,16w>"),
    (4, "int8", 17, "a8w4_rows_kernel<32x16>"),
    (4, "int8", 64, "a8w4_rows_kernel<64x16>"),
    (4, "int8", 65, "gemm_a8w4_mma_kernel<64x128>"),
    (4, "fp8", 1, "gemv_a8w4_kernel<tile16,16w>"),
    (4, "fp8", 17, "a8w4_rows_kernel<32x16>"),
    (4, "fp8", 64, "a8w4_rows_kernel<64x16>"),
    (4, "fp8", 65, "gemm_a8w4_mma_kernel<64x128>"),
    (8, "fp16", 33, "gemm_w8_mma_kernel<64x128>"),
    (8, "bf16", 33, "gemm_w8_mma_kernel<64x128>"),
    (8, "int8", 1, "generic_matmul_kernel"),
    (8, "fp8", 1, "generic_matmul_kernel"),
]


def test_scalar_zero_admission_list():
    got = WD.scalar_admissions()
    assert {(b, a) for b, a, _, _ in got} == {(b, a) for b in WD.SCALAR_BITS for a in WD.SCALAR_ACTS}  # every combination is admitted
    assert not [g for g in got if g[3].startswith("status")]
    assert got == SCALAR_ADMISSIONS


def test_scalar_zero_values_meet_the_bytewise_precondition_of_the_integer_paths():
    """((q | 0x80) - z) ^ 0x80 is q - z for every byte with q <= 127 and z <= 128 (no borrow leaves a byte); the integer paths that use
    it hold 1-, 2- and 4-bit codes.  An 8-bit code of 128 or more breaks it, so no kernel with that form may be planned for 8-bit words."""
    for nbits in (1, 2, 4):
        for z in WD.scalar_zero_values(nbits):
            q = np.arange(2 ** nbits, dtype=np.uint32)
            got = ((((q | 0x80) - z) ^ 0x80) & 0xFF).astype(np.uint8).view(np.int8)
            assert np.array_equal(got, (q.astype(np.int64) - z).astype(np.int8)), (nbits, z)
    assert (((np.uint32(200) | 0x80) - 128) ^ 0x80) & 0xFF != 200 - 128
    bytewise = ("gemv_a8w", "a8w4_rows", "a8w2_rows", "gemm_a8w4_mma", "gemm_a8w2_mma")
    assert not [g for g in SCALAR_ADMISSIONS if g[0] == 8 and g[1] == "int8" and g[3].startswith(bytewise)]
