"""Every kernel across the weight metadata a checkpoint can hold (run on a real MI355X via `pytest -m gpu`).

All other tests draw their weights from O.gen_data: uniform codes, group scales in [0.001, 0.011], zero points inside the code range.
Here the metadata of the built layer is edited in place (lin.scales.data, lin.zeros.data, lin.W_q.data), so packing and mode
selection stay on the product's path, and four things are checked on every entry of tests/test_abi_bounds_cpu.py::CASES (same
recipe, same M, same forced tuning; the planner must still name the case's kernel after the edit):

  1. column profiles   column n takes profile (n // 4) mod P, so a 16-column tile holds four profiles.  Each (row, profile) set of
                       outputs is held against its own float64 oracle:  mean|e| <= tol mean|y| + q + 2 mean|d|  and elementwise
                       |e| <= 10 tol mean|y| + 4 tol |y| + q + 2 max|d|, means and max over the set.  d = y_model - y_exact is the
                       cost of the family's documented 16-bit rounding of the dequantised weight, computed on the CPU from the same
                       inputs (never from the kernel): zero for the families of EXACT_UNPACK, one rounding of the exact weight for
                       bf16, the reference's chained fp16 arithmetic (O.dequantize(meta_code=FP16)) for fp16.  The factor 2 is a
                       condition: a single and a double rounding can each sit d away from the exact value.  A set whose oracle is
                       all zero (the `dead` profile, the all-zero activation row) must come back exactly zero.
  2. independence      replacing one 4-column block's scales, zeros and codes leaves every other column as the clean launch wrote
                       it, as raw bits (block at a tile's start, inside a tile, and as the last columns of N).
  3. non-finite        a NaN / Inf scale, a NaN zero, a NaN block-scale byte or a NaN weight code leaves every other column bit
                       identical, and every row of its own column non-finite, the all-zero activation row included.
  4. scalar zeros      every (bits, activation type, kernel) the planner admits with an integer zero point, z in {0, 1, 2^(b-1),
                       2^b - 1}: int8 activations bit-exact, the rest through the gate of 1.
Gates, case lists and their self-tests: tests/test_weight_domain_cpu.py.  Records join the JSON report of test_gpu_parity, tagged
wdom/<profile>/<case id>."""
import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, kernel_name, plan_args
from tests.test_gpu_parity import REPORT
from tests.test_gpu_parity import _report  # noqa: F401  (autouse here too: writes REPORT, these records included, when the module ends)
from tests.test_magnitude_range_gpu import (EXACT_UNPACK, FP16_E4M3_EXACT_BAND, FP16_E4M3_ROUNDING, QUANTUM, Y_LIMIT, _x_dtype,
                                            launch_rows, make_x, tol_of)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

INT_KINDS = ("wn", "a8w4", "a8w2")                                          # packed integer codes, per-group scales and zeros
CHANNEL_KINDS = ("a16w8i", "a16w8f", "a8w8i", "a8w8f", "bitnet16", "bitnet8")  # one scale per output channel
MX_KINDS = ("mx16w4", "mx16w8", "mx44", "mx84", "mx88")                      # e8m0 block scales
FP8_WEIGHT_KINDS = ("a16w8f", "a8w8f", "mx16w8", "mx88")

# case_id -> reason; every entry of CASES not named here is swept (tests/test_weight_domain_cpu.py checks the list)
SKIP = {}
SWEEP = [c for c in CASES if case_id(c) not in SKIP]

ROWS = ("amp1e-1", "amp1e-3", "mean", "zeros", "subnormal")  # activation rows of part 1 (test_magnitude_range_gpu.profile_row)


def rows_for(tdt):
    return ROWS if tdt == torch.float16 else tuple(p for p in ROWS if p != "subnormal")


# ------------------------------------------------------------------------------------------------ column profiles
INT_PROFILES = ("base", "small", "large", "neg", "altsign", "zbelow", "zabove", "zfar", "zedge", "dead")
CHANNEL_PROFILES = ("base", "small", "large", "neg", "dead")
NV_PROFILES = ("base", "sub", "top", "dead")
# e8m0 bytes of the MX scale ladder, one per profile, lowest to highest.  fp4 weights take 127 - 20 .. 127 + 6.  e4m3 weight codes over
# the whole format have an rms of ~100 (fp4: ~2.7), so a column's |y| under the 0.5-mean activation row is ~4000 at 2^0 already: their
# ladder ends at 127, where |y_ref| < Y_LIMIT ends it.  The fp16 forms of the A16W8_MXFP rows / tile kernels stay inside
# FP16_E4M3_EXACT_BAND (test_magnitude_range_gpu: e4m3 x 2^e is exact in fp16 only there, and they convert into fp16).
MX_STEPS = 7


def mx_ladder(kind, name, tdt):
    if kind == "mx16w8" and tdt == torch.float16 and name.split("<")[0] in FP16_E4M3_ROUNDING:
        lo, hi = FP16_E4M3_EXACT_BAND
        return tuple(lo + i % (hi - lo + 1) for i in range(MX_STEPS))
    top = 127 if kind in FP8_WEIGHT_KINDS else 127 + 6
    return tuple(int(v) for v in np.round(np.linspace(127 - 20, top, MX_STEPS)))


def profiles_of(case):
    kind = case["recipe"]["kind"]
    if kind in INT_KINDS:
        return INT_PROFILES
    if kind in CHANNEL_KINDS:
        return CHANNEL_PROFILES
    if kind == "nv":
        return NV_PROFILES
    return tuple(f"rung{i}" for i in range(MX_STEPS)) + ("dead",)


def passes_of(profs, N):
    """the profiles split into passes (one edited layer each) so that every profile of a pass owns at least 64 columns:
    column n of a pass takes its profile (n // 4) mod P, P <= N // 64 (a 16-column tile holds four profiles wherever P >= 4)"""
    pmax = max(1, min(len(profs), N // 64))
    return [profs[i:i + pmax] for i in range(0, len(profs), pmax)]


def columns_of(pas, N):
    """{profile: column indices} of one pass"""
    idx = (np.arange(N) // 4) % len(pas)
    return {p: np.nonzero(idx == i)[0] for i, p in enumerate(pas)}


def _tdt(r):
    return r.get("tdt", torch.float16)


def build(r, device, fma=True):
    """build_layer, with the `wn` layers also in fma_mode=False (W_group_mode 3: the zero point stored as it is)"""
    if r["kind"] != "wn" or fma:
        return build_layer(r, device)
    tdt = _tdt(r)
    W_q, sc, zr = O.gen_data(r["N"], r["K"], r["nbits"], r["gs"], seed=0, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(r["nbits"], r["gs"], r["K"], r["N"], code, code)
    lin.pack(torch.from_numpy(W_q).to(device), torch.from_numpy(sc.astype(np.float32)).to(tdt).to(device),
             torch.from_numpy(zr.astype(np.float32)).to(tdt).to(device), None, fma_mode=False)
    return lin


def _nbits(r):
    return r.get("nbits", 4 if r["kind"] == "a8w4" else 2)


def int_profile_values(r, pas):
    """(q [N, K] uint8, s [N, G] float32, z [N, G] float32) of recipe r's gen_data with the profiles of pass `pas` applied, before
    the cast to the layer's 16-bit type"""
    N, K, gs, nbits = r["N"], r["K"], r["gs"], _nbits(r)
    G, top = K // gs, 2 ** nbits - 1
    q, s, z = O.gen_data(N, K, nbits, gs, seed=0, np_float=np.float16)
    q, s, z = q.copy(), s.astype(np.float32).reshape(N, G), z.astype(np.float32).reshape(N, G)
    rng = np.random.default_rng(11)
    gi = np.arange(G)
    for p, c in columns_of(pas, N).items():
        shape = (len(c), G)
        if p == "small":  # the rule of test_magnitude_range_gpu.scale_factors: fp16 keeps every non-zero |(q - z) s| normal
            if _tdt(r) == torch.float16:
                s[c], z[c] = s[c] / 16, np.round(z[c])
            else:
                s[c] = s[c] * np.float32(2.0 ** -20)
        elif p == "large":
            s[c] = s[c] * (4 if nbits == 8 else 16)
        elif p == "neg":
            s[c] = -s[c]
        elif p == "altsign":  # sign by group; every 4th group pruned (in fma mode its stored zero term -z * 0 is 0 as well)
            s[c] = s[c] * np.where(gi % 4 == 3, 0.0, np.where(gi % 2 == 0, 1.0, -1.0)).astype(np.float32)
        elif p == "zbelow":   # [-(top + 1), 0)
            z[c] = -(top + 1) + rng.random(shape, dtype=np.float32) * (top + 1)
        elif p == "zabove":   # (top, 2 top + 1]; the lower end far enough above top to stay there in bf16
            z[c] = np.maximum(top + (1 - rng.random(shape, dtype=np.float32)) * (top + 1), top + (top + 1) / 64)
        elif p == "zfar":
            z[c] = np.where(gi % 2 == 0, 1.0, -1.0).astype(np.float32) * (2 if nbits == 8 else 4) * (top + 1)
        elif p == "zedge":    # z on the edges of the code range; every second group all codes equal to z: w = 0 there
            z[c] = rng.integers(0, 2, shape).astype(np.float32) * top
            for g in range(1, G, 2):
                q[c, g * gs:(g + 1) * gs] = z[c, g].astype(np.uint8)[:, None]
        elif p == "dead":
            s[c], z[c] = 0.0, 0.0
        else:
            assert p == "base", p
    return q, s, z


def _store_int(lin, r, q, s, z):
    """write (q, s, z) into the built layer the way pack() lays them out: [K/g, N] scales, zeros folded to -z s in fma mode"""
    N, nbits = r["N"], _nbits(r)
    dev = lin.scales.device
    pb = lin.W_q.element_size() * 8
    q0 = O.gen_data(N, r["K"], nbits, r["gs"], seed=0, np_float=np.float16)[0]
    packed0 = torch.from_numpy(O.pack_over_cols(q0, nbits, pb))
    assert torch.equal(packed0, lin.W_q.data.cpu()), "the layer's packed words are not pack_over_cols of its recipe's codes"
    sdt = lin.scales.dtype
    s_t, z_t = torch.from_numpy(s).to(sdt), torch.from_numpy(z).to(lin.zeros.dtype)
    if lin.W_group_mode == 4:
        z_t = (-z_t.float() * s_t.float()).to(lin.zeros.dtype)
    else:  # 3: the zero as it is; 1: one group per column, the scale in the epilogue
        assert lin.W_group_mode in (1, 3), lin.W_group_mode
    lin.scales.data.copy_(s_t.t().to(dev))
    lin.zeros.data.copy_(z_t.t().to(dev))
    lin.W_q.data.copy_(torch.from_numpy(O.pack_over_cols(q, nbits, pb)).to(dev))


def _fp8_codes(rng, shape):
    """every e4m3 code except the two NaN codes, each the same number of times (+- 1) along the last axis, shuffled per row"""
    codes = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)
    return rng.permuted(np.tile(np.resize(codes, shape[-1]), shape[:-1] + (1,)), axis=-1)


def _fp4_codes(rng, shape):
    return rng.permuted(np.tile(np.resize(np.arange(16, dtype=np.uint8), shape[-1]), shape[:-1] + (1,)), axis=-1)


def block_profile_values(case, pas):
    """(codes [N, K] uint8: e4m3 bytes or e2m1 codes, scale bytes [N, K/g]) of a block-scaled case under pass `pas`"""
    r = case["recipe"]
    kind, N, K = r["kind"], r["N"], r["K"]
    rng = np.random.default_rng(13)
    w8 = kind in FP8_WEIGHT_KINDS
    codes = (_fp8_codes if w8 else _fp4_codes)(rng, (N, K))
    g = 16 if kind == "nv" else 32
    B = K // g
    if kind == "nv":  # e4m3 scale bytes 0.5 .. 3.5, as build_layer draws them
        sc = torch.from_numpy((rng.random((N, B), dtype=np.float32) * 3 + 0.5)).to(torch.float8_e4m3fn).view(torch.uint8).numpy().copy()
    else:
        sc = np.zeros((N, B), np.uint8)
        ladder = mx_ladder(kind, case["name"], _tdt(r))
    bi = np.arange(B)
    for p, c in columns_of(pas, N).items():
        if p == "dead":
            codes[c] = rng.integers(0, 2, (len(c), K)).astype(np.uint8) * (0x80 if w8 else 8)  # +0 / -0
            if kind != "nv":
                sc[c] = 127
        elif p.startswith("rung"):
            sc[c] = ladder[int(p[4:])]
        elif p == "sub":   # e4m3 zero and the seven subnormals, every one in every column
            sc[c] = ((bi[None, :] + c[:, None]) % 8).astype(np.uint8)
        elif p == "top":   # 448 in every 8th block
            sc[c] = np.where((bi[None, :] + c[:, None]) % 8 == 0, 0x7E, sc[c])
        else:
            assert p == "base", p
    return codes, sc


def _w_bytes(lin):
    """the layer's weight bytes as a writable uint8 view, [K, N] (fp8) or [K/2, N] (two e2m1 codes per byte)"""
    return lin.W_q.data.view(torch.uint8) if lin.W_q.dtype != torch.uint8 else lin.W_q.data


def _store_block(lin, r, codes, sc):
    from oracle import mx_oracle as MX
    dev = lin.W_q.device
    wb = _w_bytes(lin)
    new = codes if r["kind"] in FP8_WEIGHT_KINDS else MX.fp4_pack_codes(codes)  # [N, K] or [N, K/2]
    assert tuple(wb.shape) == new.T.shape and tuple(lin.scales.shape) == sc.shape, (wb.shape, new.shape, lin.scales.shape, sc.shape)
    wb.copy_(torch.from_numpy(np.ascontiguousarray(new)).t().to(dev))
    lin.scales.data.view(torch.uint8).copy_(torch.from_numpy(sc).to(dev))


def channel_factors(r, pas):
    N = r["N"]
    f = np.ones(N, np.float32)
    small = 1.0 / 16 if _tdt(r) == torch.float16 else 2.0 ** -20
    for p, c in columns_of(pas, N).items():
        f[c] = {"base": 1.0, "small": small, "large": 16.0, "neg": -1.0, "dead": 0.0}[p]
    return f


def edit_layer(lin, case, pas):
    """apply pass `pas` of the case's profiles to the built layer, in place; returns {profile: columns}"""
    r = case["recipe"]
    kind = r["kind"]
    if kind in INT_KINDS:
        _store_int(lin, r, *int_profile_values(r, pas))
    elif kind in CHANNEL_KINDS:
        assert lin.scales.numel() == r["N"]
        f = torch.from_numpy(channel_factors(r, pas)).to(lin.scales.device)
        lin.scales.data.copy_((lin.scales.data.float().reshape(-1) * f).to(lin.scales.dtype).view_as(lin.scales.data))
    else:
        _store_block(lin, r, *block_profile_values(case, pas))
    return columns_of(pas, r["N"])


# ------------------------------------------------------------------------------------------------ the column gate
def column_gate(y, y_exact, d, cols, out_code, tol):
    """records per (row, profile) of y against y_exact [M, N] (float64), d = y_model - y_exact or None; rec['ratio'] is the larger of
    mean|e| / mean bound and max(|e| / elementwise bound), rec['ok'] the verdict"""
    y = np.asarray(y, np.float64)
    y_exact = np.asarray(y_exact, np.float64).reshape(y.shape)
    q = QUANTUM[out_code]
    recs = []
    for prof, idx in cols.items():
        e, ref = np.abs(y[:, idx] - y_exact[:, idx]), np.abs(y_exact[:, idx])
        dd = np.zeros_like(ref) if d is None else np.abs(np.asarray(d, np.float64).reshape(y.shape)[:, idx])
        for m in range(y.shape[0]):
            finite = bool(np.isfinite(y[m, idx]).all())
            scale = float(ref[m].mean())
            rec = dict(row=m, profile=prof, mean_abs_ref=scale, mean_abs_err=float(e[m].mean()) if finite else None,
                       mean_abs_d=float(dd[m].mean()), finite=finite, tol=tol)
            if not ref[m].any():  # the relative gate is undefined: the set must be exactly zero (-0 included)
                rec["ratio"] = None
                rec["ok"] = finite and bool((y[m, idx] == 0).all())
            elif not finite:
                rec["ratio"], rec["ok"] = float("inf"), False
            else:
                mean_bound = tol * scale + q + 2 * rec["mean_abs_d"]
                elem_bound = 10 * tol * scale + 4 * tol * ref[m] + q + 2 * float(dd[m].max())
                rec["ratio"] = float(max(e[m].mean() / mean_bound, (e[m] / elem_bound).max()))
                rec["ok"] = rec["ratio"] <= 1.0
            recs.append(rec)
    return recs


def rounds_weight(lin, name):
    """does kernel `name` round the dequantised weight of this layer to a 16-bit type (the families the allowance d is for)?"""
    if lin.input_dtype in (DType.MXFP16, DType.MXBF16, DType.MXFP8, DType.MXFP4, DType.NVFP4):
        return False  # block scales are powers of two (NVFP4: products in fp32); the fp16 e4m3 band is kept exact by the ladder
    if lin.input_dtype == DType.INT8 or lin.scales.numel() == 0:
        return False  # integer codes minus an integer zero
    return not name.startswith(EXACT_UNPACK)


def model_weights(q_kn, s, z, gs, wgm, scalar, meta, wcast=None):
    """W [K, N] as the family's documented rounding gives it: bf16 one rounding of the exact weight, fp16 the reference's chained
    arithmetic; then the e4m3 cast of the fp8-activation families"""
    if meta == O.FP16:
        W = O.dequantize(q_kn, s, z, gs, wgm, scalar, meta_code=O.FP16)
    else:
        W = O.round_to_dtype(O.dequantize(q_kn, s, z, gs, wgm, scalar), meta)
    return W if wcast is None else O.round_to_dtype(W, wcast)


def _model(lin, x16, name):
    """float64 result of the layer on x16 with the weight rounded as `model_weights` says (the counterpart of
    test_abi_bounds_gpu._oracle, same quantised activations), or None where the kernel's weight is exact"""
    if not rounds_weight(lin, name):
        return None
    meta_args = lin.get_meta_args()
    e, wgm, csm = meta_args[4], meta_args[10], meta_args[9]
    meta = lin.output_dtype.value
    s = O.to_f64(lin.scales.data)
    scalar = lin.zeros.numel() == 1
    z = O.to_f64(lin.zeros.data).reshape(-1) if scalar else (O.to_f64(lin.zeros.data) if lin.zeros.numel() else None)
    if e > 1:
        q_kn = O.unpack_over_cols(lin.W_q.data.cpu().numpy(), lin.W_nbits, lin.W_q.element_size() * 8).T.astype(np.float64)
    else:
        q_kn = O.to_f64(lin.W_q.data)
    code = lin.input_dtype
    if code in (DType.FP16, DType.BF16):
        xq, sx, wcast = O.to_f64(x16), None, None
    else:
        if e == 1:
            return None  # fp8 codes under fp8 activations: no weight rounding
        xq, sx = O.scale_activations_per_token(x16, O.FP8E4)
        wcast = None if name.startswith("gemv_a8w") else O.FP8E4
    W = model_weights(q_kn, s if wgm >= 2 else None, z if wgm in (1, 3, 4) else None, lin.group_size, wgm, scalar, meta, wcast)
    return O.forward(xq.reshape(-1, xq.shape[-1]), W, scales_w_channel=s if csm in (1, 3) else None, scales_x=sx,
                     channel_scale_mode=csm)


def _sweep(lin, case, tag, cols, seed, profs=None):
    """run every launch of `case` on the edited `lin`; returns (failing records, worst ratio)"""
    from tests.test_abi_bounds_gpu import _oracle, _quantised_inputs, _run
    M, K = case["M"], lin.in_features
    tdt = _x_dtype(lin)
    out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    bad, worst = [], 0.0
    for li, rows in enumerate(launch_rows(M, profs or rows_for(tdt))):
        x16 = make_x(rows, K, tdt, seed + li).to(DEV)
        xk, sx = _quantised_inputs(lin, x16, case["fused"])
        res = _run(lin, case, xk, sx, None)
        assert res is not None
        y, name, _ = res
        assert name == case["name"], name
        y_exact = np.asarray(_oracle(lin, x16, name)[0], np.float64).reshape(M, -1)
        assert float(np.abs(y_exact).max()) < Y_LIMIT, (tag, float(np.abs(y_exact).max()))
        y_model = _model(lin, x16, name)
        d = None if y_model is None else y_model.reshape(M, -1) - y_exact
        tol = tol_of(lin, name, out_code)
        recs = column_gate(y.float().cpu().numpy(), y_exact, d, cols, out_code, tol)
        for p in cols:
            mine = [r for r in recs if r["profile"] == p]
            ratios = [r["ratio"] for r in mine if r["ratio"] is not None]
            REPORT.append(dict(tag=f"wdom/{p}/{tag}", kernel=name, launch=li, rows=len(mine), ok=all(r["ok"] for r in mine),
                               worst_ratio=max(ratios) if ratios else None, mean_abs_d=float(np.mean([r["mean_abs_d"] for r in mine])),
                               exact_zero_sets=sum(r["ratio"] is None for r in mine)))
            worst = max([worst] + ratios)
        for rec in recs:
            if not rec["ok"]:
                rec.update(launch=li, act=rows[rec["row"]])
                bad.append(rec)
    return bad, worst


def _fmt(bad):
    return "\n".join(f"  row {r['row']} ({r['act']}, launch {r['launch']}) x {r['profile']}: ratio {r['ratio']} mean|y| {r['mean_abs_ref']:.3e} "
                     f"mean|e| {r['mean_abs_err']} mean|d| {r['mean_abs_d']:.3e} finite {r['finite']}" for r in bad[:16])


def modes_of(case):
    """the fma_mode settings a case is run with: both for the `wn` recipes with more than one group per column (pack() folds nothing
    for a channel-wise layer), the recipe's own otherwise"""
    r = case["recipe"]
    return (True, False) if r["kind"] == "wn" and r["gs"] != r["K"] else (True,)


PROFILE_RUNS = [(c, fma) for c in SWEEP for fma in modes_of(c)]


def run_id(cf):
    return case_id(cf[0]) + ("" if cf[1] else "-mode3")


@pytest.mark.parametrize("case,fma", PROFILE_RUNS, ids=[run_id(cf) for cf in PROFILE_RUNS])
def test_every_kernel_holds_each_column_profile(case, fma):
    r = case["recipe"]
    bad, worst = [], 0.0
    for pi, pas in enumerate(passes_of(profiles_of(case), r["N"])):
        lin = build(r, DEV, fma)
        cols = edit_layer(lin, case, pas)
        assert kernel_name(plan_args(lin, case["M"], case["tuning"], case["fused"])) == case["name"]
        b, w = _sweep(lin, case, run_id((case, fma)), cols, seed=case["M"] + 200 + pi)
        bad += b
        worst = max(worst, w)
    print(f"wdom worst ratio {worst:.3f} {run_id((case, fma))}")
    assert not bad, f"{case['name']}: {len(bad)} (row, profile) sets fail the column gate\n{_fmt(bad)}"


# ------------------------------------------------------------------------------------------------ 2. columns are independent
BLOCK_COLS = 4


def block_positions(N):
    """first column of the replaced block: at a 16-column tile's start, inside a tile, the last columns of N"""
    return {"tile_start": 32, "mid_tile": 38, "last": N - BLOCK_COLS}


def _random_words(t, shape, gen):
    """random codes for a slice of W_q of dtype t: any bit pattern, except the two e4m3 NaN codes where the bytes are fp8"""
    if t == torch.int32:
        return torch.randint(-2 ** 31, 2 ** 31, shape, generator=gen, dtype=torch.int64).to(torch.int32)
    if t == torch.int8:
        return torch.randint(-128, 128, shape, generator=gen, dtype=torch.int8)
    if t == torch.uint8:
        return torch.randint(0, 256, shape, generator=gen, dtype=torch.uint8)
    b = torch.randint(0, 0x7F, shape, generator=gen, dtype=torch.uint8) | (torch.randint(0, 2, shape, generator=gen, dtype=torch.uint8) << 7)
    return b.view(t)


def replace_block(lin, case, c0, seed=5):
    """`neg` scales, `zfar` zeros and random codes in columns c0 .. c0 + 3 of the built layer, in place"""
    r = case["recipe"]
    kind = r["kind"]
    gen = torch.Generator().manual_seed(seed)
    c = slice(c0, c0 + BLOCK_COLS)
    dev = lin.W_q.device
    if kind in INT_KINDS or kind in CHANNEL_KINDS:
        lin.scales.data[..., c] = -lin.scales.data[..., c]
        if lin.zeros.numel() > 1:
            G = lin.zeros.shape[0]
            top = 2 ** lin.W_nbits - 1
            z = (torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0) * (2 if lin.W_nbits == 8 else 4) * (top + 1))[:, None].to(dev)
            if lin.W_group_mode == 4:
                z = -z * lin.scales.data[:, c].float()
            lin.zeros.data[:, c] = z.to(lin.zeros.dtype).expand(G, BLOCK_COLS)
        w = lin.W_q.data
        w[:, c] = _random_words(w.dtype, (w.shape[0], BLOCK_COLS), gen).to(dev)
    else:
        sb = lin.scales.data.view(torch.uint8)  # [N, K/g]
        lo, hi = (0x28, 0x48) if kind == "nv" else (120, 131)
        sb[c] = torch.randint(lo, hi, (BLOCK_COLS, sb.shape[1]), generator=gen, dtype=torch.uint8).to(dev)
        wb = _w_bytes(lin)
        t = torch.uint8 if kind not in FP8_WEIGHT_KINDS else torch.float8_e4m3fn
        wb[:, c] = _random_words(t, (wb.shape[0], BLOCK_COLS), gen).view(torch.uint8).to(dev)


def _snapshot(lin):
    return [t.data.clone() for t in (lin.W_q, lin.scales, lin.zeros)]


def _restore(lin, snap):
    for t, s in zip((lin.W_q, lin.scales, lin.zeros), snap):
        t.data.copy_(s)


def _others_equal(y, y0, cols, N):
    from tests.test_abi_bounds_gpu import _raw
    keep = torch.ones(N, dtype=torch.bool, device=y.device)
    keep[cols] = False
    diff = (_raw(y) != _raw(y0)) & keep[None, :]
    return diff


@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_columns_are_independent_bit_for_bit(case):
    from tests.test_abi_bounds_gpu import _quantised_inputs, _raw, _run
    r = case["recipe"]
    N, M = r["N"], case["M"]
    lin = build_layer(r, DEV)
    tdt = _x_dtype(lin)
    x16 = torch.from_numpy(O.gen_x(M, lin.in_features, seed=M + 3).astype(np.float32)).to(tdt).to(DEV)
    xk, sx = _quantised_inputs(lin, x16, case["fused"])
    y0, name, _ = _run(lin, case, xk, sx, None)
    assert name == case["name"], name
    snap = _snapshot(lin)
    for where, c0 in block_positions(N).items():
        replace_block(lin, case, c0)
        assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
        y, name, _ = _run(lin, case, xk, sx, None)
        assert name == case["name"], name
        cols = torch.arange(c0, c0 + BLOCK_COLS, device=DEV)
        diff = _others_equal(y, y0, cols, N)
        assert not bool(diff.any()), (f"{name}: replacing columns {c0} .. {c0 + BLOCK_COLS - 1} ({where}) changed {int(diff.sum())} outputs "
                                      f"of other columns, first at column {int(diff.any(0).nonzero()[0])}")
        assert bool((_raw(y)[:, cols] != _raw(y0)[:, cols]).any()), f"{where}: the replaced block did not change its own columns"
        _restore(lin, snap)


# ------------------------------------------------------------------------------------------------ 3. non-finite metadata
POISON_COL = 37  # inside a 16-column tile, inside a 4-column quad


def poisons_of(case):
    """[(label, what)] of a case: the non-finite values its kind of metadata can hold"""
    kind = case["recipe"]["kind"]
    out = []
    if kind in INT_KINDS:
        out += [("scale_nan", "scale"), ("scale_inf", "scale"), ("zero_nan", "zero")]
    elif kind in CHANNEL_KINDS:
        out += [("scale_nan", "scale"), ("scale_inf", "scale")]
    elif kind == "nv":
        out += [("scale_0x7f", "block")]
    else:
        out += [("scale_0xff", "block")]
    if kind in FP8_WEIGHT_KINDS:  # (every fp8 layer of CASES is e4m3: no Inf code exists)
        out += [("code_0x7f", "code")]
    return out


def poison(lin, case, label, n=POISON_COL):
    """one non-finite value in column n of the built layer's metadata or codes, in place"""
    kind = case["recipe"]["kind"]
    v = float("nan") if label.endswith("nan") else float("inf")
    if label.startswith("scale_") and kind in INT_KINDS:
        lin.scales.data[lin.scales.shape[0] // 2, n] = v
    elif label.startswith("scale_") and kind in CHANNEL_KINDS:
        lin.scales.data.view(-1)[n] = v
    elif label == "zero_nan":
        lin.zeros.data[lin.zeros.shape[0] // 2, n] = v
    elif label in ("scale_0xff", "scale_0x7f"):
        sb = lin.scales.data.view(torch.uint8)
        sb[n, sb.shape[1] // 2] = int(label[-4:], 16)
    elif label == "code_0x7f":
        wb = _w_bytes(lin)
        wb[wb.shape[0] // 2 + 1, n] = 0x7F
    else:
        raise ValueError(label)


NONFINITE_ROWS = ("amp1e-1", "zeros")


@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_non_finite_metadata_stays_in_its_column_and_shows_there(case):
    from tests.test_abi_bounds_gpu import _quantised_inputs, _run
    r = case["recipe"]
    N, M = r["N"], case["M"]
    lin = build_layer(r, DEV)
    tdt = _x_dtype(lin)
    snap = _snapshot(lin)
    col = torch.tensor([POISON_COL], device=DEV)
    problems = []
    for li, rows in enumerate(launch_rows(M, NONFINITE_ROWS)):
        x16 = make_x(rows, lin.in_features, tdt, 300 + M + li).to(DEV)
        xk, sx = _quantised_inputs(lin, x16, case["fused"])
        y0, name, _ = _run(lin, case, xk, sx, None)
        assert name == case["name"], name
        assert bool(torch.isfinite(y0.float()).all())
        for label, _what in poisons_of(case):
            poison(lin, case, label)
            assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
            y, name, _ = _run(lin, case, xk, sx, None)
            _restore(lin, snap)
            diff = _others_equal(y, y0, col, N)
            if bool(diff.any()):
                problems.append(f"{label}: {int(diff.sum())} outputs of other columns changed, first at column {int(diff.any(0).nonzero()[0])}")
            yc = y[:, POISON_COL].float()
            fin = torch.isfinite(yc)
            if bool(fin.any()):
                which = [(int(m), rows[int(m)], float(yc[m])) for m in fin.nonzero().reshape(-1)[:4]]
                problems.append(f"{label}: column {POISON_COL} finite in {int(fin.sum())} of {M} rows, e.g. (row, activations, y) {which}")
    assert not problems, f"{case['name']}:\n  " + "\n  ".join(problems)


# ------------------------------------------------------------------------------------------------ 4. scalar zero points
SCALAR_BITS = (1, 2, 4, 8)
SCALAR_ACTS = ("fp16", "bf16", "int8", "fp8")
SCALAR_N, SCALAR_K, SCALAR_GS = 1024, 512, 128


def scalar_zero_values(nbits):
    return sorted({0, 1, 2 ** (nbits - 1), 2 ** nbits - 1})


def scalar_ms(nbits, act):
    """the M of the CASES entries that match: packed words of `nbits` under that activation type (8-bit activations: every A8Wn /
    BitNet entry; a width CASES does not hold under that type borrows the 4-bit entries' M)"""
    def ms(pred):
        return sorted({c["M"] for c in CASES if pred(c["recipe"])})
    if act in ("fp16", "bf16"):
        tdt = torch.float16 if act == "fp16" else torch.bfloat16
        return (ms(lambda r: r["kind"] == "wn" and r["nbits"] == nbits and _tdt(r) == tdt)
                or ms(lambda r: r["kind"] == "wn" and r["nbits"] == nbits) or ms(lambda r: r["kind"] == "wn" and r["nbits"] == 4))
    return ms(lambda r: r["kind"] in ("a8w4", "a8w2", "bitnet8"))


def scalar_layer(nbits, act, z, device):
    """a layer with an integer zero point: 16-bit activations x group scales (W_group_mode 3), fp8 activations x group scales
    (3, per-token scale in the epilogue), int8 activations x integer codes with a channel scale of 2^-6 in the epilogue (1, 3)"""
    N, K, gs = SCALAR_N, SCALAR_K, SCALAR_GS
    W_q, sc, _ = O.gen_data(N, K, nbits, gs, seed=nbits, np_float=np.float16)
    W_q = torch.from_numpy(W_q).to(device)
    if act in ("fp16", "bf16"):
        tdt = torch.float16 if act == "fp16" else torch.bfloat16
        code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
        lin = GemLiteLinear(nbits, gs, K, N, code, code)
        lin.pack(W_q, torch.from_numpy(sc.astype(np.float32)).to(tdt).to(device), int(z), None, fma_mode=True)
    elif act == "fp8":
        lin = GemLiteLinear(nbits, gs, K, N, gemlite_amd.dtypes.TORCH_TO_DTYPE[torch.float8_e4m3fn], DType.BF16, scaled_activations=True)
        lin.pack(W_q, torch.from_numpy(sc.astype(np.float32)).to(torch.bfloat16).to(device), int(z), None, fma_mode=False)
    else:
        lin = GemLiteLinear(nbits, K, K, N, DType.INT8, DType.FP16, scaled_activations=True)
        lin.pack(W_q, torch.full((N, 1), 2.0 ** -6, dtype=torch.float32, device=device), int(z), None)
        lin.W_group_mode, lin.channel_scale_mode = 1, 3
    assert lin.zeros.numel() == 1 and lin.zeros.dtype == torch.int32
    return lin


def scalar_admissions():
    """[(nbits, act, M, kernel)]: what the planner gives each combination, one M per distinct kernel (asked on the CPU)"""
    import ctypes as C
    from gemlite_amd import _hip
    out = []
    for nbits in SCALAR_BITS:
        for act in SCALAR_ACTS:
            lin = scalar_layer(nbits, act, 2 ** (nbits - 1), "cpu")
            seen = set()
            for M in scalar_ms(nbits, act):
                a = plan_args(lin, M)
                rc = _hip.load().gemlite_hip_query(C.byref(a))
                name = kernel_name(a) if rc == 0 else f"status {rc}"
                if name not in seen:
                    seen.add(name)
                    out.append((nbits, act, M, name))
    return out


def int8_reference(lin, x16):
    """int8 activations x integer codes: the exact integer sums, then (fp32(sum) * token scale) * 2^-6 in fp32 (the channel scale is a
    power of two, so every order of the two products rounds alike), rounded once to the output type"""
    xq, sx = O.scale_activations_per_token(x16, O.INT8)
    q_kn = O.unpack_over_cols(lin.W_q.data.cpu().numpy(), lin.W_nbits, lin.W_q.element_size() * 8).T.astype(np.float64)
    acc = xq @ (q_kn - float(lin.zeros.data.item()))
    assert float(np.abs(acc).max()) < 2 ** 24
    s = lin.scales.data.float().cpu().numpy().reshape(1, -1)
    y32 = (acc.astype(np.float32) * sx.astype(np.float32).reshape(-1, 1)) * s
    odt = gemlite_amd.dtypes.DTYPE_TO_TORCH[lin.output_dtype.value]
    return torch.from_numpy(y32).to(odt)


@pytest.mark.parametrize("act", SCALAR_ACTS)
@pytest.mark.parametrize("nbits", SCALAR_BITS)
def test_scalar_zero_points_over_the_code_range(nbits, act):
    from tests.test_abi_bounds_gpu import _quantised_inputs, _raw, _run
    combos = [c for c in scalar_admissions() if c[:2] == (nbits, act)]
    assert combos and not any(c[3].startswith("status") for c in combos), combos
    bad = []
    for _, _, M, name in combos:
        case = dict(recipe=dict(kind="scalar", N=SCALAR_N, K=SCALAR_K), M=M, tuning=(0, 0, 0, 0), fused=False, name=name)
        for z in scalar_zero_values(nbits):
            lin = scalar_layer(nbits, act, z, DEV)
            assert kernel_name(plan_args(lin, M)) == name
            tag = f"scalar-z{z}-w{nbits}-{act}-M{M}-{name}"
            if act == "int8":
                x16 = make_x(launch_rows(M, ("amp1e-1", "mean", "amp1e-3"))[0], SCALAR_K, torch.float16, 400 + M).to(DEV)
                xk, sx = _quantised_inputs(lin, x16, False)
                y, got, _ = _run(lin, case, xk, sx, None)
                assert got == name
                ref = int8_reference(lin, x16)
                ne = _raw(y.cpu()) != _raw(ref)
                if bool(ne.any()):
                    m, n = [int(v) for v in ne.nonzero()[0]]
                    bad.append(f"{tag}: {int(ne.sum())} outputs differ from the integer oracle, first ({m}, {n}): {float(y[m, n])} vs {float(ref[m, n])}")
                continue
            b, _ = _sweep(lin, case, tag, {f"z{z}": np.arange(SCALAR_N)}, seed=400 + M)
            bad += [f"{tag}: row {r['row']} ({r['act']}) ratio {r['ratio']} mean|d| {r['mean_abs_d']:.3e}" for r in b]
    assert not bad, "\n".join(bad[:20])
