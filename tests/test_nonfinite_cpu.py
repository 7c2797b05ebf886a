"""Helpers and gates of tests/test_nonfinite_gpu.py, and their self-tests without a GPU.

Four properties no other module looks at, because every other input of the suite is finite and moderate:
  isolate   a NaN / Inf in token r of a batch leaves every other token's output (and quantised row, and scale) as it was, bit for bit;
  visible   ... and every element of token r's output is NaN or +-Inf (a quantiser built on fmaxf / fminf drops a NaN and returns a
            plausible finite row);
  overflow  an fp16 output at or above 65520 in magnitude is +-Inf with the oracle's sign, one below 65504 is finite and right (an
            fp32 accumulator cast to fp16, the reference's contract; a clamp or a round-toward-zero convert would answer 65504);
  wide      bf16 rows of amplitude 2^40 and 2^-40 next to an ordinary row in one tile (a bf16 path through fp16 would lose both).
Each gate here is a plain function of arrays; the self-tests hand it one array it must pass and one it must fail.  The CPU tests also
recompute, from the float64 oracle alone, the amplitude table of the overflow cases and the finiteness of the 2^40 oracle."""
import numpy as np
import pytest
import torch

from gemlite_amd import DType
from oracle import gemlite_oracle as O
from oracle import mx_oracle as MX
from tests import test_magnitude_range_gpu as MR
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, cpu_layer, kernel_name, plan_args, scales_x_kind

FP16, BF16 = 1, 2
DIRECT_CODES = (DType.FP16, DType.BF16, DType.MXFP16, DType.MXBF16)


def is_direct(lin, fused):
    """the matmul kernel reads the 16-bit x itself (no activation quantiser in front of it or inside it)"""
    return not fused and lin.input_dtype in DIRECT_CODES


DIRECT_KINDS = ("wn", "bitnet16", "a16w8i", "a16w8f", "mx16w4", "mx16w8")


def case_is_direct(case):
    """is_direct from the recipe alone (test_direct_and_quantised_split holds the two together)"""
    return not case["fused"] and case["recipe"]["kind"] in DIRECT_KINDS


def is_big(case):
    """the 4096^2 entries of CASES: parts 1 and 2 only (they need no oracle)"""
    return case["recipe"]["N"] * case["recipe"]["K"] >= 4096 * 4096


def x_dtype(lin):
    return torch.bfloat16 if lin.output_dtype in (DType.BF16, DType.MXBF16) else torch.float16


# ------------------------------------------------------------------------------------------------ poisoned launches
KINDS = ("nan", "inf", "inf-inf")


def poison_rows(M):
    """first, last and (from four rows) a middle row"""
    return sorted({0, M - 1} | ({M // 2} if M >= 4 else set()))


def launches(M):
    """[(poisoned row, kind)], one launch each: every poison row once and every kind at least once (kinds cycle over the launches;
    with fewer than three rows the rows come round again)"""
    rows = poison_rows(M)
    return [(rows[i % len(rows)], KINDS[i % 3]) for i in range(max(len(rows), 3))]


def quant_group(lin):
    g = lin.group_size
    return g if g and 0 < g < lin.in_features else 32


def poison_ks(kind, K, group, rng):
    """[(k, value)] of one poisoned row.  inf-inf: +Inf and -Inf in different 512-element chunks where K holds two, else in different
    quantisation groups, else in different halves of the row"""
    if kind == "nan":
        return [(int(rng.integers(K)), float("nan"))]
    if kind == "inf":
        return [(int(rng.integers(K)), float("inf"))]
    chunk = 512 if K >= 1024 else (group if K >= 2 * group else K // 2)
    c0, c1 = (int(c) for c in rng.choice(K // chunk, 2, replace=False))
    return [(c0 * chunk + int(rng.integers(chunk)), float("inf")), (c1 * chunk + int(rng.integers(chunk)), float("-inf"))]


def poison(x16, r, kind, group, seed):
    """(copy of x16 with row r poisoned, the [(k, value)] used)"""
    ks = poison_ks(kind, x16.shape[1], group, np.random.default_rng(seed))
    x = x16.clone()
    for k, v in ks:
        x[r, k] = v
    return x, ks


# ------------------------------------------------------------------------------------------------ gates of parts 1 and 2
def isolation_gate(bits, bits_clean, r):
    """rows m != r whose raw bits differ from the clean launch's (the gate passes on an empty list)"""
    bits, bits_clean = np.asarray(bits), np.asarray(bits_clean)
    assert bits.shape == bits_clean.shape and bits.dtype == bits_clean.dtype and bits.dtype.kind in "iu"
    rows = bits.reshape(bits.shape[0], -1) != bits_clean.reshape(bits.shape[0], -1)
    return [int(m) for m in np.nonzero(rows.any(axis=1))[0] if m != r]


def visible_gate(y_row):
    """number of FINITE elements of a poisoned row's output (the gate passes on zero: no tolerance, no element left out)"""
    return int(np.isfinite(np.asarray(y_row, np.float64)).sum())


E8M0_NAN, E4M3_NAN = 0xFF, 0x7F


def block_scale_gate(scale_row, blocks, nan_code):
    """block scales of the library's own quantiser: every poisoned block carries the format's NaN code (stricter than "or the row's
    output is non-finite", which the visibility gate asks of every row anyway: this is what pins the quantiser's scale byte)"""
    return all(int(scale_row[b]) == nan_code for b in blocks)


# ------------------------------------------------------------------------------------------------ part 4: fp16 output overflow
F16_MAX = 65504.0        # largest finite fp16
F16_TO_INF = 65520.0     # round-to-nearest-even sends |y| >= 65520 to Inf


def overflow_classes(y_ref_row, tol):
    """(over, under) masks of one oracle row; what is in neither is the band where either result is accepted"""
    a = np.abs(np.asarray(y_ref_row, np.float64))
    return a > F16_TO_INF * (1 + 4 * tol), a < F16_MAX * (1 - 4 * tol)


def overflow_shares(y_ref, tol):
    """per row (over, under, band) as fractions of the row"""
    out = []
    for row in np.asarray(y_ref, np.float64):
        over, under = overflow_classes(row, tol)
        out.append((float(over.mean()), float(under.mean()), float((~over & ~under).mean())))
    return out


def shares_ok(shares):
    return all(band <= 0.02 and over >= 0.10 and under >= 0.10 for over, under, band in shares)


def overflow_gate(y, y_ref, tol):
    """per-row records of an fp16 output y against the oracle: over -> exactly +-Inf with the oracle's sign; under -> finite and inside
    the elementwise bound of MR.row_gate (10 tol mean|y_ref_row| + 4 tol |y_ref| + q); band -> anything"""
    y = np.asarray(y, np.float64)
    y_ref = np.asarray(y_ref, np.float64).reshape(y.shape)
    q = MR.QUANTUM[FP16]
    recs = []
    for m in range(y.shape[0]):
        over, under = overflow_classes(y_ref[m], tol)
        scale = float(np.abs(y_ref[m]).mean())
        want = np.where(y_ref[m] > 0, np.inf, -np.inf)
        bad_over = over & ~(np.isinf(y[m]) & (y[m] == want))
        with np.errstate(invalid="ignore"):
            err = np.abs(y[m] - y_ref[m])
            bad_under = under & ~(np.isfinite(y[m]) & (err <= 10 * tol * scale + 4 * tol * np.abs(y_ref[m]) + q))
        recs.append(dict(row=m, over=int(over.sum()), under=int(under.sum()), band=int((~over & ~under).sum()),
                         over_not_inf=int(bad_over.sum()), under_wrong=int(bad_under.sum()), mean_abs_ref=scale, tol=tol,
                         ok=not bad_over.any() and not bad_under.any()))
    return recs


# Cases: the fp16 entries of the weight-scale sweep at its large factor, plus the fp16 direct entries of CASES whose kernel family the
# sweep does not hold (the unpacked 8-bit weights: their channel scales take the factor).
OVERFLOW_UNPACKED_FACTOR = 100.0


def _overflow_cases():
    fp16 = [c for c in MR.SCALE_CASES if c["recipe"].get("tdt", torch.float16) == torch.float16]
    have = {c["name"].split("<")[0] for c in fp16}
    for c in CASES:
        fam = c["name"].split("<")[0]
        if c["recipe"].get("tdt", torch.float16) == torch.float16 and fam not in have and case_is_direct(c):
            have.add(fam)
            fp16.append(c)
    return fp16


OVERFLOW_CASES = _overflow_cases()


def overflow_layer(r, device):
    if r["kind"] in MR.PACKED:
        return MR.scaled_layer(r, MR.scale_factors(torch.float16, r.get("nbits"))[1], device)
    lin = build_layer(r, device)
    assert lin.scales.numel() == r["N"] and lin.scales.is_floating_point(), r  # per-channel weight scales
    lin.scales.data.mul_(OVERFLOW_UNPACKED_FACTOR)
    return lin


# case_id -> amplitude A of the N(0, A) rows.  Derived on the CPU from the oracle alone (the smallest two-digit A at which 40 % of
# |y_ref| lies above 65520; test_overflow_amplitudes_give_the_shares_the_gate_needs recomputes the shares), never from a kernel.
OVERFLOW_A = {
    "gemv_wn_kernel<tile64>-wn-nbits1-gs32-1024x2048-M1": 4500,
    "gemv_w2_mfma_kernel<tile16>-wn-nbits2-gs128-3072x128-M1": 7600,
    "gemv_mfma_kernel<tile16,rows4>-wn-nbits4-gs128-1024x512-M3": 820,
    "gemm_wn_direct_kernel<tile32,8w>-wn-nbits4-gs128-4096x4096-M7": 290,
    "gemm_w2_rows_kernel<16x16>-wn-nbits2-gs32-1008x512-M33": 3700,
    "gemm_w4_mma_kernel<64x64>-wn-nbits4-gs128-4096x4096-M255": 300,
    "gemm_w1_mma_kernel<128x128>-wn-nbits1-gs64-1024x1024-M65": 6400,
    "gemm_w8_mma_kernel<64x128>-wn-nbits8-gs128-1024x512-M33": 540,
    "gemm_a8w2_mma_kernel<256x128>-a8w2-gs128-1024x512-M129": 3900,
    "a16w4_mxfp_rows_kernel<32x16>-mx16w4-1024x512-M17": 83,
    "gemm_a16w4_mxfp_kernel<128x128>-mx16w4-1024x512-M257": 83,
    "mx_rows_a4w4_kernel<32x16>-mx44-1024x512-M17": 83,
    "mx_rows_a8w4_kernel<16x16>-mx84-postTrue-1024x512-M15": 83,
    "mx_rows_a8w8_kernel<64x16>-mx88-postTrue-1024x512-M33": 65,
    "gemm_mx_a4w4_sq_kernel<64x64>-mx44-1024x512-M129": 83,
    "gemm_mx_a8w4_sq_kernel<64x64>-mx84-postTrue-1024x1024-M65": 57,
    "gemm_mx_a8w8_sq_kernel<64x64>-mx88-postTrue-1024x512-M127": 65,
    "gemm_wn_stream_kernel-wn-nbits4-gs128-1024x512-M17": 850,
    "mx_gemv_w8_kernel-mx16w8-1024x512-M2": 68,
    "mx_gemv_w4_kernel-mx16w4-1024x512-M3": 85,
    "a16w8_mxfp_rows_kernel<16x16>-mx16w8-1024x512-M1": 67,
    "gemm_a16w8_mxfp_kernel<128x128>-mx16w8-1024x512-M129": 65,
    "gemm_w4_rows_kernel<64x16>-wn-nbits4-gs128-4096x4096-M64": 300,
    "gemm_w2_mma_kernel<128x128>-wn-nbits2-gs128-4096x4096-M255": 1400,
    "a16w8_decode_kernel<tile16,16w>-a16w8i-1024x1024-M1": 740,
    "a16w8_rows_kernel<16x16>-a16w8i-1008x512-M3": 1100,
    "gemm_a16w8_kernel<128x128>-a16w8i-1024x512-M65": 1100,
}


def overflow_x(case, A):
    """[M, K] fp16 rows N(0, A), all finite"""
    r = case["recipe"]
    x = (np.random.default_rng(1000 + case["M"]).standard_normal((case["M"], r["K"])) * A).astype(np.float32)
    x16 = torch.from_numpy(x).to(torch.float16)
    assert bool(torch.isfinite(x16).all()), (case_id(case), A)
    return x16


# ------------------------------------------------------------------------------------------------ part 5: bf16 exponent range
WIDE_PROFILES = ("amp2^40", "amp1e-1", "amp2^-40")
WIDE_Y_LIMIT = 2.0 ** 100
WIDE_CASES = [c for c in CASES if c["recipe"].get("tdt", torch.float16) == torch.bfloat16 and not is_big(c)]


def wide_row(name, K, rng):
    """one row (float32, exact in bf16): amp2^e = standard normal values rounded to bf16, times 2^e"""
    if name.startswith("amp2^"):
        r = torch.from_numpy(rng.standard_normal(K).astype(np.float32)).to(torch.bfloat16).float().numpy()
        return r * np.float32(2.0 ** int(name[5:]))
    return MR.profile_row(name, K, rng)


def make_wide_x(rows, K, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([wide_row(p, K, rng) for p in rows])).to(torch.bfloat16)


# "<part>/<case_id>" or "wide/<profile>/<case_id>" -> reason.  Overflow: no finite fp16 x reaches the shares.  Wide: the oracle itself
# is not finite at that profile.  Empty: nothing is left out.
SKIP = {}


def wide_profiles_for(case):
    return tuple(p for p in WIDE_PROFILES if f"wide/{p}/{case_id(case)}" not in SKIP)


# ------------------------------------------------------------------------------------------------ the oracle without a GPU
def oracle_cpu(lin, x16, name):
    """tests.test_abi_bounds_gpu._oracle for a layer on the CPU: block-scaled activations go through the oracle's own quantisers (the
    library's are bit-identical to them: test_abi_bounds_gpu.test_activation_quantisers_stay_inside_their_outputs)"""
    from tests.test_abi_bounds_gpu import _oracle
    from tests.test_mx_gpu import _weights_nk
    code, g = lin.input_dtype, lin.group_size
    if code not in (DType.MXFP8, DType.MXFP4, DType.NVFP4):
        return np.asarray(_oracle(lin, x16, name)[0], np.float64)
    wv, ws = _weights_nk(lin)
    xf = x16.float().numpy()
    if code == DType.MXFP8 and lin.channel_scale_mode == 2:
        xq, sx = O.scale_activations_per_token(x16, O.FP8E4)
        return MX.mx_matmul(np.asarray(xq, np.float32), wv, sw=ws, group=g, scales_x_token=sx)
    if code == DType.MXFP8:
        xq, sx = MX.scale_activations_mxfp8(xf)
        return MX.mx_matmul(MX.fp8_e4m3_decode(xq), wv, sx=sx, sw=ws, group=g)
    nv = code == DType.NVFP4
    xq, sx = (MX.scale_activations_nvfp4 if nv else MX.scale_activations_mxfp4)(xf)
    return MX.mx_matmul(MX.fp4_unpack(xq), wv, sx=sx, sw=ws, group=g, e4m3_scales=nv, post=0.05 ** 2 if nv else 1.0)


# ================================================================================================ self-tests
def test_launches_poison_every_row_once_and_use_every_kind():
    assert poison_rows(1) == [0] and poison_rows(2) == [0, 1] and poison_rows(3) == [0, 2] and poison_rows(4) == [0, 2, 3]
    assert poison_rows(300) == [0, 150, 299]
    for c in CASES:
        ls = launches(c["M"])
        assert {r for r, _ in ls} == set(poison_rows(c["M"])), case_id(c)
        assert {k for _, k in ls} == set(KINDS), case_id(c)
        assert len(ls) == 3


def test_poison_positions():
    for K, group in ((4096, 128), (1024, 32), (512, 128), (512, 64), (64, 32), (128, 128), (256, 128)):
        for seed in range(20):
            rng = np.random.default_rng(seed)
            (k, v), = poison_ks("nan", K, group, rng)
            assert 0 <= k < K and v != v
            (k, v), = poison_ks("inf", K, group, rng)
            assert 0 <= k < K and v == float("inf")
            (k0, v0), (k1, v1) = poison_ks("inf-inf", K, group, rng)
            assert (v0, v1) == (float("inf"), float("-inf")) and 0 <= k0 < K and 0 <= k1 < K
            if K >= 1024:
                assert k0 // 512 != k1 // 512
            elif K >= 2 * group:
                assert k0 // group != k1 // group
            else:
                assert k0 // (K // 2) != k1 // (K // 2)
    x = torch.zeros(3, 64, dtype=torch.bfloat16)
    xp, ks = poison(x, 1, "inf-inf", 32, 0)
    assert not x.any() and bool(torch.isfinite(xp[[0, 2]]).all()) and int((~torch.isfinite(xp[1])).sum()) == 2


def test_isolation_gate_sees_one_changed_bit_in_another_row_and_ignores_the_poisoned_one():
    rng = np.random.default_rng(0)
    clean = rng.integers(-2 ** 15, 2 ** 15, (5, 64)).astype(np.int16)
    y = clean.copy()
    y[2] = -1  # the poisoned row may hold anything
    assert isolation_gate(y, clean, 2) == []
    y[4, 63] ^= 1
    assert isolation_gate(y, clean, 2) == [4]
    assert isolation_gate(y, clean, 4) == [2]
    zero = np.zeros((2, 4), np.int16)
    negzero = zero.copy()
    negzero[0, 1] = np.int16(-2 ** 15)  # -0.0 against +0.0: equal as numbers, different as bits
    assert isolation_gate(negzero, zero, 1) == [0]


def test_visible_gate_counts_every_finite_element():
    row = np.array([np.nan, np.inf, -np.inf, np.nan])
    assert visible_gate(row) == 0
    row[2] = 65504.0
    assert visible_gate(row) == 1
    assert visible_gate(np.zeros(8)) == 8


def test_block_scale_gate():
    s = np.full(16, 127, np.uint8)
    assert not block_scale_gate(s, [3], E8M0_NAN)
    s[3] = 254  # the clamped exponent
    assert not block_scale_gate(s, [3], E8M0_NAN)
    s[3] = 0xFF
    assert block_scale_gate(s, [3], E8M0_NAN)
    assert not block_scale_gate(s, [3, 4], E8M0_NAN)
    assert not block_scale_gate(s, [3], E4M3_NAN)


def _overflow_pair(N=1024, seed=0):
    rng = np.random.default_rng(seed)
    y_ref = rng.standard_normal((2, N)) * 70000.0
    with np.errstate(over="ignore"):
        y = y_ref.astype(np.float32).astype(np.float16).astype(np.float64)  # an fp32 accumulator cast to fp16
    return y, y_ref


def test_overflow_gate_accepts_the_cast_and_rejects_a_clamp_a_sign_and_a_wrong_finite_value():
    tol = 1e-3
    y, y_ref = _overflow_pair()
    assert shares_ok(overflow_shares(y_ref, tol))
    assert all(r["ok"] for r in overflow_gate(y, y_ref, tol))
    clamped = np.clip(y, -F16_MAX, F16_MAX)  # a saturating or round-toward-zero convert
    recs = overflow_gate(clamped, y_ref, tol)
    assert not any(r["ok"] for r in recs) and all(r["over_not_inf"] == r["over"] and r["under_wrong"] == 0 for r in recs)
    over = np.abs(y_ref[0]) > 70000
    flipped = y.copy()
    flipped[0, np.nonzero(over)[0][0]] *= -1  # Inf of the wrong sign
    assert [r["ok"] for r in overflow_gate(flipped, y_ref, tol)] == [False, True]
    nan = y.copy()
    nan[1, np.nonzero(np.abs(y_ref[1]) > 70000)[0][0]] = np.nan
    assert [r["ok"] for r in overflow_gate(nan, y_ref, tol)] == [True, False]
    early = y.copy()
    i = int(np.argmax(np.where(np.abs(y_ref[0]) < 60000, np.abs(y_ref[0]), 0)))
    early[0, i] = np.inf * np.sign(y_ref[0, i])  # Inf below the threshold
    assert [r["ok"] for r in overflow_gate(early, y_ref, tol)] == [False, True]
    off = y.copy()
    j = int(np.argmin(np.abs(y_ref[1])))
    off[1, j] += 2 * (10 * tol * np.abs(y_ref[1]).mean() + 4 * tol * abs(y_ref[1, j]))
    assert [r["ok"] for r in overflow_gate(off, y_ref, tol)] == [True, False]


def test_overflow_gate_leaves_the_band_alone():
    tol = 1e-3
    y_ref = np.array([[65504.0, 65519.0, 65520.0, 65600.0, -65510.0, 100.0, 70000.0, -70000.0]])
    over, under = overflow_classes(y_ref[0], tol)
    assert over.tolist() == [False] * 6 + [True, True] and under.tolist() == [False] * 5 + [True, False, False]
    for band in (65504.0, np.inf, -np.inf):
        y = np.array([[band] * 5 + [100.0, np.inf, -np.inf]])
        assert overflow_gate(y, y_ref, tol)[0]["ok"]
    assert not shares_ok(overflow_shares(y_ref, tol))  # 5 of 8 in the band


def test_wide_profiles_are_exact_in_bf16_and_have_the_magnitudes_they_name():
    K = 4096
    for e in (40, -40):
        r = wide_row(f"amp2^{e}", K, np.random.default_rng(0))
        assert 0.9 < r.std() / 2.0 ** e < 1.1
        assert np.array_equal(torch.from_numpy(r).to(torch.bfloat16).float().numpy(), r)
    x = make_wide_x(WIDE_PROFILES, K, 0).float().numpy()
    assert 0.09 < x[1].std() < 0.11 and np.isfinite(x).all()
    for c in WIDE_CASES:
        rows = MR.launch_rows(c["M"], WIDE_PROFILES)
        assert set(p for r in rows for p in r) == set(WIDE_PROFILES), case_id(c)


def test_case_lists():
    assert all(c in CASES or c in MR.SCALE_CASES for c in OVERFLOW_CASES)
    fams = {c["name"].split("<")[0] for c in OVERFLOW_CASES}
    for want in ("gemv_mfma_kernel", "gemm_wn_stream_kernel", "gemm_w4_mma_kernel", "a16w8_decode_kernel", "a16w8_rows_kernel",
                 "gemm_a16w8_kernel", "mx_gemv_w8_kernel", "gemm_a16w8_mxfp_kernel", "gemm_a8w2_mma_kernel"):
        assert want in fams, want
    direct16 = {c["name"].split("<")[0] for c in CASES if c["recipe"].get("tdt", torch.float16) == torch.float16 and case_is_direct(c)}
    assert direct16 <= fams, sorted(direct16 - fams)
    assert len(WIDE_CASES) >= 20 and all(x_dtype(cpu_layer(c["recipe"])) == torch.bfloat16 for c in WIDE_CASES)
    assert sorted(OVERFLOW_A) == sorted(case_id(c) for c in OVERFLOW_CASES if "overflow/" + case_id(c) not in SKIP)


def test_every_skip_names_a_case_and_a_reason():
    ids = {"overflow/" + case_id(c) for c in OVERFLOW_CASES} | {f"wide/{p}/{case_id(c)}" for c in WIDE_CASES for p in WIDE_PROFILES}
    for key, reason in SKIP.items():
        assert key in ids and len(reason) > 20, key
    assert SKIP == {}  # the goal; an entry needs its reason above


@pytest.mark.parametrize("case", [c for c in OVERFLOW_CASES if "overflow/" + case_id(c) not in SKIP], ids=case_id)
def test_overflow_amplitudes_give_the_shares_the_gate_needs(case):
    """per row of the oracle, at the case's A: band <= 2 %, over >= 10 %, under >= 10 %"""
    lin = overflow_layer(case["recipe"], "cpu")
    assert kernel_name(plan_args(lin, case["M"], case["tuning"], case["fused"])) == case["name"]
    M = case["M"]
    rows = sorted({0, M // 2, M - 1})  # rows are independent in the oracle: three of them keep this test short (the GPU test holds all)
    x16 = overflow_x(case, OVERFLOW_A[case_id(case)])[rows]
    y_ref = oracle_cpu(lin, x16, case["name"]).reshape(len(rows), -1)
    shares = overflow_shares(y_ref, MR.tol_of(lin, case["name"], FP16))
    assert shares_ok(shares), [s for s in shares if not shares_ok([s])][:4]


@pytest.mark.parametrize("case", WIDE_CASES, ids=case_id)
def test_wide_oracle_is_finite_and_below_the_limit(case):
    """the float64 oracle of one row per wide profile that is not skipped (rows are independent in the oracle): finite, |y_ref| < 2^100"""
    lin = cpu_layer(case["recipe"])
    rows = wide_profiles_for(case)
    y_ref = oracle_cpu(lin, make_wide_x(rows, lin.in_features, case["M"]), case["name"])
    assert np.isfinite(y_ref).all() and float(np.abs(y_ref).max()) < WIDE_Y_LIMIT, (rows, float(np.abs(y_ref).max()))


def test_direct_and_quantised_split():
    kinds = {c["recipe"]["kind"]: is_direct(cpu_layer(c["recipe"]), False) for c in CASES}
    assert kinds["wn"] and kinds["bitnet16"] and kinds["a16w8i"] and kinds["mx16w4"] and kinds["mx16w8"]
    assert not (kinds["a8w8i"] or kinds["a8w4"] or kinds["bitnet8"] or kinds["mx44"] or kinds["mx88"] or kinds["nv"])
    assert all(not is_direct(cpu_layer(c["recipe"]), True) for c in CASES if c["fused"])
    assert all(case_is_direct(c) == is_direct(cpu_layer(c["recipe"]), c["fused"]) for c in CASES)
    assert {scales_x_kind(cpu_layer(c["recipe"])) for c in CASES if not is_direct(cpu_layer(c["recipe"]), c["fused"])} == {"token", "block"}
