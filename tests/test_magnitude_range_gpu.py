"""Every kernel across activation and weight-scale magnitudes, checked row by row (run on a real MI355X via `pytest -m gpu`).

test_gpu_parity._compare normalises by the mean |y| of the WHOLE output, so a row whose activations are 1000x smaller than its
neighbours' can come back wrong (or zero) and still pass.  Here every output row is held against its own float64 oracle row:
  row gate    mean|err_row| / mean|y_ref_row| < tol + q / mean|y_ref_row|, and elementwise |err| <= 10 tol mean|y_ref_row| +
              4 tol |y_ref| + q, where q is the output's absolute quantum (2^-25 for fp16, 2^-134 for bf16: half the smallest
              subnormal) and tol the number the family is held to by the parity gates (REL_TOL by output type); 16-bit activations x
              packed words on kernels whose unpack is exact are held to the decode-kernel contract, 4e-4 for fp16 out.  A row whose
              oracle is exactly zero must come back exactly zero.
Kernel set: every entry of tests/test_abi_bounds_cpu.py::CASES (same layer recipe, M and forced tuning), dense tensors, through
gemlite_hip_forward; 8-bit and block-scaled activations go through the library's quantiser and the oracle runs on the quantised
inputs (test_abi_bounds_gpu._oracle).
Activation profiles: row m of a launch takes profile m mod P (a case with M < P takes several launches), so mixed magnitudes share one
row tile.  Weight-scale sweep: one case per packed family and bit width with the group scales multiplied by a small and a large factor,
MX layers with e8m0 scale bytes spread around 127.  Per-row numbers join the JSON report of test_gpu_parity (its REPORT list and
module fixture, imported here), tagged act/... and scale<factor>/...."""
import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear
from gemlite_amd import helper as H
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, kernel_name, plan_args
from tests.test_gpu_parity import REL_TOL, REPORT
from tests.test_gpu_parity import _report  # noqa: F401  (autouse here too: writes REPORT, these rows included, when the module ends)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# ------------------------------------------------------------------------------------------------ activation profiles
PROFILES = ("amp1e-4", "amp1e-3", "amp1e-1", "amp10", "outliers", "mean", "zeros", "subnormal")
Y_LIMIT = 2.0 ** 14  # |y_ref| stays below this: output overflow is not what is tested


def profiles_for(x_dtype):
    """the profiles a case whose 16-bit activations are `x_dtype` takes (fp16 subnormals exist in fp16 only)"""
    return PROFILES if x_dtype == torch.float16 else tuple(p for p in PROFILES if p != "subnormal")


def launch_rows(M, profs):
    """[launch][row] -> profile name: row m of launch l takes profs[(l M + m) mod P]; enough launches for every profile to get a row"""
    P = len(profs)
    return [[profs[(l * M + m) % P] for m in range(M)] for l in range(-(-P // M))]


def profile_row(name, K, rng):
    """one row of K activations (float32, before the cast to the case's 16-bit type)"""
    if name.startswith("amp"):
        return (rng.standard_normal(K) * float(name[3:])).astype(np.float32)
    if name == "outliers":  # LLM-style outlier channels: 1 % of k at x300 over N(0, 0.1)
        r = rng.standard_normal(K) * 0.1
        idx = rng.choice(K, max(1, K // 100), replace=False)
        r[idx] *= 300.0
        return r.astype(np.float32)
    if name == "mean":  # non-zero mean: exercises the OFF sum(x) and z sum(x) cancellations
        return (0.5 + rng.standard_normal(K) * 0.05).astype(np.float32)
    if name == "zeros":
        return np.zeros(K, np.float32)
    if name == "subnormal":  # every non-zero value an fp16 subnormal (|v| = n 2^-24, 1 <= n <= 1023)
        n = rng.integers(1, 1024, K) * rng.choice((-1.0, 1.0), K)
        return (n * 2.0 ** -24).astype(np.float32)
    raise ValueError(name)


def make_x(rows, K, tdt, seed):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([profile_row(p, K, rng) for p in rows])).to(tdt)


# ------------------------------------------------------------------------------------------------ the row gate
QUANTUM = {1: 2.0 ** -25, 2: 2.0 ** -134, 0: 0.0}  # half the smallest subnormal of the output type, by output dtype code


def row_gate(y, y_ref, out_code, tol):
    """per-row records of y against y_ref [M, N] (float64 arrays); rec['ok'] is the verdict of the row gate"""
    y = np.asarray(y, np.float64)
    y_ref = np.asarray(y_ref, np.float64).reshape(y.shape)
    q = QUANTUM[out_code]
    recs = []
    for m in range(y.shape[0]):
        err = np.abs(y[m] - y_ref[m])
        scale = float(np.abs(y_ref[m]).mean())
        finite = bool(np.isfinite(y[m]).all())
        rec = dict(row=m, mean_abs_ref=scale, mean_abs_err=float(err.mean()), max_abs_err=float(err.max()), finite=finite, tol=tol)
        if scale == 0.0:  # the relative gate is undefined: the row must be exactly zero
            rec["rel_mean"] = None
            rec["ok"] = finite and bool((y[m] == 0).all())
        else:
            rec["rel_mean"] = float(err.mean() / scale)
            viol = err > 10 * tol * scale + 4 * tol * np.abs(y_ref[m]) + q
            rec["elementwise_violations"] = int(viol.sum())
            rec["ok"] = finite and rec["rel_mean"] < tol + q / scale and rec["elementwise_violations"] == 0
        recs.append(rec)
    return recs


# 16-bit activations x packed words on kernels that unpack the codes exactly and accumulate in fp32 (subnormal / magic-number
# unpack, scale and zero applied to the fp32 sums): the decode-kernel contract.  The MFMA tile kernels dequantise the weight to the
# 16-bit type before the product (rounds where the reference rounds, gemm_wn_mma_kernel.inc) and keep REL_TOL.
EXACT_UNPACK = ("gemv_w4_decode", "gemv_wn_kernel", "gemv_mfma_kernel", "gemv_w2_mfma_kernel", "gemm_wn_direct_kernel",
                "gemm_wn_stream_kernel", "gemm_w4_rows_kernel", "gemm_w2_rows_kernel")
EXACT_TOL = 4e-4


def tol_of(lin, name, out_code):
    if out_code == 1 and lin.input_dtype == DType.FP16 and lin.elements_per_sample > 1 and name.startswith(EXACT_UNPACK):
        return EXACT_TOL
    return REL_TOL[out_code]


# ------------------------------------------------------------------------------------------------ the kernel set
# case_id -> reason; every entry of CASES not named here is swept (tests/test_magnitude_range_cpu.py checks the list)
SKIP = {}
SWEEP = [c for c in CASES if case_id(c) not in SKIP]


def _x_dtype(lin):
    return torch.bfloat16 if lin.output_dtype in (DType.BF16, DType.MXBF16) else torch.float16


def _sweep(lin, case, tag, profs, seed):
    """run every launch of `case` on `lin` with profile rows; returns the failing row records"""
    from tests.test_abi_bounds_gpu import _oracle, _quantised_inputs, _run
    M, K = case["M"], lin.in_features
    tdt = _x_dtype(lin)
    out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    bad = []
    for li, rows in enumerate(launch_rows(M, profs)):
        x16 = make_x(rows, K, tdt, seed + li).to(DEV)
        xk, sx = _quantised_inputs(lin, x16, case["fused"])
        res = _run(lin, case, xk, sx, None)
        assert res is not None
        y, name, _ = res
        assert name == case["name"], name
        y_ref, _ = _oracle(lin, x16, name)
        y_ref = np.asarray(y_ref, np.float64).reshape(M, -1)
        assert float(np.abs(y_ref).max()) < Y_LIMIT, (tag, float(np.abs(y_ref).max()))
        tol = tol_of(lin, name, out_code)
        for rec in row_gate(y.float().cpu().numpy(), y_ref, out_code, tol):
            rec.update(tag=tag, kernel=name, launch=li, profile=rows[rec["row"]])
            REPORT.append(rec)
            if not rec["ok"]:
                bad.append(rec)
    return bad


def _fmt(bad):
    return "\n".join(f"  row {r['row']} ({r['profile']}, launch {r['launch']}): rel {r['rel_mean']} tol {r['tol']} "
                     f"mean|y_ref| {r['mean_abs_ref']:.3e} max|err| {r['max_abs_err']:.3e} viol {r.get('elementwise_violations')}"
                     for r in bad[:12])


@pytest.mark.parametrize("case", SWEEP, ids=case_id)
def test_every_kernel_holds_each_row_across_activation_magnitudes(case):
    lin = build_layer(case["recipe"], DEV)
    assert kernel_name(plan_args(lin, case["M"], case["tuning"], case["fused"])) == case["name"]
    profs = profiles_for(_x_dtype(lin))
    bad = _sweep(lin, case, "act/" + case_id(case), profs, seed=case["M"])
    assert not bad, f"{case['name']}: {len(bad)} rows fail the row gate\n{_fmt(bad)}"


# ------------------------------------------------------------------------------------------------ weight-scale sweep
PACKED = ("wn", "a8w4", "a8w2", "mx16w4", "mx16w8", "mx44", "mx84", "mx88")


def _scale_cases():
    """the first default-planned case of every packed layer family, bit width and kernel family in CASES, plus launch sites the
    table holds only under other settings: the streaming kernel and the MX decode kernels under fp16 activations (both forced, as
    CASES forces them), and the default kernels of fp16 A16W8_MXFP layers (CASES runs them in bf16, where e4m3 x 2^e is exact)"""
    out, seen = [], set()
    for c in CASES:
        r = c["recipe"]
        key = (r["kind"], r.get("nbits"), c["name"].split("<")[0])
        if r["kind"] in PACKED and c["tuning"] == (0, 0, 0, 0) and not c["fused"] and key not in seen:
            seen.add(key)
            out.append(c)
    out += [c for c in CASES if c["name"] == "gemm_wn_stream_kernel"]
    out += [dict(recipe=dict(kind="mx16w8", N=1024, K=512), M=2, tuning=(5, 0, 0, 0), fused=False, name="mx_gemv_w8_kernel"),
            dict(recipe=dict(kind="mx16w4", N=1024, K=512), M=3, tuning=(5, 0, 0, 0), fused=False, name="mx_gemv_w4_kernel"),
            dict(recipe=dict(kind="mx16w8", N=1024, K=512), M=1, tuning=(0, 0, 0, 0), fused=False, name="a16w8_mxfp_rows_kernel<16x16>"),
            dict(recipe=dict(kind="mx16w8", N=1024, K=512), M=129, tuning=(0, 0, 0, 0), fused=False, name="gemm_a16w8_mxfp_kernel<128x128>")]
    return out


SCALE_CASES = _scale_cases()
# profiles of the sweep: |y_ref| < 2^14 under the large factor (amplitude 10 and the outlier channels would leave it)
SCALE_PROFILES = ("amp1e-4", "amp1e-3", "amp1e-1", "mean", "zeros")


def scale_factors(tdt, nbits=None):
    """(small, large) group-scale factors.  fp16 keeps |(q - z) s| normal (kernels that dequantise to fp16 round where the reference
    rounds): with integer zero points and s >= 0.001 / 16 every non-zero product is >= 2^-14.  bf16 has fp32's exponent range.
    8-bit words (|q - z| up to 255) take 10 instead of 100, which keeps the non-zero-mean row's |y_ref| below 2^14."""
    return (1.0 / 16 if tdt == torch.float16 else 1e-3), (1e1 if nbits == 8 else 1e2)


# Measured and kept: the fp16 forms of the A16W8_MXFP rows and tile kernels convert each e4m3 weight together with its block's 2^e into
# fp16 before the product (v_cvt_scalef32_pk_f16_fp8 with the scale; the tile kernel dequantises the way the reference's kernels do,
# into the activations' type).  e4m3 x 2^e is exact in fp16 only for e >= -15; at e = -19 .. -16 the weights land on fp16's
# subnormal grid and rows with a non-zero mean come out 2.5e-3 of their mean |y| off (both kernels, 1024 x 512, on an MI355X).  Their
# small-scale sweep therefore stays on e = -15 .. -12, where that conversion is exact; mx_gemv_w8_kernel applies 2^e to its fp32 sums
# and takes the full e = -19 .. -16 band.
FP16_E4M3_ROUNDING = {"a16w8_mxfp_rows_kernel", "gemm_a16w8_mxfp_kernel"}
FP16_E4M3_EXACT_BAND = (112, 115)


def scaled_layer(r, factor, device, seed=0, band=None):
    """the layer of recipe r with its group scales multiplied by `factor` (packed integer words), or with random e8m0 scale bytes
    (MX).  factor < 1: 107 .. 111 (e = -20 .. -16; fp8 weights 108 .. 111), every block small, so that an e4m3 value times 2^e, which
    fp16 holds only inexactly for e <= -16, is not hidden behind larger blocks.  Else 127 .. 135 for fp8 weights (e >= 8: the largest
    e4m3 values overflow fp16) and 127 .. 132 for fp4 weights, where |y_ref| < 2^14 ends it."""
    kind, N, K = r["kind"], r["N"], r["K"]
    tdt = r.get("tdt", torch.float16)
    if kind in ("wn", "a8w4", "a8w2"):
        nbits = r.get("nbits", 4 if kind == "a8w4" else 2)
        W_q, sc, zr = O.gen_data(N, K, nbits, r["gs"], seed=seed, np_float=np.float32)
        sc = sc * np.float32(factor)
        if tdt == torch.float16 and factor < 1:
            zr = np.round(zr)
        sc_t, zr_t = torch.from_numpy(sc).to(tdt), torch.from_numpy(zr).to(tdt)
        if kind == "wn":
            code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
            lin = GemLiteLinear(nbits, r["gs"], K, N, code, code)
            lin.pack(torch.from_numpy(W_q).to(device), sc_t.to(device), zr_t.to(device), None, fma_mode=True)
            return lin
        return H.A8Wn_HQQ_INT_dynamic(device=device, dtype=tdt, W_nbits=nbits).from_weights(torch.from_numpy(W_q), sc_t, zr_t)
    lin = build_layer(r, device, seed)
    w8 = kind in ("mx16w8", "mx88")
    lo, hi = ((108, 111) if w8 else (107, 111)) if factor < 1 else ((127, 135) if w8 else (127, 132))
    if band is not None:
        lo, hi = band
    s = lin.scales.data.view(torch.uint8)
    g = torch.Generator().manual_seed(seed + 7)
    s.copy_(torch.randint(lo, hi + 1, tuple(s.shape), generator=g, dtype=torch.uint8).to(s.device))
    return lin


@pytest.mark.parametrize("which", ["small", "large"])
@pytest.mark.parametrize("case", SCALE_CASES, ids=case_id)
def test_packed_families_hold_each_row_across_weight_scales(case, which):
    r = case["recipe"]
    tdt = r.get("tdt", torch.float16)
    factor = scale_factors(tdt, r.get("nbits"))[which == "large"]
    rounds = tdt == torch.float16 and r["kind"] == "mx16w8" and case["name"].split("<")[0] in FP16_E4M3_ROUNDING
    lin = scaled_layer(r, factor, DEV, band=FP16_E4M3_EXACT_BAND if (rounds and which == "small") else None)
    assert kernel_name(plan_args(lin, case["M"], case["tuning"], case["fused"])) == case["name"]
    bad = _sweep(lin, case, f"scale{factor:g}/" + case_id(case), SCALE_PROFILES, seed=case["M"] + 100)
    assert not bad, f"{case['name']} (scales x {factor:g}): {len(bad)} rows fail the row gate\n{_fmt(bad)}"
