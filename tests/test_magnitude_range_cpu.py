"""The row gate and the case list of tests/test_magnitude_range_gpu.py, without a GPU.

The gate exists for a blind spot of test_gpu_parity._compare: it normalises by the mean |y| of the whole output, so a row of
1e-3 amplitude inside an output of amplitude 1 can come back zeroed, or 1 % off, and pass.  These tests pin that the row gate
rejects such a row while _compare's arithmetic accepts it, and that the GPU module sweeps every launch site of CASES with every
activation profile."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemlite_amd import _hip
from tests import test_magnitude_range_gpu as MR
from tests.test_abi_bounds_cpu import CASES, case_id, kernel_name, plan_args
from tests.test_gpu_parity import REL_TOL

FP16 = 1


def _compare_accepts(y, y_ref, tol):
    """test_gpu_parity._compare's gates (whole-output normalisation), without its report"""
    err = np.abs(y - y_ref)
    scale = max(float(np.abs(y_ref).mean()), 1e-12)
    return (err.mean() / scale < tol and err.max() / scale < 60 * tol
            and not (err > 10 * tol * scale + 4 * tol * np.abs(y_ref)).any() and (scale >= 5.0 or err.mean() < 1e-3))


def _output(M=8, N=512, seed=0):
    rng = np.random.default_rng(seed)
    y_ref = rng.standard_normal((M, N))
    y_ref[3] *= 1e-3
    y = (y_ref * (1 + rng.standard_normal((M, N)) * 1e-4)).astype(np.float16).astype(np.float64)  # output rounding + small noise
    return y, y_ref


@pytest.mark.parametrize("how", ["zeroed", "one_percent_off"])
def test_row_gate_rejects_a_small_row_that_the_whole_output_gate_accepts(how):
    y, y_ref = _output()
    tol = REL_TOL[FP16]
    assert _compare_accepts(y, y_ref, tol) and all(r["ok"] for r in MR.row_gate(y, y_ref, FP16, tol))
    y[3] = 0.0 if how == "zeroed" else y_ref[3] * 1.01
    assert _compare_accepts(y, y_ref, tol), "the whole-output gate is expected to miss this row"
    recs = MR.row_gate(y, y_ref, FP16, tol)
    assert [r["row"] for r in recs if not r["ok"]] == [3]


def test_row_gate_zero_rows_must_be_exactly_zero():
    y_ref = np.zeros((2, 64))
    y_ref[0] = 1.0
    y = y_ref.copy()
    assert all(r["ok"] for r in MR.row_gate(y, y_ref, FP16, 1e-3))
    y[1, 5] = 2.0 ** -24
    assert [r["ok"] for r in MR.row_gate(y, y_ref, FP16, 1e-3)] == [True, False]


def test_row_gate_allows_the_output_quantum_and_nothing_more():
    """a row near fp16's subnormal range: the output's rounding to the 2^-24 grid passes, a 5 % error does not"""
    rng = np.random.default_rng(3)
    y_ref = rng.standard_normal((1, 256)) * 2.0 ** -20
    y = y_ref.astype(np.float16).astype(np.float64)
    assert MR.row_gate(y, y_ref, FP16, MR.EXACT_TOL)[0]["ok"]
    assert not MR.row_gate(y_ref * 1.05, y_ref, FP16, MR.EXACT_TOL)[0]["ok"]
    assert not MR.row_gate(np.where(np.arange(256) == 9, np.nan, y), y_ref, FP16, MR.EXACT_TOL)[0]["ok"]


def test_the_sweep_is_exactly_the_abi_case_table():
    assert MR.SKIP == {}  # nothing is left out; a skip would need its reason here
    assert [case_id(c) for c in MR.SWEEP] == [case_id(c) for c in CASES]
    assert MR.SWEEP == CASES


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_every_profile_reaches_a_row_of_every_case(tdt):
    profs = MR.profiles_for(tdt)
    assert ("subnormal" in profs) == (tdt == torch.float16)
    for c in CASES:
        rows = MR.launch_rows(c["M"], profs)
        assert all(len(r) == c["M"] for r in rows)
        assert set(p for r in rows for p in r) == set(profs), case_id(c)
        assert len(rows) == -(-len(profs) // c["M"])  # no launch more than needed


def test_profiles_have_the_magnitudes_they_name():
    rng = np.random.default_rng(0)
    K = 4096
    for amp in (1e-4, 1e-3, 1e-1, 10):
        r = MR.profile_row(f"amp{amp:g}", K, rng)
        assert 0.9 * amp < r.std() < 1.1 * amp
    r = MR.profile_row("outliers", K, rng)
    assert K // 200 <= (np.abs(r) > 1).sum() <= K // 100 and np.median(np.abs(r)) < 0.1  # N(0, 0.1) alone never reaches 1
    r = MR.profile_row("mean", K, rng)
    assert abs(r.mean() - 0.5) < 0.01
    assert not MR.profile_row("zeros", K, rng).any()
    x = MR.make_x(["subnormal"], K, torch.float16, 0).float().numpy()
    assert (x != 0).all() and (np.abs(x) < 2.0 ** -14).all()
    assert np.array_equal(x, MR.profile_row("subnormal", K, np.random.default_rng(0)).reshape(1, -1))  # exact in fp16


def test_weight_scale_sweep_cases_plan_the_kernels_they_name():
    names = [c["name"] for c in MR.SCALE_CASES]
    for want in ("gemm_wn_direct_kernel<tile32,8w>", "gemm_wn_stream_kernel", "mx_gemv_w8_kernel", "mx_gemv_w4_kernel"):
        assert want in names
    kinds = {(c["recipe"]["kind"], c["recipe"].get("nbits")) for c in MR.SCALE_CASES}
    assert {("wn", 1), ("wn", 2), ("wn", 4), ("wn", 8), ("a8w4", None), ("a8w2", None), ("mx16w4", None), ("mx16w8", None),
            ("mx44", None), ("mx84", None), ("mx88", None)} <= kinds
    for c in MR.SCALE_CASES:
        for which in (0, 1):
            tdt = c["recipe"].get("tdt", torch.float16)
            lin = MR.scaled_layer(c["recipe"], MR.scale_factors(tdt, c["recipe"].get("nbits"))[which], "cpu")
            a = plan_args(lin, c["M"], c["tuning"], c["fused"])
            assert _hip.load().gemlite_hip_query(C.byref(a)) == 0
            assert kernel_name(a) == c["name"], case_id(c)


def test_small_weight_scales_keep_fp16_dequantised_weights_normal():
    """fp16 layers of the sweep: every non-zero |(q - z) s| at or above 2^-14 (a kernel that dequantises into fp16 then rounds only
    where the reference rounds)"""
    for c in MR.SCALE_CASES:
        r = c["recipe"]
        if r["kind"] not in ("wn", "a8w4", "a8w2") or r.get("tdt", torch.float16) != torch.float16:
            continue
        lin = MR.scaled_layer(r, MR.scale_factors(torch.float16)[0], "cpu")
        s = lin.scales.data.float().numpy().astype(np.float64)
        assert s.min() >= 2.0 ** -14, (case_id(c), s.min())  # and |q - z| >= 1 where non-zero: integer zero points


def test_fp16_e4m3_band_is_exact_where_the_sweep_keeps_it_and_only_there():
    """the e = -15 .. -12 band the fp16 A16W8_MXFP rows / tile kernels are swept on holds every e4m3 value times 2^e exactly in fp16;
    e = -16 (the band mx_gemv_w8_kernel is held to) does not"""
    from oracle import mx_oracle as MX
    v = MX.fp8_e4m3_decode(np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)).astype(np.float64)
    lo, hi = MR.FP16_E4M3_EXACT_BAND
    for byte in range(lo, hi + 1):
        w = v * 2.0 ** (byte - 127)
        assert np.array_equal(w.astype(np.float16).astype(np.float64), w), byte
    w = v * 2.0 ** -16
    assert not np.array_equal(w.astype(np.float16).astype(np.float64), w)
