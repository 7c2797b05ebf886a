"""Non-finite activations, fp16 output overflow and bf16's exponent range, per kernel (run on a real MI355X via `pytest -m gpu`).

Every other module of the suite feeds finite, moderate activations.  Here every entry of tests/test_abi_bounds_cpu.py::CASES runs
through gemlite_hip_forward on its own small shape (dense layout, the guards of test_abi_bounds_gpu._run on) with
  isolate/   one row r of the batch poisoned (a NaN, a +Inf, or +Inf and -Inf), one launch per poisoned row: every other row equals
             the clean launch's as raw bits — the output and, for layers whose activations the library quantises in a launch of its
             own, the quantised rows and their scales too.  No oracle, no tolerance: same kernel, same plan, same workspace size.
  visible/   ... and every element of row r is NaN or +-Inf (which of the two is not constrained); a per-token scale of row r is
             non-finite, a poisoned block's scale byte is the format's NaN code.  One-row cases run this part alone.
  overflow/  fp16 outputs around 65504: rows N(0, A) with A from the oracle alone (tests/test_nonfinite_cpu.py::OVERFLOW_A), each
             element classed by the float64 oracle as over (must be +-Inf, oracle's sign), under (finite, inside the elementwise bound
             of the row gate) or band (within 4 tol of the threshold: either).
  wide/      bf16 cases: rows of amplitude 2^40 and 2^-40 share a tile with an ordinary row; the row gate of
             test_magnitude_range_gpu, unchanged, with |y_ref| < 2^100.
Gates, case lists and the amplitude table live in tests/test_nonfinite_cpu.py with their self-tests.  Per-row and per-launch records
join the JSON report of test_gpu_parity."""
import numpy as np
import pytest
import torch

import gemlite_amd
from oracle import gemlite_oracle as O
from tests import test_magnitude_range_gpu as MR
from tests import test_nonfinite_cpu as NF
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, kernel_name, plan_args, scales_x_kind
from tests.test_gpu_parity import REPORT
from tests.test_gpu_parity import _report  # noqa: F401  (autouse here too: writes REPORT, these rows included, when the module ends)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _bits(t):
    """raw bits of a tensor as a numpy integer array (16- / 32-bit floats, or bytes)"""
    from tests.test_abi_bounds_gpu import _raw
    if t.element_size() == 1:
        return t.contiguous().view(torch.uint8).cpu().numpy()
    return _raw(t).cpu().numpy()


# ------------------------------------------------------------------------------------------------ parts 1 and 2: one set of launches
_POISONED = {}


def _poisoned_launches(case):
    """the clean launch and every poisoned launch of `case`, run once and shared by the tests below:
    dict(clean=dict(ybits, xq, sx, ...), runs=[dict(r, kind, ks, yrow (row r as float64), ybits, xq, sx, ...)], own_quantiser, sk, ...)"""
    from tests.test_abi_bounds_gpu import _quantised_inputs, _run
    cid = case_id(case)
    if cid in _POISONED:
        return _POISONED[cid]
    lin = build_layer(case["recipe"], DEV)
    M, K = case["M"], lin.in_features
    assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
    x_clean = torch.from_numpy(O.gen_x(M, K, seed=M).astype(np.float32)).to(NF.x_dtype(lin)).to(DEV)
    own_quantiser = not NF.is_direct(lin, case["fused"]) and not case["fused"]  # the library's quantiser runs as a launch of its own

    def one(x16):
        xk, sx = _quantised_inputs(lin, x16, case["fused"])
        res = _run(lin, case, xk, sx, None)
        assert res is not None
        y, name, need = res
        assert name == case["name"], name
        return dict(yt=y.cpu(), ybits=_bits(y), name=name, need=need,
                    xq=_bits(xk) if own_quantiser else None, sx=_bits(sx) if own_quantiser else None,
                    sx_val=sx.float().cpu().numpy() if own_quantiser and sx.dtype == torch.float32 else None)

    clean = one(x_clean)
    del clean["yt"]
    out = dict(clean=clean, runs=[], own_quantiser=own_quantiser, sk=scales_x_kind(lin), group=lin.group_size, M=M)
    for li, (r, kind) in enumerate(NF.launches(M)):
        xp, ks = NF.poison(x_clean, r, kind, NF.quant_group(lin), seed=1000 * M + li)
        run = one(xp)
        run.update(r=r, kind=kind, ks=ks, launch=li, yrow=run.pop("yt")[r].float().numpy().astype(np.float64))
        assert (run["name"], run["need"]) == (out["clean"]["name"], out["clean"]["need"])  # same kernel, same plan
        out["runs"].append(run)
    _POISONED[cid] = out
    return out


@pytest.mark.parametrize("case", [c for c in CASES if c["M"] >= 2], ids=case_id)
def test_a_poisoned_row_leaves_every_other_row_bit_identical(case):
    L = _poisoned_launches(case)
    clean, bad = L["clean"], []
    for run in L["runs"]:
        changed = dict(y=NF.isolation_gate(run["ybits"], clean["ybits"], run["r"]))
        if L["own_quantiser"]:
            changed["xq"] = NF.isolation_gate(run["xq"], clean["xq"], run["r"])
            sx, sx0 = run["sx"], clean["sx"]
            if sx.ndim == 1:  # per-token scales [M]
                sx, sx0 = sx.reshape(-1, 1), sx0.reshape(-1, 1)
            changed["scales_x"] = NF.isolation_gate(sx, sx0, run["r"])  # (block scales: the padded rows M .. M_pad - 1 included)
        rec = dict(tag="isolate/" + case_id(case), kernel=run["name"], launch=run["launch"], row=run["r"], kind=run["kind"],
                   ks=[k for k, _ in run["ks"]], changed={k: v[:8] for k, v in changed.items()}, ok=not any(changed.values()))
        REPORT.append(rec)
        if not rec["ok"]:
            bad.append(rec)
    assert not bad, f"{case['name']}: rows other than the poisoned one changed\n" + "\n".join(
        f"  launch {b['launch']}: row {b['row']} {b['kind']} at k {b['ks']} -> changed rows {b['changed']}" for b in bad)


def _visibility(case):
    """records of the visibility gate over the poisoned launches of `case`"""
    L = _poisoned_launches(case)
    recs = []
    for run in L["runs"]:
        r = run["r"]
        rec = dict(tag="visible/" + case_id(case), kernel=run["name"], launch=run["launch"], row=r, kind=run["kind"],
                   ks=[k for k, _ in run["ks"]], finite_outputs=NF.visible_gate(run["yrow"]), n=int(run["yrow"].size))
        rec["ok"] = rec["finite_outputs"] == 0
        if L["own_quantiser"] and L["sk"] == "token":
            rec["scale_x"] = float(run["sx_val"].reshape(-1)[r])
            rec["ok"] = rec["ok"] and not np.isfinite(rec["scale_x"])
        elif L["own_quantiser"] and L["sk"] == "block":
            g = L["group"]
            blocks = sorted({k // g for k, _ in run["ks"]})
            code = NF.E4M3_NAN if g == 16 else NF.E8M0_NAN
            rec["scale_bytes"] = [int(run["sx"][r, b]) for b in blocks]
            rec["ok"] = rec["ok"] and NF.block_scale_gate(run["sx"][r], blocks, code)
        recs.append(rec)
    return recs


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_poisoned_row_comes_back_non_finite_in_every_element(case):
    recs = _visibility(case)
    REPORT.extend(recs)
    bad = [r for r in recs if not r["ok"]]
    assert not bad, f"{case['name']}: a non-finite activation came back finite\n" + "\n".join(
        f"  launch {b['launch']}: row {b['row']} {b['kind']} at k {b['ks']}: {b['finite_outputs']} of {b['n']} outputs finite"
        f" (scale_x {b.get('scale_x')}, scale bytes {b.get('scale_bytes')})" for b in bad)


def _pairs():
    """(fused case, two-launch case) of one layer and M"""
    key = lambda c: (tuple(sorted((k, str(v)) for k, v in c["recipe"].items())), c["M"])  # noqa: E731
    two = {}
    for c in CASES:
        if not c["fused"] and not NF.case_is_direct(c):
            two.setdefault(key(c), []).append(c)
    return [(f, t) for f in CASES if f["fused"] for t in two.get(key(f), [])]


@pytest.mark.parametrize("fused,two", _pairs(), ids=lambda c: c["name"])
def test_fused_and_two_launch_forms_agree_on_the_poisoned_rows(fused, two):
    """same layer, same M, same poison (the launches are seeded by M): wherever one form's poisoned row is non-finite the other's is"""
    A, B = _poisoned_launches(fused), _poisoned_launches(two)
    for ra, rb in zip(A["runs"], B["runs"]):
        assert (ra["r"], ra["kind"], ra["ks"][0][0]) == (rb["r"], rb["kind"], rb["ks"][0][0])
        fa, fb = np.isfinite(ra["yrow"]), np.isfinite(rb["yrow"])
        assert not fa.any() and not fb.any(), (fused["name"], two["name"], ra["kind"], int(fa.sum()), int(fb.sum()))


def test_the_pairs_cover_the_fused_one_row_layers():
    names = {f["name"].split("<")[0] for f, _ in _pairs()}
    assert {"a8w8_decode_fused_quant_kernel", "gemv_a8w4_fused_quant_kernel", "gemv_a8w2_fused_quant_kernel", "kmajor_fused_quant_kernel",
            "a8w8_rows_fq_kernel"} <= names


# ------------------------------------------------------------------------------------------------ part 4: fp16 output overflow
@pytest.mark.parametrize("case", [c for c in NF.OVERFLOW_CASES if "overflow/" + case_id(c) not in NF.SKIP], ids=case_id)
def test_fp16_outputs_overflow_to_inf_and_stay_finite_below(case):
    from tests.test_abi_bounds_gpu import _oracle, _quantised_inputs, _run
    lin = NF.overflow_layer(case["recipe"], DEV)
    assert kernel_name(plan_args(lin, case["M"], case["tuning"], case["fused"])) == case["name"]
    x16 = NF.overflow_x(case, NF.OVERFLOW_A[case_id(case)]).to(DEV)
    tol = MR.tol_of(lin, case["name"], NF.FP16)
    y_ref = np.asarray(_oracle(lin, x16, case["name"])[0], np.float64).reshape(case["M"], -1)
    shares = NF.overflow_shares(y_ref, tol)
    assert NF.shares_ok(shares), [s for s in shares if not NF.shares_ok([s])][:4]  # the oracle first: the rows straddle the threshold
    xk, sx = _quantised_inputs(lin, x16, case["fused"])
    res = _run(lin, case, xk, sx, None)
    assert res is not None
    y, name, _ = res
    assert name == case["name"] and y.dtype == torch.float16
    bad = []
    for rec in NF.overflow_gate(y.float().cpu().numpy(), y_ref, tol):
        rec.update(tag="overflow/" + case_id(case), kernel=name)
        REPORT.append(rec)
        if not rec["ok"]:
            bad.append(rec)
    assert not bad, f"{name}: {len(bad)} rows fail the overflow gate\n" + "\n".join(
        f"  row {b['row']}: {b['over_not_inf']} of {b['over']} over elements not +-Inf of the oracle's sign, "
        f"{b['under_wrong']} of {b['under']} under elements wrong or not finite" for b in bad[:12])


# ------------------------------------------------------------------------------------------------ part 5: bf16 exponent range
@pytest.mark.parametrize("case", NF.WIDE_CASES, ids=case_id)
def test_bf16_rows_of_amplitude_2_to_the_40_and_minus_40_share_a_tile(case):
    from tests.test_abi_bounds_gpu import _oracle, _quantised_inputs, _run
    lin = build_layer(case["recipe"], DEV)
    M, K = case["M"], lin.in_features
    assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
    assert NF.x_dtype(lin) == torch.bfloat16
    out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[torch.bfloat16].value
    bad = []
    for li, rows in enumerate(MR.launch_rows(M, NF.wide_profiles_for(case))):
        x16 = NF.make_wide_x(rows, K, M + li).to(DEV)
        xk, sx = _quantised_inputs(lin, x16, case["fused"])
        res = _run(lin, case, xk, sx, None)
        assert res is not None
        y, name, _ = res
        assert name == case["name"], name
        y_ref = np.asarray(_oracle(lin, x16, name)[0], np.float64).reshape(M, -1)
        assert np.isfinite(y_ref).all() and float(np.abs(y_ref).max()) < NF.WIDE_Y_LIMIT
        for rec in MR.row_gate(y.float().cpu().numpy(), y_ref, out_code, MR.tol_of(lin, name, out_code)):
            rec.update(tag="wide/" + case_id(case), kernel=name, launch=li, profile=rows[rec["row"]])
            REPORT.append(rec)
            if not rec["ok"]:
                bad.append(rec)
    assert not bad, f"{case['name']}: {len(bad)} rows fail the row gate\n{MR._fmt(bad)}"
