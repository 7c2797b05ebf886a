"""The inventory of kernel forms (tests/kernel_forms.py, tests/golden/kernel_forms.json) on the CPU — the planner plans without a device:

  * every frozen request still plans to its frozen form and workspace size;
  * the recipes of the sweep describe the layers the GPU test builds: the same request on a layer packed through the public path (CPU tensors) has the same
    fields and the same plan;
  * completeness: every kernel label in csrc and every form the sweep reaches has a frozen row or stands in EXEMPT with a reason that is checked;
  * the rows are small;
  * the comparison the GPU test makes accepts the oracle's result and rejects four kinds of subtly wrong ones at the frozen shapes.
Regenerate the inventory after an intended planner change: `python tests/kernel_forms.py --write`."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from tests import kernel_forms as KF  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = KF.load_rows()

# A label that no frozen row plans to.  Two kinds of reason only:
#   ("entry", <entry point or kernel label>, <tests/file that pins it>, <why>)   not a forward plan: launched through that entry point, pinned by that file
#   ("unreachable", <file:line>, <text of that line>, <why>)                      no request reaches it; the sweep must indeed never return it, and the
#                                                                                 named line must still hold the quoted text
# Every forward form is reachable in the shipped build or compiled out of it, and the launches that are no forward plan (grouped decode, experts,
# quantise / dequantise, activation quantisers, pack / unpack) label their kernels in other words than `..._kernel`, so only the second kind occurs today.
EXEMPT = {
    "gemm_a8w8_sq_kernel": ("unreachable", "gemm_a8w8.hip:619", '("gemm_a8w8_sq_kernel")',
                            "the family's name quoted in a comment; the planner's labels are gemm_a8w8_sq_kernel<64x64> / <128x128>"),
    "gemm_mx_sq_kernel": ("unreachable", "gemm_mx.hip:1408", '("gemm_mx_sq_kernel")',
                          "the family's name quoted in a comment; the planner's labels are gemm_mx_a?w?_sq_kernel<64x64>"),
    "gemm_w4_tiled_kernel<legacy>": ("unreachable", "gemm_wn_tiled.hip:628", "if (a.tuning[2] == 4 || a.tuning[2] == 8) return false;",
                                     "tuning[2] = 4 is refused unless the library is built with GL_AB_KERNELS (make AB=1)"),
    "gemm_w4_tiled_kernel<256x128>": ("unreachable", "gemm_wn_tiled.hip:628", "if (a.tuning[2] == 4 || a.tuning[2] == 8) return false;",
                                      "tuning[2] = 8 is refused unless the library is built with GL_AB_KERNELS (make AB=1)"),
    "gemm_wn_direct_kernel<tile16,8w>": ("unreachable", "gemm_wn_direct.hip:304", "if constexpr (V >= 2 && MT == 1)",
                                         "dpick_spg has an 8-wave instantiation only for V >= 2: 16-column tiles always run 4 waves"),
}
# The labels pw_label can compose (`<...,b8>` / `<...,b16>`, KF.pack_width_names()) are no literals: one rule per group that no request with 8- / 16-bit
# words reaches — (pattern, reason); every composable label without a frozen row matches a rule, and no swept label does.
EXEMPT_PACK_WIDTH = (
    (r"gemm_(a16w[48]_mxfp|a16w8|nvfp4_f16)_kernel<", ("unreachable", "gemm_wn_mma.hip:197", "lp.name = nv ? nv_names[",
     "plan_gemm_wn_mma_mx (K-contiguous bytes, never packed words) labels its plans itself and shares the file with the callers of pw_label")),
    (r"gemm_a8w[24]_mma_kernel<", ("unreachable", "gemm_wn_mma.hip:227", "a.input_dtype != GEMLITE_DT_FP16 && a.input_dtype != GEMLITE_DT_BF16",
     "8- / 16-bit words are taken under 16-bit activations only")),
    (r"gemm_w8_mma_kernel<[^>]*,b8>", ("unreachable", "gemm_wn_mma.hip:227", "(nbits == 8 && pb != 16)", "8-bit codes in 8-bit words are not packed words")),
    (r"gemm_w\d_mma_kernel<32x128,g32,", ("unreachable", "gemm_wn_mma.hip:255", "if (pw) return false;", "the group-32 tiles have no 8- / 16-bit word form")),
    (r"gemm_w[24]_mma_kernel<128x64,", ("unreachable", "gemm_wn_mma.hip:337", "(pw && v != 0)", "of the narrow tiles only variant 0 (64 x 64) takes 8- / 16-bit words")),
    (r"gemv_wn_kernel<tile16[,>]", ("unreachable", "gemv_wn.hip:846", "if (pw && cq < 3) return false;", "8- / 16-bit words run on 32- and 64-column tiles only")),
    (r"gemv_wn_kernel<tile(32|64),xdirect", ("unreachable", "gemv_wn.hip:897", "bool xd = !pw &&", "no direct-x form for 8- / 16-bit words")),
    (r"gemv_w4_decode3?_kernel<", ("unreachable", "gemv_wn.hip:944", "if (xd && cq == 2 &&", "the decode kernels take the direct-x shapes, which 8- / 16-bit words never are (gemv_wn.hip:897)")),
)


def _check_reason(name, reason):
    assert reason[0] in ("entry", "unreachable") and len(reason) == 4, name
    if reason[0] == "entry":   # the named test file exists and speaks of the kernel or the entry point
        path = os.path.join(ROOT, reason[2])
        assert os.path.isfile(path), (name, reason[2])
        text = open(path).read()
        assert name.split("<")[0] in text or reason[1] in text, (name, reason)
    else:                      # the named line of a file of csrc still holds the quoted text
        m = re.fullmatch(r"([a-z0-9_]+\.(?:hip|h|inc)):(\d+)", reason[1])
        assert m, (name, reason[1])
        with open(os.path.join(KF.CSRC, m.group(1))) as f:
            lines = f.readlines()
        assert int(m.group(2)) <= len(lines) and reason[2] in lines[int(m.group(2)) - 1], (name, reason[1], "the line no longer reads: " + reason[2])


def test_frozen_rows_still_plan():
    lib = KF.load_lib()
    assert len(ROWS) >= 400
    moved = []
    for r in ROWS:
        got = KF.plan(lib, KF.row_args(r))
        if got != (r["name"], r["workspace_bytes"]):
            moved.append((KF.row_id(r), got))
    assert not moved, (len(moved), moved[:8])
    for r in ROWS:   # what the selection promises
        assert (r["role"] == "split") <= (r["workspace_bytes"] > 0), KF.row_id(r)
    # the tile forms that take K slices have a launch through the slab / combine path: workspace bytes alone do not say so for NVFP4 (KF.has_slices)
    sliced = {(r["name"], r["tdt"]) for r in ROWS if KF.has_slices((r["family"], 0, r["M"], r["N"], r["K"], 0, 0, r["name"], r["workspace_bytes"]))}
    for form in ("gemm_nvfp4_f16_kernel<128x128>", "gemm_nvfp4_f16_kernel<32x128>", "gemm_nvfp4_f16_kernel<64x64>", "gemm_w4_mma_kernel<64x128>", "gemm_a8w8_lds_kernel<128x128>"):
        assert (form, "fp16") in sliced and (form, "bf16") in sliced, form


def test_recipes_describe_the_layers_the_gpu_test_builds():
    """The sweep plans on hand-filled requests; the GPU test asks the planner on real tensors.  For every frozen row the request core._call_args builds on
    the layer of build_layer() — CPU tensors here — equals the recipe field by field (pointers: NULL or not), and plans to the frozen form."""
    lib = KF.load_lib()
    pointers = {"x", "w_q", "scales", "zeros", "out", "scales_x"}
    skip = {"workspace", "workspace_bytes"}
    bad = []
    for r in sorted(ROWS, key=lambda r: (r["family"], r["tdt"], r["N"], r["K"], r["M"])):
        case = KF.build_case(r, "cpu")
        real, want = KF.call_args(r, case), KF.row_args(r)
        for f, _ in _hip.ForwardArgs._fields_:
            if f in skip:
                continue
            a, b = getattr(real, f), getattr(want, f)
            if f == "tuning":
                a, b = list(a), list(b)
            if f in pointers:
                a, b = bool(a), bool(b)
            if a != b:
                bad.append((KF.row_id(r), f, a, b))
        got = KF.plan(lib, real)
        if got != (r["name"], r["workspace_bytes"]):
            bad.append((KF.row_id(r), "plan", got))
    assert not bad, (len(bad), bad[:8])


def test_every_kernel_label_is_frozen_or_exempt_with_a_checked_reason():
    frozen = {r["name"] for r in ROWS}
    swept = {c[7] for c in KF.sweep() if c[7].endswith(("_kernel", ">"))}
    literal, composed = KF.source_names(), KF.pack_width_names()
    assert len(literal) >= 150 and "gemm_w4_mma_kernel<64x128>" in literal and "gemv_w4_decode3_kernel<tile16,16w>" in literal
    assert "gemm_w4_mma_kernel<256x256,b8>" in composed and "gemv_wn_kernel<tile64,8w,b16>" in composed
    universe = literal | composed | swept
    assert not (swept - frozen), ("forms the sweep reaches without a frozen row: run python tests/kernel_forms.py --write", sorted(swept - frozen))
    assert not (frozen - swept), ("frozen forms the sweep no longer reaches", sorted(frozen - swept))
    assert not (swept & set(EXEMPT)), ("exempt, yet the sweep reaches it", sorted(swept & set(EXEMPT)))
    assert not [n for n in swept if n.endswith((",b8>", ",b16>")) and n not in composed], "a pack-width label that pack_width_names() does not compose"
    rules = [(re.compile(pat), reason) for pat, reason in EXEMPT_PACK_WIDTH]

    def rule_of(name):
        return [reason for rx, reason in rules if name in composed and rx.match(name)]

    assert not [n for n in swept if rule_of(n)], ("exempt by a pack-width rule, yet the sweep reaches it", sorted(n for n in swept if rule_of(n)))
    lost = sorted(n for n in universe - frozen - set(EXEMPT) if not rule_of(n))
    assert not lost, ("neither frozen nor exempt: extend the sweep of tests/kernel_forms.py, or show why no request reaches it", lost)
    assert not (set(EXEMPT) - universe), ("exempt labels that no longer exist", sorted(set(EXEMPT) - universe))
    for name, reason in EXEMPT.items():
        _check_reason(name, reason)
    for rx, reason in rules:
        assert any(rx.match(n) for n in composed - frozen), ("a pack-width rule that exempts nothing", rx.pattern)
        _check_reason(rx.pattern, reason)


def test_rows_are_small():
    small = [r for r in ROWS if r["N"] * r["K"] <= KF.SMALL_NK]
    assert len(small) * 10 >= len(ROWS) * 9, (len(small), len(ROWS))
    for r in ROWS:
        assert r["N"] * r["K"] <= 4096 * 4096, KF.row_id(r)
        assert r["N"] * r["K"] <= KF.SMALL_NK or r.get("why"), KF.row_id(r)
        assert r["M"] in KF.MS and r["M"] * r["N"] <= 513 * 8192


def _distinct_problems():
    """(family, type, shape, M): what the comparison depends on — and, for fp8 activations over packed words, whether the form is the one-row GEMV"""
    seen = {}
    for r in ROWS:
        key = (r["family"], r["tdt"], r["N"], r["K"], r["M"], r["name"].startswith("gemv_a8w"))
        seen.setdefault(key, r)
    return list(seen.values())


def test_the_comparison_accepts_the_oracle_and_rejects_wrong_results():
    """The checker of the GPU test (KF.check: `_compare` of test_gpu_parity, `_check` of test_mx_gpu, bit for bit for int8 x int8) on the float64 oracle's
    own result and on four wrong copies of it, with the data of the GPU test at every frozen shape.  A wrong copy that passes means the data cannot tell a
    kernel that makes this mistake from a correct one: the fix is the data (make_x, build_layer), never the gate."""
    passed_wrong, rejected_clean, n = [], [], 0
    for r in sorted(_distinct_problems(), key=lambda r: (r["family"], r["tdt"], r["N"], r["K"], r["M"])):
        case = KF.build_case(r, "cpu")
        fam, tdt = case["fam"], case["tdt"]
        parts = KF.oracle_parts(fam, case["lin"], case["xq"], case["sx"], r["name"])
        ref, ys = KF.wrong_results(fam, tdt, parts)
        assert torch.isfinite(ys["clean"]).all() and float(abs(ref).mean()) > 1e-3, KF.row_id(r)
        for what, y in ys.items():
            try:
                KF.check(fam, tdt, KF.row_id(r), y, ref, parts)
                ok = True
            except AssertionError:
                ok = False
            if what == "clean" and not ok:
                rejected_clean.append(KF.row_id(r))
            if what != "clean" and ok:
                passed_wrong.append((KF.row_id(r), what))
        n += 1
    assert n >= 100
    assert not rejected_clean, (len(rejected_clean), rejected_clean[:8])
    assert not passed_wrong, (len(passed_wrong), passed_wrong[:8])


def test_the_oracle_in_parts_is_the_family_tests_oracle():
    """oracle_parts() composes the oracle's own functions; on one row per family its result equals `_oracle_from_layer` (test_gpu_parity) / `_oracle`
    (test_mx_gpu) on CPU tensors, to float64 rounding.  (fp8 activations over packed words: those helpers do not round the weights to e4m3; the family's
    own test calls forward_packed with weight_cast_code, as oracle_parts does.)"""
    import numpy as np
    from tests.test_gpu_parity import _oracle_from_layer
    seen = set()
    for r in ROWS:
        F = KF.FAMILIES[r["family"]]
        if r["family"] in seen or F.kind == "mx" or (F.kind == "a8wn" and F.params["act"] == KF.FP8E4) or r["M"] > 64:
            continue
        seen.add(r["family"])
        case = KF.build_case(r, "cpu")
        ref = KF.oracle_out(KF.oracle_parts(r["family"], case["lin"], case["xq"], case["sx"], r["name"]))
        sx = None if case["sx"] is None else case["sx"].numpy()
        want = _oracle_from_layer(case["lin"], case["xq"], sx)
        assert np.allclose(ref, want, rtol=1e-12, atol=1e-12 * float(np.abs(want).max())), r["family"]
    assert len(seen) >= 15
