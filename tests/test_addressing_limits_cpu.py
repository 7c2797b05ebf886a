"""Addressing limits of every planner (no GPU, nothing is launched).

Most kernels address an operand with a 32-bit byte offset from a uniform base (buffer descriptors, `global_load saddr + voffset`); a
hand-written gate in each planner keeps a request whose strides carry an operand past that reach away from the kernel.  For every entry
of tests/test_abi_bounds_cpu.py::CASES and every stride of the request that addresses more than one row, edge() raises that one stride on
the lattice s0 + 64 j (which keeps every 16-byte alignment condition) and bisects for the last stride at which the planner still names the
case's kernel, up to an addressed extent of 2^33 + 2^26 bytes.  The edges are frozen in tests/golden/addressing_edges.json (stride, addressed
bytes and the answer one step later), every finite edge must lie below 2^32 addressed bytes, and an operand that is never declined must be
listed, with its source line, in ADDRESSES_64BIT.  Nothing here launches a kernel: tests/test_addressing_limits_gpu.py runs both sides of every edge.

The addressed extent of a stride is ((rows - 1) * stride + last row) * element size, with the rows the request names: M for x and out, M
rounded up to the scale block rows (32; NVFP4 16) for the activation block scales, K / elements_per_sample or N for w_q, K / group or N
for the metadata.  A kernel that reads padded rows of x addresses more than that, so the bound is a necessary one.

Regenerate after an intended change: `python tests/test_addressing_limits_cpu.py --write`."""
import ctypes as C
import functools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import DType, _hip  # noqa: E402
from tests.test_abi_bounds_cpu import CASES, case_id, cpu_layer, kernel_name, plan_args, scales_x_kind, x_format  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "addressing_edges.json")
STEP = 64
CAP_BYTES = (1 << 33) + (1 << 26)
NO_FUSED_QUANT = "GEMLITE_ERR_NO_FUSED_QUANT"

# Operands a kernel addresses with 64-bit arithmetic: the only (kernel, stride) pairs that may stay admitted up to CAP_BYTES.
# stride_om: every kernel listed with it stores through the shared Epilogue (gl_common.h:183: int64_t stride_om), whose helpers take
# the row as int64_t and form out + m * stride_om in 64 bits (gl_common.h:199 epilogue_store, :234 store_out_t, :252 store_out4_t,
# :271 / :282 store_out4_any); the comment of an entry names the kernel's call of that helper.
_OM = "stride_om"
ADDRESSES_64BIT = {
    "gemv_mfma_kernel": {_OM},  # gemv_mfma.hip:345 store_out_t
    "gemm_wn_direct_kernel": {"stride_xm", "stride_wk", "stride_meta_g", _OM},  # gemm_wn_direct.hip:116 x, :110 / :127 w, :106 / :141 int64 mstride, :270 / :290 store_out_t
    "gemm_wn_stream_kernel": {"stride_xm", "stride_wk", "stride_meta_g", _OM},  # gemm_wn_stream.hip:144 x, :99 / :104 w, :96 / :109 int64 mstride, :360 / :377 store_out_t
    "gemm_w4_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234 store_out4_t / store_out4_any
    "gemm_w2_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_w1_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_w8_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_a8w4_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:907 / :1070 / :1142 / :1235 store_out4_any
    "gemm_a8w2_mma_kernel": {_OM},  # gemm_wn_mma_kernel.inc:907 / :1070 / :1142 / :1235 store_out4_any
    "gemm_a16w8_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_a16w4_mxfp_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_a16w8_mxfp_kernel": {_OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    # NVFP4 above the rows kernel: nvfp4_expand_f16_kernel writes x as dense fp16 rows for the fp16 tile kernel; it reads x and the block
    # scales at (int64_t)m * stride (gemm_mx.hip:222, :223)
    "gemm_nvfp4_f16_kernel": {"stride_xm", "stride_sx_m", _OM},  # gemm_wn_mma_kernel.inc:906 / :1069 / :1141 / :1234
    "gemm_w4_tiled_kernel": {_OM},  # gemm_wn_tiled.hip:118 / :148 store_out4_t
    "generic_matmul_kernel": {"stride_xm", "stride_wk", "stride_meta_g", _OM},  # generic.hip:33-34 int64 n, m; :50-57 w, :63-65 meta, :71-73 x, :77 epilogue_store
    "kmajor_matmul_kernel": {"stride_wn"},  # generic.hip:97 int64 n, :102 wcol = w + n * stride_wn * esz
    "kmajor_fused_quant_kernel": {"stride_wn"},  # generic.hip:268 int64 n, :270 wcol = w + n * stride_wn
    "kmajor_w8a16_kernel": {"stride_xm", "stride_wn", _OM},  # generic.hip:162-163 int64 n, m0; :165 w, :187 x, :204 epilogue_store
    "a16w8_decode_kernel": {"stride_wn"},  # generic.hip:454 int64 n, :455 wcol = w + n * stride_wn
    "a8w8_decode_kernel": {"stride_wn"},  # generic.hip:318 int64 n, :319 wcol = w + n * stride_wn
    "a8w8_decode_fused_quant_kernel": {"stride_wn"},  # the same kernel: generic.hip:319
    "a16w8_rows_kernel": {_OM},  # gemm_a8w8.hip:1576 epilogue_store
    "a16w8_mxfp_rows_kernel": {_OM},  # gemm_a8w8.hip:1576 epilogue_store
    "a16w4_mxfp_rows_kernel": {_OM},  # gemm_a8w8.hip:1576 epilogue_store
    "a16w8_rows_lds_kernel": {_OM},  # gemm_w8_rows.hip:229 epilogue_store
    "a8w8_rows_lds_kernel": {_OM},  # gemm_w8_rows.hip:229 epilogue_store
    "a8w8_rows_kernel": {_OM},  # gemm_a8w8.hip:1370 epilogue_store
    # the producer blocks read the 16-bit rows at (int64_t)m * cq_stride_xm (gl_coopquant.h:40); the consumers read the dense workspace
    "a8w8_rows_fq_kernel": {"stride_xm", _OM},  # gemm_a8w8.hip:1370 epilogue_store
    "gemm_a8w8_kernel": {_OM},  # gemm_a8w8.hip:190 epilogue_store / :236 store_out4_any
    "gemm_a8w8_lds_kernel": {_OM},  # gemm_a8w8.hip:809 store_out4_any
    "gemm_a8w8_mma_kernel": {_OM},  # gemm_a8w8.hip:236 store_out4_any
    "gemm_a8w8_sq_kernel": {_OM},  # gemm_a8w8.hip:993 store_out4_any
    "gemv_a8w4_kernel": {"stride_wk", "stride_meta_g"},  # gemv_a8wn.hip:87 wq + (int64_t)row * stride_wk, :88 int64 mg
    "gemv_a8w2_kernel": {"stride_wk"},  # gemv_a8wn.hip:87
    "gemv_a8w4_fused_quant_kernel": {"stride_wk", "stride_meta_g"},  # the same kernel: gemv_a8wn.hip:87, :88
    "gemv_a8w2_fused_quant_kernel": {"stride_wk"},  # gemv_a8wn.hip:87
    "a8w4_rows_kernel": {_OM},  # gemv_a8wn.hip:468 epilogue_store
    "a8w2_rows_kernel": {_OM},  # gemv_a8wn.hip:468 epilogue_store
    "mx_gemv_w4_kernel": {"stride_xm", "stride_wn", "stride_meta_g", "stride_sx_m", _OM},  # gemm_mx.hip:255-256 int64 n, m0; :258 w, :271 scales, :314 sx, :329 x, :346 epilogue_store
    "mx_gemv_w8_kernel": {"stride_xm", "stride_wn", "stride_meta_g", _OM},  # gemm_mx.hip:258 w, :271 scales, :316 x, :346 epilogue_store
    "mx_rows_a4w4_kernel": {_OM},  # gemm_mx.hip:592 epilogue_store
    "mx_rows_a8w4_kernel": {_OM},  # gemm_mx.hip:590 store_from_float at (int64_t)m * stride_om
    "mx_rows_a8w8_kernel": {_OM},  # gemm_mx.hip:590 / :592
    "nvfp4_rows_kernel": {_OM},  # gemm_mx.hip:791 epilogue_store
    "gemm_mx_a4w4_kernel": {_OM},  # gemm_mx.hip:1048 store_out4_any
    "gemm_mx_a8w4_kernel": {_OM},  # gemm_mx.hip:1048
    "gemm_mx_a8w8_kernel": {_OM},  # gemm_mx.hip:1048
    "gemm_mx_a4w4_sq_kernel": {_OM},  # gemm_mx.hip:1568 store_out4_any
    "gemm_mx_a8w4_sq_kernel": {_OM},  # gemm_mx.hip:1568
    "gemm_mx_a8w8_sq_kernel": {_OM},  # gemm_mx.hip:1568
    "gemm_mx_a4w4_tile_kernel": {_OM},  # gemm_mx.hip:1350 store_out4_any
    "gemm_mx_a8w4_tile_kernel": {_OM},  # gemm_mx.hip:1350
    "gemm_mx_a8w8_tile_kernel": {_OM},  # gemm_mx.hip:1350
    "mx_generic_kernel": {"stride_xm", "stride_wn", "stride_meta_g", "stride_sx_m", _OM},  # gemm_mx.hip:170-171 int64 n, m; :177 x, :181 scales, :184 sx, :192 / :195 w, :202 epilogue_store
}


def _meta_tensor(lin):
    if lin.scales.numel() > 0 and lin.scales.dim() == 2:
        return lin.scales
    if lin.zeros.dim() == 2 and lin.zeros.numel() > 1:
        return lin.zeros
    return None


def fields(case):
    """The sweepable strides of a case: {field: (s0, rows, last row in elements, element size)} for every stride of the request that
    is not 1 and steps between more than one row."""
    lin = cpu_layer(case["recipe"])
    M, fused = case["M"], case["fused"]
    a = plan_args(lin, M, case["tuning"], fused)
    out = {}
    if M >= 2:
        xdt, xrow, _ = x_format(lin, fused)
        out["stride_xm"] = (xrow, M, xrow, xdt.itemsize)
        out["stride_om"] = (a.N, M, a.N, 2)
    wes = lin.W_q.element_size()
    wrows, wcols = lin.W_q.shape
    if a.stride_wk != 1 and wrows > 1:
        out["stride_wk"] = (a.stride_wk, wrows, wcols, wes)
    if a.stride_wn != 1 and wcols > 1:
        out["stride_wn"] = (a.stride_wn, wcols, wrows, wes)
    meta = _meta_tensor(lin)
    if meta is not None:
        mes = meta.element_size()
        groups = a.K // a.group_size
        if a.stride_meta_g != 1 and groups > 1:
            out["stride_meta_g"] = (a.stride_meta_g, groups, a.N, mes)
        if a.stride_meta_n != 1 and a.N > 1:
            out["stride_meta_n"] = (a.stride_meta_n, a.N, groups, mes)
    if scales_x_kind(lin) == "block" and not fused:
        blk = 16 if lin.input_dtype == DType.NVFP4 else 32
        mp = (M + blk - 1) // blk * blk
        out["stride_sx_m"] = (a.stride_sx_m, mp, a.stride_sx_m, 1)
    return out


def extent(f, s):
    s0, rows, last, es = f
    return ((rows - 1) * s + last) * es


def answer(case, field, s):
    """What the planner says to the case with `field` = s: a kernel name, or GEMLITE_ERR_NO_FUSED_QUANT on a fused request.  Any other
    status, or a workspace of 2^36 bytes or more, fails here: every swept request has an answer."""
    lib = _hip.load()
    a = plan_args(cpu_layer(case["recipe"]), case["M"], case["tuning"], case["fused"])
    setattr(a, field, s)
    rc = lib.gemlite_hip_query(C.byref(a))
    if rc == _hip.ERR_NO_FUSED_QUANT and case["fused"]:
        return NO_FUSED_QUANT
    assert rc == 0, (case_id(case), field, s, _hip.status_string(rc))
    ws = int(lib.gemlite_hip_workspace_bytes(C.byref(a)))
    assert ws < (1 << 36), (case_id(case), field, s, ws)
    name = kernel_name(a)
    assert name.endswith("_kernel") or "_kernel<" in name, (case_id(case), field, s, name)
    return name


def cap_steps(f):
    s0, rows, last, es = f
    return (CAP_BYTES // es - last - (rows - 1) * s0) // ((rows - 1) * STEP)


@functools.lru_cache(maxsize=None)
def _edge(i, field):
    case = CASES[i]
    f = fields(case)[field]
    s0 = f[0]
    assert answer(case, field, s0) == case["name"]
    hi = cap_steps(f)
    if answer(case, field, s0 + STEP * hi) == case["name"]:
        return dict(stride="unbounded", cap_stride=s0 + STEP * hi, extent=extent(f, s0 + STEP * hi), next=None)
    lo = 0  # invariant: named at lo, not named at hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if answer(case, field, s0 + STEP * mid) == case["name"]:
            lo = mid
        else:
            hi = mid
    s = s0 + STEP * lo
    return dict(stride=s, cap_stride=s0 + STEP * cap_steps(f), extent=extent(f, s), next=answer(case, field, s + STEP))


def edge(case, field):
    """{stride: the last lattice stride at which the planner names the case's kernel (or "unbounded": still named at the cap),
    extent: the bytes that stride addresses, next: the planner's answer one step later, cap_stride: where the sweep stops}"""
    return _edge(CASES.index(case), field)


def rows():
    out = []
    for c in CASES:
        for field in fields(c):
            e = edge(c, field)
            out.append([case_id(c), field, e["stride"], e["extent"], e["next"]])
    return out


PAIRS = [(c, field) for c in CASES for field in fields(c)]


def pair_id(p):
    return f"{case_id(p[0])}-{p[1]}"


def test_edges_match_the_golden_file():
    fx = json.load(open(GOLDEN))["rows"]
    got = rows()
    keys, want = [r[:2] for r in got], [r[:2] for r in fx]
    assert keys == want, dict(new=[k for k in keys if k not in want][:8], gone=[k for k in want if k not in keys][:8])
    moved = [(g, w) for g, w in zip(got, fx) if g != w]
    assert not moved, moved[:8]


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_every_finite_edge_addresses_less_than_4_gib(pair):
    e = edge(*pair)
    if e["stride"] != "unbounded":
        assert e["extent"] < (1 << 32), e


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_unbounded_operands_are_the_ones_addressed_with_64_bits(pair):
    case, field = pair
    e = edge(case, field)
    if e["stride"] == "unbounded":
        assert field in ADDRESSES_64BIT.get(case["name"].split("<")[0], ()), \
            f"{case['name']} keeps any {field}: gate it, or list it in ADDRESSES_64BIT with the line that addresses it in 64 bits"


@pytest.mark.parametrize("pair", PAIRS, ids=pair_id)
def test_the_kernel_never_comes_back_past_its_edge(pair):
    case, field = pair
    e = edge(case, field)
    if e["stride"] == "unbounded":
        return
    f = fields(case)[field]
    j0, j1 = (e["stride"] - f[0]) // STEP + 1, (e["cap_stride"] - f[0]) // STEP
    for i in range(32):
        j = int(round(j0 * (j1 / j0) ** (i / 31)))
        assert answer(case, field, f[0] + STEP * j) != case["name"], (field, f[0] + STEP * j)


def test_every_case_and_every_kernel_has_an_edge():
    with_edge = {case_id(c) for c, _ in PAIRS}
    assert with_edge == {case_id(c) for c in CASES}
    assert {c["name"].split("<")[0] for c, _ in PAIRS} == {c["name"].split("<")[0] for c in CASES}


def test_the_64_bit_table_names_kernels_and_fields_of_the_case_table():
    bases = {c["name"].split("<")[0] for c in CASES}
    for k, fs in ADDRESSES_64BIT.items():
        assert k in bases, k
        assert fs <= {f for c, f in PAIRS if c["name"].split("<")[0] == k}, (k, fs)


if __name__ == "__main__" and "--write" in sys.argv:
    rs = rows()
    with open(GOLDEN, "w") as f:
        f.write('{"_note": "per (case of tests/test_abi_bounds_cpu.py::CASES, stride): the largest stride on the lattice s0 + 64 j at which the planner still names the case\'s kernel '
                '(or \\"unbounded\\": still named where the stride addresses 2^33 + 2^26 bytes), the bytes it addresses, and the planner\'s answer 64 elements later; '
                'regenerate with python tests/test_addressing_limits_cpu.py --write", "rows": [\n')
        f.write(",\n".join(" " + json.dumps(r) for r in rs))
        f.write("\n]}\n")
    print(len(rs), "rows")
