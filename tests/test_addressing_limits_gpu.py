"""Both sides of every addressing edge, launched (run on a real MI355X via `pytest -m gpu`).

tests/golden/addressing_edges.json holds, per (entry of tests/test_abi_bounds_cpu.py::CASES, stride), the largest stride at which the
planner still names the case's kernel and its answer 64 elements later (tests/test_addressing_limits_cpu.py pins them without a launch).
Here each of those rows calls gemlite_hip_forward at two points:
  edge   the largest admitted stride (for "unbounded" the stride where the sweep stopped: the far rows lie beyond base + 4 GiB).  The
         kernel is the case's; the output window is bit-identical to the dense call of the case (same plan, only the addresses moved)
         and passes the gates of test_gpu_parity and the row gate of test_magnitude_range_gpu against the float64 oracle.
  past   the first declined stride.  The kernel is the golden file's successor, and its result passes the same two gates.  int8 x int8
         (unpacked A8W8) is bit-identical to the dense call as well: every kernel of that family sums the products exactly in int32 and
         scales the sum in the shared epilogue, as the int8 comparisons of test_gpu_parity already ask between its kernels.  Where the
         golden answer is GEMLITE_ERR_NO_FUSED_QUANT the call returns that status and leaves `out` as it was.

Layout rules (_place): they keep a wrong offset a wrong number rather than a fault.
  * The operand under test is a view into one allocation filled with 0xFF bytes (NaN in fp16 / bf16 / fp32).
  * The view's base sits 2 GiB into the allocation, and the allocation extends max(addressed extent, 4 GiB) + 64 MiB beyond the base: a
    32-bit offset that wraps, or is taken as signed, still lands in mapped memory of the same tensor.
  * Only the rows the view addresses are written with data; everything between them keeps 0xFF.
  * After the call the view must still equal its source; it is then filled with 0xFF again and the whole allocation is checked for 0xFF
    in one device-side reduction.  For stride_om that is the store check (nothing outside the window written), for an input it is the
    check that no input byte changed.
  * Every other operand is the dense tensor of the case inside a small guarded allocation, compared byte for byte after the call.
  * One stride is moved per launch (scales and zeros share stride_meta_g: both move).  No single allocation exceeds 12 GiB (asserted),
    and it is freed before the next launch.

The four activation quantisers and pack_over_cols have no planner in front of them; they run at 3 and 33 rows with a row stride that puts
the last row just below 2^31, just above 2^31 and just above 2^32 bytes, bit-exact against the oracle."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, _hip
from oracle import gemlite_oracle as O
from oracle import mx_oracle as MX
from tests import test_abi_bounds_gpu as A
from tests.test_abi_bounds_cpu import CASES, build_layer, case_id, kernel_name, plan_args
from tests.test_addressing_limits_cpu import GOLDEN, NO_FUSED_QUANT, STEP, cap_steps, extent, fields
from tests.test_gpu_parity import _compare
from tests.test_gpu_parity import _report  # noqa: F401  (autouse here too: writes the report, these rows included, when the module ends)
from tests.test_magnitude_range_gpu import row_gate, tol_of

pytestmark = pytest.mark.gpu
DEV = A.DEV
GIB = 1 << 30
BASE = 2 * GIB  # bytes in front of a moved view
REACH = 4 * GIB  # what any 32-bit offset can reach behind the base
TAIL = 64 << 20
MAX_ALLOC = 12 * GIB
INTS = {1: torch.uint8, 2: torch.int16, 4: torch.int32}
ROWS = json.load(open(GOLDEN))["rows"]
CASE_BY_ID = {case_id(c): c for c in CASES}


def _ints(t):
    """the bits of t as integers of its own width (a view: any strides)"""
    return t.view(INTS[t.element_size()])


def _place(t, dim, stride):
    """(view of t's values whose dimension `dim` steps by `stride` elements and the other by 1, the allocation) under the layout
    rules of the module docstring"""
    es = t.element_size()
    ext = ((t.shape[dim] - 1) * stride + t.shape[1 - dim]) * es
    nbytes = (BASE + max(ext, REACH) + TAIL + 7) // 8 * 8
    assert nbytes <= MAX_ALLOC, (nbytes, tuple(t.shape), dim, stride)
    buf = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    strides = [1, 1]
    strides[dim] = stride
    v = buf.view(t.dtype).as_strided(tuple(t.shape), tuple(strides), BASE // es)
    _ints(v).copy_(_ints(t))
    return v, buf


def _all_ff(buf):
    return bool((buf.view(torch.int64) == -1).all())


def _check_and_clear(v, buf, src, what):
    """the view still holds src; with it cleared, the whole allocation is 0xFF again"""
    assert torch.equal(_ints(v), _ints(src)), f"{what}: the rows of the view changed"
    _ints(v).fill_(0xFF if v.element_size() == 1 else -1)
    assert _all_ff(buf), f"{what}: bytes outside the view changed"


# ------------------------------------------------------------------------------------------------ per case: layer, inputs, dense twin
class _State:
    pass


_STATES = {}


def _state(case):
    key = case_id(case)
    if key not in _STATES:
        st = _State()
        st.lin = lin = build_layer(case["recipe"], DEV)
        M, K = case["M"], lin.in_features
        assert kernel_name(plan_args(lin, M, case["tuning"], case["fused"])) == case["name"]
        tdt = torch.bfloat16 if lin.output_dtype in (DType.BF16, DType.MXBF16) else torch.float16
        st.out_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
        st.x16 = torch.from_numpy(O.gen_x(M, K, seed=M).astype(np.float32)).to(tdt).to(DEV)
        st.xk, st.sx = A._quantised_inputs(lin, st.x16, case["fused"])
        y, name, _ = A._run(lin, case, st.xk, st.sx, None)
        assert name == case["name"], name
        st.dense = y
        st.oracles = {}  # by weight rounding (A._oracle): computed once, shared by every stride of the case
        _STATES[key] = st
    return _STATES[key]


def _moved(case, st, field):
    """{operand name: dimension that takes the stride} for the operands `field` moves"""
    lin = st.lin
    if field == "stride_xm":
        return {"x": 0}
    if field == "stride_om":
        return {"out": 0}
    if field == "stride_sx_m":
        return {"sx": 0}
    if field in ("stride_wk", "stride_wn"):
        return {"w": 0 if field == "stride_wk" else 1}
    assert field in ("stride_meta_g", "stride_meta_n"), f"{field}: a stride _moved() does not know; name the operand it steps"
    # [groups, N] with rows stride_meta_g (the block-scaled layers hold the [N, groups] transpose, core._build_template): stride_meta_g
    # moves the dimension whose stride is not 1, stride_meta_n (swept only where it is not 1) the other one
    meta = [(k, t) for k, t in (("s", lin.scales.data), ("z", lin.zeros.data)) if t.dim() == 2 and min(t.shape) > 1]
    if field == "stride_meta_n":
        mv = {k: (1 if t.shape[1] == lin.out_features else 0) for k, t in meta}
    else:
        mv = {k: (0 if t.stride(1) == 1 else 1) for k, t in meta}
    assert mv, "no two-dimensional metadata"
    return mv


def _launch(case, st, field, stride):
    """One gemlite_hip_forward of `case` with `field` = stride; returns (window, kernel name), or None where the library answers
    GEMLITE_ERR_NO_FUSED_QUANT (and `out` is untouched)."""
    lin, M, N, fused = st.lin, case["M"], st.lin.out_features, case["fused"]
    lib = A._lib()
    mv = _moved(case, st, field)
    src = dict(x=st.xk, w=lin.W_q.data, s=lin.scales.data, z=lin.zeros.data, sx=st.sx)
    big, small, views = [], [], {}
    torch.cuda.empty_cache()  # the allocation of the launch before this one
    try:
        for k, t in src.items():
            if t is None:
                views[k] = None
            elif k in mv:
                v, buf = _place(t, mv[k], stride)
                big.append((k, v, buf, t))
                views[k] = v
            else:
                v, buf = A._place(t, None)
                if buf is not None:
                    small.append((k, buf))
                views[k] = v
        odt = gemlite_amd.dtypes.DTYPE_TO_TORCH[lin.output_dtype.value]
        es = torch.empty((), dtype=odt).element_size()
        if "out" in mv:
            so = stride
            win, obuf = _place(torch.empty((M, N), dtype=odt, device=DEV), 0, stride)
            _ints(win).fill_(-1)  # the window starts as 0xFF too
        else:
            so = N
            obuf = torch.full(((256 + (M + 64) * N * es + 7) // 8 * 8,), 0xFF, dtype=torch.uint8, device=DEV)
            win = obuf.view(odt).as_strided((M, N), (N, 1), 256 // es)
        xv, sxv = views["x"], views["sx"]
        a = plan_args(lin, M, case["tuning"], fused, x=xv.data_ptr(), out=win.data_ptr(), stride_xm=xv.stride(0), stride_om=so,
                      tensors=(views["w"], views["s"], views["z"]))
        if sxv is not None:
            a.scales_x = sxv.data_ptr()
            a.stride_sx_m = sxv.stride(0) if sxv.dim() == 2 else 1
        assert getattr(a, field) == stride, (field, getattr(a, field), stride)
        need = int(lib.gemlite_hip_workspace_bytes(C.byref(a)))
        ws = torch.full((need + A.WS_GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
        ws[:need].zero_()
        a.workspace, a.workspace_bytes = ws.data_ptr(), need
        before = [A._bytes(b) for _, b in small]
        rc = lib.gemlite_hip_forward(C.byref(a), A._stream())
        torch.cuda.synchronize()
        what = f"{case_id(case)} {field}={stride}"
        if rc == _hip.ERR_NO_FUSED_QUANT:
            assert fused, what
            assert _all_ff(obuf), f"{what}: refused call wrote its output"
            return None
        assert rc == 0, (what, _hip.status_string(rc))
        name = kernel_name(a)
        y = win.clone()
        _ints(win).fill_(-1)
        assert _all_ff(obuf), f"{what} ({name}): store outside the output window"
        assert bool((ws[need:] == 0xFF).all()), f"{what} ({name}): write past the {need} workspace bytes it asked for"
        if need >= A.COUNTER_BYTES:
            assert bool((ws[:A.COUNTER_BYTES] == 0).all()), f"{what} ({name}): arrival counters not left at zero"
        for (k, buf), b0 in zip(small, before):
            assert torch.equal(b0, A._bytes(buf)), f"{what} ({name}): input {k} changed"
        for k, v, buf, t in big:
            _check_and_clear(v, buf, t, f"{what} ({name}): input {k}")
        return y, name
    finally:
        del big, small, views
        win = obuf = ws = a = None
        torch.cuda.empty_cache()


def _gates(case, st, tag, y, name):
    okey = name.startswith("gemv_a8w")
    if okey not in st.oracles:
        y_ref, abs_gate = A._oracle(st.lin, st.x16, name)
        st.oracles[okey] = (np.asarray(y_ref, np.float64).reshape(case["M"], -1), abs_gate)
    y_ref, abs_gate = st.oracles[okey]
    _compare(f"addressing/{case_id(case)}/{tag}", y, y_ref, st.out_code, abs_gate=abs_gate, extra=dict(kernel=name))
    bad = [r for r in row_gate(y.float().cpu().numpy(), y_ref, st.out_code, tol_of(st.lin, name, st.out_code)) if not r["ok"]]
    assert not bad, (tag, name, bad[:4])


@pytest.mark.parametrize("row", ROWS, ids=lambda r: f"{r[0]}-{r[1]}")
def test_both_sides_of_every_edge(row):
    cid, field, stride, ext, nxt = row
    case = CASE_BY_ID[cid]
    f = fields(case)[field]
    st = _state(case)
    edge = f[0] + STEP * cap_steps(f) if stride == "unbounded" else stride
    assert extent(f, edge) == ext, (extent(f, edge), ext)
    if stride == "unbounded":
        assert ext > BASE + REACH  # the far rows lie beyond base + 4 GiB
    y, name = _launch(case, st, field, edge)
    assert name == case["name"], name
    assert torch.equal(A._raw(y), A._raw(st.dense)), f"{name}: {field} = {edge} differs from the dense call on the same plan"
    _gates(case, st, f"{field}/edge", y, name)
    if stride == "unbounded":
        return
    res = _launch(case, st, field, edge + STEP)
    if nxt == NO_FUSED_QUANT:
        assert res is None, res[1]
        return
    assert res is not None, f"GEMLITE_ERR_NO_FUSED_QUANT where the planner names {nxt}"
    y, name = res
    assert name == nxt, (name, nxt)
    _gates(case, st, f"{field}/past", y, name)
    if case["recipe"]["kind"] == "a8w8i" and not case["fused"]:
        assert torch.equal(A._raw(y), A._raw(st.dense)), f"{name}: int8 x int8 differs from {case['name']} on the dense call"


# ------------------------------------------------------------------------------------------------ writers without a planner
SPANS = {"below_2^31": (1 << 31) - (1 << 20), "above_2^31": (1 << 31) + (1 << 20), "above_2^32": (1 << 32) + (1 << 20)}


def _stride_for(span, rows, es):
    """row stride in elements, a multiple of 64, with (rows - 1) * stride * es the first such value at or above `span` bytes"""
    per = (rows - 1) * es * 64
    return (span + per - 1) // per * 64


@pytest.mark.parametrize("span", SPANS, ids=list(SPANS))
@pytest.mark.parametrize("M", [3, 33])
@pytest.mark.parametrize("kind", ["int8", "mxfp8", "mxfp4", "nvfp4"])
def test_activation_quantisers_read_rows_past_2_and_4_gib(kind, M, span):
    lib = A._lib()
    K = 512
    tdt = torch.float16
    stride = _stride_for(SPANS[span], M, 2)
    assert SPANS[span] <= (M - 1) * stride * 2 < SPANS[span] + (1 << 20)
    src = torch.randn(M, K, generator=torch.Generator().manual_seed(M), dtype=torch.float32).to(tdt).to(DEV)
    x, xbuf = _place(src, 0, stride)
    in_code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    try:
        if kind == "int8":
            y = torch.empty((M, K), dtype=torch.int8, device=DEV)
            s = torch.empty((M,), dtype=torch.float32, device=DEV)
            rc = lib.gemlite_hip_scale_activations_per_token(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(s.data_ptr()),
                                                             M, K, stride, in_code, gemlite_amd.dtypes.TORCH_TO_DTYPE[torch.int8].value,
                                                             C.c_void_p(A._stream()))
            torch.cuda.synchronize()
            assert rc == 0, _hip.status_string(rc)
            y_o, s_o = O.scale_activations_per_token(src.cpu(), O.INT8)
            assert np.array_equal(y.float().cpu().numpy().astype(np.float64), y_o)
            assert np.array_equal(s.cpu().numpy(), s_o.reshape(-1))
        else:
            g = 16 if kind == "nvfp4" else 32
            mp = (M + g - 1) // g * g if kind == "nvfp4" else (M + 31) // 32 * 32
            yk = K if kind == "mxfp8" else K // 2
            y = torch.empty((M, yk), dtype=torch.uint8, device=DEV)
            s = torch.empty((mp, K // g), dtype=torch.uint8, device=DEV)
            fn = getattr(lib, "gemlite_hip_scale_activations_" + kind)
            rc = fn(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), C.c_void_p(s.data_ptr()), M, K, stride, in_code, C.c_void_p(A._stream()))
            torch.cuda.synchronize()
            assert rc == 0, _hip.status_string(rc)
            y_o, s_o = getattr(MX, "scale_activations_" + kind)(src.float().cpu().numpy())
            assert np.array_equal(y.cpu().numpy(), y_o)
            assert np.array_equal(s.cpu().numpy(), s_o)
        _check_and_clear(x, xbuf, src, f"{kind} x")
    finally:
        x = xbuf = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("span", SPANS, ids=list(SPANS))
@pytest.mark.parametrize("N", [3, 33])
@pytest.mark.parametrize("nbits,pb", [(4, 32), (4, 8)])
def test_pack_over_cols_reads_rows_past_2_and_4_gib(nbits, pb, N, span):
    """rows of W_q at ld_in (the tiled 32-bit packer and the plain one); the packed words are the oracle's"""
    lib = A._lib()
    K = 512
    e = pb // nbits
    ld = _stride_for(SPANS[span], N, 1)
    src = torch.randint(0, 2 ** nbits, (N, K), generator=torch.Generator().manual_seed(N), dtype=torch.uint8).to(DEV)
    W, wbuf = _place(src, 0, ld)
    try:
        pdt = {8: torch.uint8, 32: torch.int32}[pb]
        packed = torch.empty((K // e, N), dtype=pdt, device=DEV)
        rc = lib.gemlite_hip_pack_over_cols(C.c_void_p(W.data_ptr()), C.c_void_p(packed.data_ptr()), N, K, ld, nbits, pb, C.c_void_p(A._stream()))
        torch.cuda.synchronize()
        assert rc == 0, _hip.status_string(rc)
        ref = O.pack_over_cols(src.cpu().numpy(), nbits, pb).view({8: np.uint8, 32: np.uint32}[pb]).astype(np.uint64)
        got = packed.cpu().numpy().view({8: np.uint8, 32: np.uint32}[pb]).astype(np.uint64)
        assert np.array_equal(got, ref)
        _check_and_clear(W, wbuf, src, "pack_over_cols w_q")
    finally:
        W = wbuf = None
        torch.cuda.empty_cache()
