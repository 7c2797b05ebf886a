"""gemlite_hip_forward_experts_rows_glu / gemlite_hip_experts_combine and the module methods on top of them (forward_batched_glu,
combine_batched, GemLiteExpertsMLP.forward_batched_fused), the parts that need no GPU: symbols, struct layouts against the header, one
refusal per rule, the block sizes the library resolves, the fakes, and the module on CPU tensors."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from gemlite_amd import DType, ExpertsRouting, GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X
from tests.test_experts_cpu import make_layers, set_
from tests.test_experts_rows_cpu import BAD_ARG, BAD_SHAPE, OK, UNSUPPORTED, WORKSPACE, rows_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, B16, F32, I32, I64 = (DType.FP16.value, DType.BF16.value, DType.FP32.value, DType.INT32.value, DType.INT64.value)
GLU_SYMBOLS = ("gemlite_hip_forward_experts_rows_glu", "gemlite_hip_experts_rows_glu_query", "gemlite_hip_experts_rows_glu_per_block")
COMBINE_SYMBOLS = ("gemlite_hip_experts_combine", "gemlite_hip_experts_combine_query")


def glu_request(R=0, **kw):
    """A valid GLU request on stand-in addresses: tests/test_experts_rows_cpu.py's rows request (N = 768: I = 384), rows I wide."""
    g = _hip.ExpertsRowsGluArgs()
    g.struct_size = C.sizeof(_hip.ExpertsRowsGluArgs)
    g.activation = _hip.ACT_SILU
    g.rows = rows_request(R, **kw)
    g.rows.experts.stride_out_slot = g.rows.experts.layer.N // 2
    return g


def glu_query(g):
    return _hip.load().gemlite_hip_experts_rows_glu_query(C.byref(g))


def glu_rpb(g):
    return _hip.load().gemlite_hip_experts_rows_glu_per_block(C.byref(g))


def combine_request(n_slots=12, spt=3, N=768, dt=F16, ids=I64, w=F32):
    c = _hip.ExpertsCombineArgs()
    c.struct_size = C.sizeof(_hip.ExpertsCombineArgs)
    c.dtype, c.ids_dtype, c.weights_dtype = dt, ids, w
    c.y, c.ids, c.weights, c.out = 0x10000, 0x20000, 0x30000, 0x40000
    c.n_slots, c.n_experts, c.slots_per_token, c.N = n_slots, 8, spt, N
    c.stride_y_slot = c.stride_out_token = N
    return c


def combine_query(c):
    return _hip.load().gemlite_hip_experts_combine_query(C.byref(c))


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in GLU_SYMBOLS + COMBINE_SYMBOLS:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
        want = _hip.ExpertsRowsGluArgs if sym in GLU_SYMBOLS else _hip.ExpertsCombineArgs
        assert getattr(lib, sym).argtypes[0] == C.POINTER(want), sym
    assert lib.gemlite_hip_forward_experts_rows_glu.argtypes[1] == C.c_void_p and lib.gemlite_hip_experts_combine.argtypes[1] == C.c_void_p
    assert lib.gemlite_hip_abi_version() == 1 and _hip.ABI_VERSION == 1
    assert "#define GEMLITE_EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN 64" in header and _hip.EXPERTS_COMBINE_MAX_SLOTS_PER_TOKEN == 64


def test_the_struct_mirrors_have_the_size_and_offsets_of_the_header(tmp_path):
    G, K = _hip.ExpertsRowsGluArgs, _hip.ExpertsCombineArgs
    assert [f[0] for f in G._fields_] == ["struct_size", "activation", "rows", "reserved"] and G._fields_[2][1] is _hip.ExpertsRowsArgs
    assert C.sizeof(G) == 8 + C.sizeof(_hip.ExpertsRowsArgs) + 16
    names = [f[0] for f in K._fields_]
    assert names == ["struct_size", "dtype", "ids_dtype", "weights_dtype", "y", "ids", "weights", "out", "n_slots", "n_experts",
                     "slots_per_token", "N", "stride_y_slot", "stride_out_token", "reserved"]
    assert C.sizeof(K) == 16 + 4 * 8 + 6 * 8 + 16
    if shutil.which("gcc") is None:
        return  # the numbers above stand alone; with a C compiler the header itself is asked
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gemlite_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu", sizeof(gemlite_hip_experts_rows_glu_args), sizeof(gemlite_hip_experts_combine_args));\n'
                   + "".join(f'    printf(" %zu", offsetof(gemlite_hip_experts_rows_glu_args, {f[0]}));\n' for f in G._fields_)
                   + "".join(f'    printf(" %zu", offsetof(gemlite_hip_experts_combine_args, {f}));\n' for f in names)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(G), C.sizeof(K)] + [getattr(G, f[0]).offset for f in G._fields_] + [getattr(K, f).offset for f in names]


@pytest.mark.parametrize("dt", [F16, B16])
@pytest.mark.parametrize("gs", [64, 128, 256])
def test_valid_glu_requests_are_accepted(dt, gs):
    for N, K in ((32, 256), (96, 768), (512, 4352), (1536, 2048)):
        for R in (0, 16, 32) + ((48, 64) if gs > 64 else ()):
            for bias in (True, False):
                assert glu_query(glu_request(R, N=N, K=K, gs=gs, dt=dt, bias=bias)) == OK, (N, K, R)
    assert glu_query(glu_request(gs=gs, dt=dt, scalar_zero=True)) == OK


GLU_REFUSALS = [
    ("struct_size + 4", set_("struct_size", C.sizeof(_hip.ExpertsRowsGluArgs) + 4), BAD_ARG),
    ("struct_size - 4", set_("struct_size", C.sizeof(_hip.ExpertsRowsGluArgs) - 4), BAD_ARG),
    ("nested struct_size", set_("rows.struct_size", C.sizeof(_hip.ExpertsRowsArgs) - 4), BAD_ARG),
    ("nested nested struct_size", set_("rows.experts.struct_size", C.sizeof(_hip.ExpertsArgs) - 4), BAD_ARG),
    # the rules of the nested request come through unchanged
    ("N % 16", set_("rows.experts.layer.N", 776), BAD_SHAPE), ("ids int16", set_("rows.experts.ids_dtype", DType.INT16.value), UNSUPPORTED),
    ("out 2-byte aligned", set_("rows.experts.layer.out", 0x50002), BAD_ARG), ("odd out stride", set_("rows.experts.stride_out_slot", 385), BAD_ARG),
    ("rows_per_block 24", set_("rows.rows_per_block", 24), BAD_ARG),
    ("workspace null", set_("rows.workspace", None), WORKSPACE),
    ("workspace one byte short", lambda g: set_("rows.workspace_bytes", g.rows.workspace_bytes - 1)(g), WORKSPACE),
    # the GLU forms' own
    ("N % 32", lambda g: (set_("rows.experts.layer.N", 784)(g), set_("rows.experts.layer.stride_wk", 784)(g)), BAD_SHAPE),
    ("activation 0", set_("activation", 0), UNSUPPORTED), ("activation 2", set_("activation", 2), UNSUPPORTED),
]


@pytest.mark.parametrize("what,change,status", GLU_REFUSALS, ids=[r[0] for r in GLU_REFUSALS])
def test_one_glu_refusal_per_rule(what, change, status):
    g = glu_request()
    assert glu_query(g) == OK
    change(g)
    assert glu_query(g) == status, what
    # the launch validates first too: a refused request never reaches a device
    assert _hip.load().gemlite_hip_forward_experts_rows_glu(C.byref(g), None) == status


def test_glu_refusals_that_depend_on_the_group_size():
    assert glu_query(glu_request(gs=32)) == UNSUPPORTED and glu_query(glu_request(16, gs=32)) == UNSUPPORTED
    assert glu_query(glu_request(48, gs=32)) == BAD_SHAPE  # (the nested request refuses 48 rows on groups of 32 first)
    for R in (48, 64):
        assert glu_query(glu_request(R, gs=64)) == BAD_SHAPE and glu_query(glu_request(R, gs=128)) == OK
        assert _hip.load().gemlite_hip_experts_rows_query(C.byref(glu_request(R, gs=64).rows)) == OK  # the plain launch takes them
    assert glu_query(glu_request(32, gs=64)) == OK
    assert _hip.load().gemlite_hip_experts_rows_glu_query(None) == BAD_ARG and _hip.load().gemlite_hip_experts_rows_glu_per_block(None) == BAD_ARG


def test_the_glu_block_size_is_the_plain_answer_under_the_glu_cap():
    lib = _hip.load()
    for n, E in ((6, 8), (96, 8), (112, 8), (216, 8), (320, 8), (65535, 8), (512, 128), (65535, 4096), (65535, 1024)):
        for gs in (64, 128, 256):
            g = glu_request(0, gs=gs)
            g.rows.experts.n_slots, g.rows.experts.n_experts = n, E
            plain = lib.gemlite_hip_experts_rows_per_block(C.byref(g.rows))
            assert plain > 0 and glu_rpb(g) == (plain if gs >= 128 else min(plain, 32)), (n, E, gs)
    g = glu_request(0, gs=64)
    g.rows.experts.n_slots = 8 * 40  # a mean of 40 slots per expert: the plain launch takes blocks of 64, the GLU launch 32
    assert lib.gemlite_hip_experts_rows_per_block(C.byref(g.rows)) == 64 and glu_rpb(g) == 32
    # the workspace of a default request is the table of THAT R (631 entries), not of the plain launch's 64 (914)
    need = lambda R: lib.gemlite_hip_experts_rows_workspace_bytes(320, 8, R)  # noqa: E731
    g.rows.workspace_bytes = need(32)
    assert need(32) == 4 * 631 < need(64) == 4 * 914 and glu_query(g) == OK
    g.rows.workspace_bytes = need(32) - 1
    assert glu_query(g) == WORKSPACE
    for R in (16, 32):
        assert glu_rpb(glu_request(R, gs=64)) == R
    assert glu_rpb(glu_request(0, gs=32)) == UNSUPPORTED and glu_rpb(glu_request(16, gs=32)) == UNSUPPORTED
    # it never reads the workspace fields
    g = glu_request(0)
    g.rows.workspace, g.rows.workspace_bytes = None, 0
    assert glu_rpb(g) == 16 and glu_query(g) == WORKSPACE


@pytest.mark.parametrize("dt", [F16, B16])
@pytest.mark.parametrize("ids", [I32, I64])
def test_valid_combine_requests_are_accepted(dt, ids):
    for w in (F32, dt):
        for n, spt, N in ((1, 1, 16), (12, 3, 48), (64 * 40, 64, 2048), (65535, 1, 16), (65535, 5, 4096)):
            assert combine_query(combine_request(n, spt, N, dt, ids, w)) == OK, (n, spt, N)
    c = combine_request(dt=dt, ids=ids)
    c.y, c.stride_y_slot, c.out, c.stride_out_token = 0x10004, 770, 0x40004, 1000  # 4-byte aligned rows, even strides
    assert combine_query(c) == OK


COMBINE_REFUSALS = [
    ("struct_size + 4", set_("struct_size", C.sizeof(_hip.ExpertsCombineArgs) + 4), BAD_ARG),
    ("struct_size - 4", set_("struct_size", C.sizeof(_hip.ExpertsCombineArgs) - 4), BAD_ARG),
    ("null y", set_("y", None), BAD_ARG), ("null ids", set_("ids", None), BAD_ARG), ("null weights", set_("weights", None), BAD_ARG),
    ("null out", set_("out", None), BAD_ARG),
    ("y 2-byte aligned", set_("y", 0x10002), BAD_ARG), ("out 2-byte aligned", set_("out", 0x40002), BAD_ARG),
    ("ids 4-byte aligned int64", set_("ids", 0x20004), BAD_ARG), ("weights 2-byte aligned fp32", set_("weights", 0x30002), BAD_ARG),
    ("odd y stride", set_("stride_y_slot", 769), BAD_ARG), ("odd out stride", set_("stride_out_token", 769), BAD_ARG),
    ("negative y stride", set_("stride_y_slot", -768), BAD_ARG), ("negative out stride", set_("stride_out_token", -768), BAD_ARG),
    ("no slots", set_("n_slots", 0), BAD_ARG), ("no experts", set_("n_experts", 0), BAD_ARG), ("slots per token 0", set_("slots_per_token", 0), BAD_ARG),
    ("negative slots per token", set_("slots_per_token", -3), BAD_ARG), ("N 0", set_("N", 0), BAD_ARG),
    ("fp32 y", set_("dtype", F32), UNSUPPORTED), ("int8 y", set_("dtype", DType.INT8.value), UNSUPPORTED),
    ("ids int16", set_("ids_dtype", DType.INT16.value), UNSUPPORTED), ("ids fp32", set_("ids_dtype", F32), UNSUPPORTED),
    ("weights of the other 16-bit type", set_("weights_dtype", B16), UNSUPPORTED), ("weights int32", set_("weights_dtype", I32), UNSUPPORTED),
    ("N % 16", set_("N", 776), BAD_SHAPE),
    ("slots per token 65", lambda c: (set_("slots_per_token", 65)(c), set_("n_slots", 130)(c)), BAD_SHAPE),
    ("not a divisor", set_("slots_per_token", 5), BAD_SHAPE),
    ("too many slots", lambda c: (set_("n_slots", 65536)(c), set_("slots_per_token", 1)(c)), BAD_SHAPE),
    ("y offsets at 2^31", set_("stride_y_slot", ((1 << 31) - 768 + 10) // 11 // 2 * 2 + 2), BAD_SHAPE),
    ("out offsets at 2^31", set_("stride_out_token", ((1 << 31) - 768 + 2) // 3 // 2 * 2 + 2), BAD_SHAPE),
]


@pytest.mark.parametrize("what,change,status", COMBINE_REFUSALS, ids=[r[0] for r in COMBINE_REFUSALS])
def test_one_combine_refusal_per_rule(what, change, status):
    c = combine_request()
    assert combine_query(c) == OK
    change(c)
    assert combine_query(c) == status, what
    assert _hip.load().gemlite_hip_experts_combine(C.byref(c), None) == status


def test_the_edges_of_the_combine_domain_are_inside():
    c = combine_request(64 * 3, 64, 16)
    assert combine_query(c) == OK
    # 11 strides of the largest even value with 11 s + 768 < 2^31, and 3 token strides
    c = combine_request()
    c.stride_y_slot = ((1 << 31) - 768 - 1) // 11 // 2 * 2
    c.stride_out_token = ((1 << 31) - 768 - 1) // 3 // 2 * 2
    assert 11 * c.stride_y_slot + 768 < (1 << 31) and combine_query(c) == OK
    assert _hip.load().gemlite_hip_experts_combine_query(None) == BAD_ARG


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def stacks(gs_gate=128, gs_down=128, E=3):
    gate = make_layers(E=E, N=256, K=768, gs=gs_gate, bias=False)
    up = make_layers(E=E, N=256, K=768, gs=gs_gate, bias=False, seed=1)
    return GemLiteExpertsMLP(GemLiteExperts.from_gate_up(gate, up), GemLiteExperts.from_layers(make_layers(E=E, N=768, K=256, gs=gs_down, bias=False)))


def test_rows_per_block_with_glu_and_the_unchanged_default():
    ex = GemLiteExperts.from_layers(make_layers(E=3, N=96))
    ex64 = GemLiteExperts.from_layers(make_layers(E=3, N=96, gs=64))
    ex32 = GemLiteExperts.from_layers(make_layers(E=3, N=96, gs=32))
    odd = GemLiteExperts.from_layers(make_layers(E=3, N=48))
    for n in (10, 3 * 30, 3 * 40):
        assert ex.rows_per_block(n, glu=True) == ex.rows_per_block(n) == ex.rows_per_block(n, None, False)
        assert ex64.rows_per_block(n, glu=True) == min(ex64.rows_per_block(n), 32)
    assert ex.rows_per_block(3 * 40) == 64 == ex64.rows_per_block(3 * 40) and ex.rows_per_block(10, 64, glu=True) == 64
    assert ex64.rows_per_block(10, 32, glu=True) == 32
    with pytest.raises(NotImplementedError, match="up to 32 for groups of 64"):
        ex64.rows_per_block(10, 48, glu=True)
    with pytest.raises(NotImplementedError, match="groups of 32 have no GLU form"):
        ex32.rows_per_block(10, glu=True)
    with pytest.raises(NotImplementedError, match="N % 32 == 0"):
        odd.rows_per_block(10, glu=True)
    with pytest.raises(ValueError, match="rows_per_block is 24"):
        ex.rows_per_block(10, 24, glu=True)


def test_the_mlp_keeps_its_block_size_and_the_fused_path_has_its_own():
    for gs_gate, gs_down, plain, fused in ((128, 128, 64, 64), (128, 32, 32, 32), (64, 128, 64, 32), (64, 32, 32, 32), (32, 128, 32, 32)):
        mlp = stacks(gs_gate, gs_down)
        assert mlp.rows_per_block(120) == plain, (gs_gate, gs_down)  # as before: min of the two plain answers
        assert mlp.rows_per_block(120) == min(mlp.gate_up.rows_per_block(120), mlp.down.rows_per_block(120))
        assert mlp.glu_fused() == (gs_gate != 32)
        assert mlp.rows_per_block_fused(120) == fused, (gs_gate, gs_down)
        if gs_gate != 32:
            assert fused == min(mlp.gate_up.rows_per_block(120, glu=True), mlp.down.rows_per_block(120))
        assert mlp.rows_per_block_fused(12) == 16


def test_the_new_methods_refuse_in_words_and_have_no_cpu_path():
    mlp = stacks()
    ex, ex64, ex32 = mlp.gate_up, stacks(64).gate_up, stacks(32).gate_up
    ids, x = torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 768, dtype=torch.float16)
    routing = ExpertsRouting(torch.zeros(X.rows_workspace_ints(10, 3, 48), dtype=torch.int32), 48, 10, 3)
    with pytest.raises(ValueError, match="asks for"):
        ex.forward_batched_glu(torch.zeros(5, 3, 768, dtype=torch.float16), ids, routing)
    with pytest.raises(NotImplementedError, match="x is torch.bfloat16"):
        ex.forward_batched_glu(x.bfloat16(), ids, routing)
    with pytest.raises(TypeError, match="ExpertsRouting"):
        ex.forward_batched_glu(x, ids, routing.workspace)
    with pytest.raises(ValueError, match="holds 10 slots over 3 experts"):
        ex.forward_batched_glu(x[:4], ids[:4], routing)
    with pytest.raises(NotImplementedError, match="up to 32 for groups of 64"):  # a routing above the GLU cap
        ex64.forward_batched_glu(x, ids, routing)
    with pytest.raises(NotImplementedError, match="groups of 32 have no GLU form"):
        ex32.forward_batched_glu(x, ids, ExpertsRouting(routing.workspace, 16, 10, 3))
    for call in (lambda: ex.forward_batched_glu(x, ids, routing), lambda: ex.forward_batched_glu(x, ids)):
        with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
            call()
    y, w = torch.zeros(5, 2, 48, dtype=torch.float16), torch.zeros(5, 2)
    with pytest.raises(ValueError, match="asks for"):
        ex.combine_batched(y[:4], ids, w)
    with pytest.raises(ValueError, match="one weight per slot"):
        ex.combine_batched(y, ids, torch.zeros(5, 3))
    with pytest.raises(NotImplementedError, match="float32 or torch.float16"):
        ex.combine_batched(y, ids, w.bfloat16())
    with pytest.raises(NotImplementedError, match="float16 or bfloat16"):
        ex.combine_batched(y.float(), ids, w)
    with pytest.raises(NotImplementedError, match="int32 or int64"):
        ex.combine_batched(y, ids.short(), w)
    with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
        ex.combine_batched(y, ids, w)
    with pytest.raises(ValueError, match="one weight per slot"):
        mlp.forward_batched_fused(x, ids, torch.zeros(5, 3))
    for m in (mlp, stacks(32)):  # with the GLU launch and with its stand-in
        with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
            m.forward_batched_fused(x, ids, w)


def test_the_fake_implementations_give_shape_and_dtype():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ex = GemLiteExperts.from_layers(make_layers(E=3, N=96))
    glu, combine = torch.ops.gemlite.forward_experts_rows_glu, torch.ops.gemlite.experts_combine
    assert "gemlite::forward_experts_rows_glu" in str(glu.default._schema) and "gemlite::experts_combine" in str(combine.default._schema)
    with FakeTensorMode() as mode:
        targs = [mode.from_tensor(t) for t in ex.get_tensor_args()]
        ids = torch.empty((5, 2), dtype=torch.int64)
        ws = torch.empty((X.rows_workspace_ints(10, 3, 16),), dtype=torch.int32)
        for x in (torch.empty((5, 768), dtype=torch.float16), torch.empty((5, 2, 768), dtype=torch.bfloat16)):
            h = glu(x, ids, ws, 16, None, targs, ex.get_meta_args())
            assert tuple(h.shape) == (5, 2, 48) and h.dtype == x.dtype
        with pytest.raises(Exception):
            glu(torch.empty((5, 3, 768), dtype=torch.float16), ids, ws, 16, None, targs, ex.get_meta_args())
        for dtype in (torch.float16, torch.bfloat16):
            for w in (torch.empty((5, 2)), torch.empty((5, 2), dtype=dtype)):
                out = combine(torch.empty((5, 2, 96), dtype=dtype), ids, w, 3)
                assert tuple(out.shape) == (5, 96) and out.dtype == dtype
        with pytest.raises(Exception):
            combine(torch.empty((5, 3, 96), dtype=torch.float16), ids, torch.empty((5, 2)), 3)
