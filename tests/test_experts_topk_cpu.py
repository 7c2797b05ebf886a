"""gemlite_hip_experts_topk and what stands on it (experts_topk, ExpertsRouter, GemLiteExpertsMLP.forward_routed /
forward_batched_fused_routed), the parts that need no GPU: symbols, the struct layout against the header, one refusal per rule of the
domain, the edges, the fake op, the wrappers on CPU tensors, and the float64 restatement (tests/experts_topk_spec.py) against torch."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gemlite_amd import DType, ExpertsRouter, GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X, experts_topk
from tests import experts_topk_spec as spec
from tests.test_experts_cpu import make_layers, set_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, BAD_SHAPE = _hip.OK, _hip.ERR_BAD_ARGUMENT, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_SHAPE
F16, B16, F32, I32, I64 = (DType.FP16.value, DType.BF16.value, DType.FP32.value, DType.INT32.value, DType.INT64.value)
SYMBOLS = ("gemlite_hip_experts_topk", "gemlite_hip_experts_topk_query")
SOFTMAX, SIGMOID = _hip.EXPERTS_TOPK_SOFTMAX, _hip.EXPERTS_TOPK_SIGMOID


def topk_request(T=5, E=128, k=8, ldt=F16, ids=I32, w=F32, scoring=SOFTMAX, renorm=1, bias=False, stride=None):
    t = _hip.ExpertsTopkArgs()
    t.struct_size = C.sizeof(_hip.ExpertsTopkArgs)
    t.logits_dtype, t.ids_dtype, t.weights_dtype = ldt, ids, w
    t.scoring, t.renormalize, t.scale = scoring, renorm, 1.0
    t.logits, t.ids, t.weights = 0x10000, 0x20000, 0x30000
    t.bias = 0x40000 if bias else None
    t.n_tokens, t.n_experts, t.top_k = T, E, k
    t.stride_logits_token = E if stride is None else stride
    return t


def topk_query(t):
    return _hip.load().gemlite_hip_experts_topk_query(C.byref(t))


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in SYMBOLS:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes[0] == C.POINTER(_hip.ExpertsTopkArgs) and getattr(lib, sym).restype == C.c_int, sym
    assert lib.gemlite_hip_experts_topk.argtypes[1] == C.c_void_p and len(lib.gemlite_hip_experts_topk_query.argtypes) == 1
    assert lib.gemlite_hip_abi_version() == 1 and _hip.ABI_VERSION == 1
    assert "#define GEMLITE_EXPERTS_TOPK_MAX_EXPERTS 1024" in header and _hip.EXPERTS_TOPK_MAX_EXPERTS == 1024
    assert "#define GEMLITE_EXPERTS_TOPK_SOFTMAX 0" in header and "#define GEMLITE_EXPERTS_TOPK_SIGMOID 1" in header
    assert (SOFTMAX, SIGMOID) == (0, 1)


def test_the_struct_mirror_has_the_size_and_offsets_of_the_header(tmp_path):
    K = _hip.ExpertsTopkArgs
    names = [f[0] for f in K._fields_]
    assert names == ["struct_size", "logits_dtype", "ids_dtype", "weights_dtype", "scoring", "renormalize", "scale", "reserved0", "logits",
                     "bias", "ids", "weights", "n_tokens", "n_experts", "top_k", "stride_logits_token", "reserved"]
    assert C.sizeof(K) == 8 * 4 + 4 * 8 + 4 * 8 + 16 and K.reserved.offset == C.sizeof(K) - 16 and K.struct_size.offset == 0
    if shutil.which("gcc") is None:
        return  # the numbers above stand alone; with a C compiler the header itself is asked
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gemlite_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(gemlite_hip_experts_topk_args));\n'
                   + "".join(f'    printf(" %zu", offsetof(gemlite_hip_experts_topk_args, {f}));\n' for f in names)
                   + '    printf("\\n");\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(K)] + [getattr(K, f).offset for f in names]


@pytest.mark.parametrize("ldt", [F16, B16, F32])
@pytest.mark.parametrize("ids", [I32, I64])
def test_valid_requests_are_accepted(ldt, ids):
    for w in (F32, F16, B16):
        for T, E, k in ((1, 128, 8), (5, 8, 2), (257, 256, 8), (64, 512, 10), (3, 160, 6), (7, 65, 1)):
            for scoring, renorm, bias in ((SOFTMAX, 1, False), (SOFTMAX, 0, False), (SIGMOID, 1, False), (SIGMOID, 0, True), (SIGMOID, 1, True)):
                assert topk_query(topk_request(T, E, k, ldt, ids, w, scoring, renorm, bias)) == OK, (T, E, k, scoring, renorm, bias)
    t = topk_request(ldt=ldt, ids=ids, stride=1000)  # a padded row stride; element-aligned pointers
    t.logits = 0x10000 + (4 if ldt == F32 else 2)
    t.weights = 0x30004
    assert topk_query(t) == OK


REFUSALS = [
    # BAD_ARGUMENT: struct_size, null or misaligned pointers, non-positive counts, a renormalize flag that is no flag
    ("struct_size + 4", set_("struct_size", C.sizeof(_hip.ExpertsTopkArgs) + 4), BAD_ARG),
    ("struct_size - 4", set_("struct_size", C.sizeof(_hip.ExpertsTopkArgs) - 4), BAD_ARG),
    ("null logits", set_("logits", None), BAD_ARG), ("null ids", set_("ids", None), BAD_ARG), ("null weights", set_("weights", None), BAD_ARG),
    ("odd fp16 logits", set_("logits", 0x10001), BAD_ARG),
    ("2-byte aligned fp32 logits", lambda t: (set_("logits_dtype", F32)(t), set_("logits", 0x10002)(t)), BAD_ARG),
    ("2-byte aligned int32 ids", set_("ids", 0x20002), BAD_ARG),
    ("4-byte aligned int64 ids", lambda t: (set_("ids_dtype", I64)(t), set_("ids", 0x20004)(t)), BAD_ARG),
    ("2-byte aligned fp32 weights", set_("weights", 0x30002), BAD_ARG),
    ("odd fp16 weights", lambda t: (set_("weights_dtype", F16)(t), set_("weights", 0x30001)(t)), BAD_ARG),
    ("2-byte aligned bias", lambda t: (set_("scoring", SIGMOID)(t), set_("bias", 0x40002)(t)), BAD_ARG),
    ("no tokens", set_("n_tokens", 0), BAD_ARG), ("negative tokens", set_("n_tokens", -1), BAD_ARG),
    ("no experts", set_("n_experts", 0), BAD_ARG), ("top_k 0", set_("top_k", 0), BAD_ARG), ("negative top_k", set_("top_k", -2), BAD_ARG),
    ("renormalize 2", set_("renormalize", 2), BAD_ARG),
    # UNSUPPORTED: dtypes, the scoring mode, a bias without sigmoid
    ("int8 logits", set_("logits_dtype", DType.INT8.value), UNSUPPORTED), ("fp8 logits", set_("logits_dtype", DType.FP8.value), UNSUPPORTED),
    ("ids int16", set_("ids_dtype", DType.INT16.value), UNSUPPORTED), ("ids fp32", set_("ids_dtype", F32), UNSUPPORTED),
    ("weights int32", set_("weights_dtype", I32), UNSUPPORTED), ("weights fp8", set_("weights_dtype", DType.FP8.value), UNSUPPORTED),
    ("scoring 2", set_("scoring", 2), UNSUPPORTED), ("scoring -1", set_("scoring", -1), UNSUPPORTED),
    ("a bias with softmax", set_("bias", 0x40000), UNSUPPORTED),
    # BAD_SHAPE: the expert count, top_k, the row stride, n_tokens * top_k
    ("1025 experts", lambda t: (set_("n_experts", 1025)(t), set_("stride_logits_token", 1025)(t)), BAD_SHAPE),
    ("top_k above E", lambda t: (set_("n_experts", 6)(t), set_("stride_logits_token", 6)(t), set_("top_k", 7)(t)), BAD_SHAPE),
    ("top_k 65", set_("top_k", 65), BAD_SHAPE),
    ("row stride below E", set_("stride_logits_token", 127), BAD_SHAPE), ("row stride 0", set_("stride_logits_token", 0), BAD_SHAPE),
    ("negative row stride", set_("stride_logits_token", -128), BAD_SHAPE),
    ("n_tokens * top_k at 2^32", set_("n_tokens", (1 << 32) // 8), BAD_SHAPE),
]


@pytest.mark.parametrize("what,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_refusal_per_rule_of_the_domain(what, change, status):
    t = topk_request()
    assert topk_query(t) == OK
    change(t)
    assert topk_query(t) == status, what
    # the launch validates first too: a refused request never reaches a device
    assert _hip.load().gemlite_hip_experts_topk(C.byref(t), None) == status


def test_the_edges_of_the_domain_are_inside():
    assert topk_query(topk_request(E=1, k=1)) == OK
    assert topk_query(topk_request(E=1024, k=8)) == OK and topk_query(topk_request(E=1024, k=64)) == OK
    for E in (2, 17, 63, 64):
        assert topk_query(topk_request(E=E, k=E)) == OK, E  # top_k = E
    assert topk_query(topk_request(E=64, k=64)) == OK and topk_query(topk_request(E=65, k=64)) == OK
    assert topk_query(topk_request(T=((1 << 32) - 1) // 8, k=8)) == OK  # the last n_tokens with n_tokens * top_k < 2^32
    assert topk_query(topk_request(T=(1 << 32) - 1, E=1, k=1)) == OK and topk_query(topk_request(T=1 << 32, E=1, k=1)) == BAD_SHAPE
    assert _hip.load().gemlite_hip_experts_topk_query(None) == BAD_ARG and _hip.load().gemlite_hip_experts_topk(None, None) == BAD_ARG


# ---- the Python layer -------------------------------------------------------------------------------------------------------------------
def test_the_fake_op_gives_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    op = torch.ops.gemlite.experts_topk
    assert "gemlite::experts_topk" in str(op.default._schema)
    with FakeTensorMode():
        for shape in ((128,), (5, 128), (2, 3, 128)):
            for ldt in (torch.float16, torch.bfloat16, torch.float32):
                for idt, wdt in ((torch.int32, torch.float32), (torch.int64, torch.bfloat16), (torch.int32, torch.float16)):
                    ids, w = op(torch.empty(shape, dtype=ldt), 8, "softmax", True, 1.0, None, idt, wdt)
                    assert tuple(ids.shape) == tuple(w.shape) == shape[:-1] + (8,) and ids.dtype == idt and w.dtype == wdt
        ids, w = op(torch.empty((4, 256), dtype=torch.float32), 8, "sigmoid", True, 2.5, torch.empty(256), torch.int32, torch.float32)
        assert tuple(ids.shape) == (4, 8)
        for bad in (lambda: op(torch.empty((4, 6)), 7, "softmax", True, 1.0, None, torch.int32, torch.float32),
                    lambda: op(torch.empty((4, 128)), 8, "softmax", True, 1.0, torch.empty(128), torch.int32, torch.float32),
                    lambda: op(torch.empty((4, 128)), 8, "sigmoid", True, 1.0, torch.empty(64), torch.int32, torch.float32),
                    lambda: op(torch.empty((4, 128), dtype=torch.float64), 8, "softmax", True, 1.0, None, torch.int32, torch.float32)):
            with pytest.raises(Exception):
                bad()


def test_the_wrappers_refuse_in_words_and_have_no_cpu_path():
    l = torch.zeros(5, 128, dtype=torch.float16)
    with pytest.raises(ValueError, match="'softmax' or 'sigmoid'"):
        experts_topk(l, 8, scoring="tanh")
    with pytest.raises(NotImplementedError, match="float16, bfloat16 or float32"):
        experts_topk(l.double(), 8)
    with pytest.raises(NotImplementedError, match="int32 or int64"):
        experts_topk(l, 8, ids_dtype=torch.int16)
    with pytest.raises(NotImplementedError, match="float32, float16 or bfloat16"):
        experts_topk(l, 8, weights_dtype=torch.float64)
    with pytest.raises(NotImplementedError, match="1025 experts"):
        experts_topk(torch.zeros(2, 1025), 8)
    for k in (0, 65, 129):
        with pytest.raises(NotImplementedError, match=f"top_k={k} of 128 experts"):
            experts_topk(l, k)
    with pytest.raises(NotImplementedError, match="top_k=7 of 6 experts"):
        experts_topk(torch.zeros(3, 6), 7)
    with pytest.raises(ValueError, match="sigmoid"):
        experts_topk(l, 8, bias=torch.zeros(128))
    with pytest.raises(ValueError, match=r"float32 \(128,\)"):
        experts_topk(l, 8, scoring="sigmoid", bias=torch.zeros(64))
    with pytest.raises(ValueError, match=r"float32 \(128,\)"):
        experts_topk(l, 8, scoring="sigmoid", bias=torch.zeros(128, dtype=torch.float16))
    with pytest.raises(ValueError, match=r"\[\.\.\., E\]"):
        experts_topk(torch.tensor(1.0), 1)
    for call in (lambda: experts_topk(l, 8), lambda: experts_topk(l, 8, "sigmoid", bias=torch.zeros(128)),
                 lambda: ExpertsRouter(8)(l), lambda: ExpertsRouter(8, "sigmoid", bias=torch.zeros(128))(l.float())):
        with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
            call()


def test_the_router_module_keeps_its_settings_and_its_bias_is_a_buffer():
    r = ExpertsRouter(8, "sigmoid", renormalize=True, scale=2.5, bias=torch.arange(16, dtype=torch.float64) / 8, weights_dtype=torch.bfloat16)
    assert (r.top_k, r.scoring, r.renormalize, r.scale, r.weights_dtype) == (8, "sigmoid", True, 2.5, torch.bfloat16)
    assert r.bias.dtype == torch.float32 and "bias" in dict(r.named_buffers()) and "bias" in r.state_dict() and not list(r.parameters())
    r2 = ExpertsRouter(8, "sigmoid", bias=torch.zeros(16))
    r2.load_state_dict(r.state_dict())
    assert torch.equal(r2.bias, r.bias)
    plain = ExpertsRouter(2)
    assert plain.bias is None and plain.state_dict() == {} and (plain.scoring, plain.renormalize, plain.scale) == ("softmax", True, 1.0)
    with pytest.raises(ValueError, match="'softmax' or 'sigmoid'"):
        ExpertsRouter(2, "relu")
    with pytest.raises(ValueError, match="sigmoid"):
        ExpertsRouter(2, "softmax", bias=torch.zeros(8))
    with pytest.raises(NotImplementedError, match="top_k=65"):
        ExpertsRouter(65)


def test_the_routed_mlp_methods_reach_the_router_first_and_have_no_cpu_path():
    gate = make_layers(E=3, N=256, K=768, bias=False)
    up = make_layers(E=3, N=256, K=768, bias=False, seed=1)
    mlp = GemLiteExpertsMLP(GemLiteExperts.from_gate_up(gate, up), GemLiteExperts.from_layers(make_layers(E=3, N=768, K=256, bias=False)))
    x, logits = torch.zeros(5, 768, dtype=torch.float16), torch.zeros(5, 3, dtype=torch.float16)
    for method in (mlp.forward_routed, mlp.forward_batched_fused_routed):
        with pytest.raises(NotImplementedError, match="top_k=4 of 3 experts"):
            method(x, logits, ExpertsRouter(4))
        with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
            method(x, logits, ExpertsRouter(2))


# ---- the restatement against torch ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [1, 64, 65, 128, 160, 1024])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
def test_on_tie_free_logits_the_spec_selects_what_torch_topk_of_the_softmax_selects(E, dtype):
    k = min(E, 8)
    logits = spec.tie_free_logits(6, E, dtype, seed=E)
    assert all(logits[t].double().unique().numel() == E for t in range(6))  # exact in every type: still tie-free
    ids, w = spec.topk(logits, k, "softmax", True)
    for prec in (torch.float64, torch.float32):
        p = torch.softmax(logits.to(prec), -1)
        tv, ti = torch.topk(p, k, dim=-1, sorted=True)
        assert np.array_equal(ids, ti.numpy()), (E, dtype, prec)
    tv, _ = torch.topk(torch.softmax(logits.double(), -1), k, dim=-1)
    np.testing.assert_allclose(w, (tv / tv.sum(-1, keepdim=True)).numpy(), rtol=1e-12)
    _, w_all = spec.topk(logits, k, "softmax", False, scale=2.0)
    np.testing.assert_allclose(w_all, 2.0 * tv.numpy(), rtol=1e-12)
    # sigmoid without a bias selects the same experts; its weights are the sigmoids
    ids_s, w_s = spec.topk(logits, k, "sigmoid", False)
    assert np.array_equal(ids_s, ids)
    np.testing.assert_allclose(w_s, torch.sigmoid(logits.double()).gather(-1, torch.from_numpy(ids)).numpy(), rtol=1e-12)


def test_the_spec_orders_ties_by_index_and_nan_above_infinity():
    inf, nan = float("inf"), float("nan")
    key = np.array([[1.0, 3.0, 3.0, -inf, 3.0, 2.0],
                    [nan, inf, 5.0, nan, -inf, inf],
                    [-0.0, 0.0, -0.0, 0.0, -1.0, -0.0],
                    [-inf, -inf, -inf, -inf, -inf, -inf]])
    assert spec.select(key, 6).tolist() == [[1, 2, 4, 5, 0, 3], [0, 3, 1, 5, 2, 4], [0, 1, 2, 3, 5, 4], [0, 1, 2, 3, 4, 5]]
    # with a bias the key is sigmoid + bias, and the weights leave the bias out
    logits = torch.tensor([[0.0, 2.0, -2.0, 1.0]])
    bias = torch.tensor([0.5, -0.5, 0.5, 0.0])
    ids, w = spec.topk(logits, 2, "sigmoid", True, 1.0, bias)
    assert ids.tolist() == [[0, 3]]  # keys 1.0, 0.38, 0.62, 0.73
    s = 1 / (1 + np.exp(-np.array([0.0, 1.0])))
    np.testing.assert_allclose(w[0], s / s.sum(), rtol=1e-15)
