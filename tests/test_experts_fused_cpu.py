"""gemlite_hip_forward_experts_fused / gemlite_hip_experts_fused_query, GemLiteExperts.forward_glu / forward_combine / from_gate_up and
GemLiteExpertsMLP, the parts that need no GPU: symbols, the fused rules of include/gemlite_hip.h (one refusal per rule, with its status
code), the fake implementations and the modules on CPU tensors."""
import ctypes as C
import os

import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X
from tests.test_experts_cpu import make_layers, request, set_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, BAD_SHAPE = _hip.OK, _hip.ERR_BAD_ARGUMENT, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_SHAPE
GLU, COMBINE = _hip.EXPERTS_GLU, _hip.EXPERTS_COMBINE


def fused(epilogue, spt=1, wdt=DType.FP32.value, n_slots=None, **kw):
    """A valid fused request on stand-in addresses around test_experts_cpu.request()."""
    e = request(**kw)
    e.n_slots = spt * 3 if n_slots is None else n_slots
    e.slots_per_x_row = 1
    f = _hip.ExpertsFusedArgs()
    f.struct_size = C.sizeof(_hip.ExpertsFusedArgs)
    f.epilogue = epilogue
    f.experts = e
    f.activation = _hip.ACT_SILU
    f.weights_dtype = wdt
    f.weights = 0x80000
    f.slots_per_token = spt
    return f


def query(f):
    return _hip.load().gemlite_hip_experts_fused_query(C.byref(f))


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in ("gemlite_hip_forward_experts_fused", "gemlite_hip_experts_fused_query"):
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes[0] == C.POINTER(_hip.ExpertsFusedArgs)
    assert lib.gemlite_hip_abi_version() == 1 and _hip.ABI_VERSION == 1
    assert "typedef struct gemlite_hip_experts_fused_args" in header
    for name, value in (("GEMLITE_EXPERTS_GLU", GLU), ("GEMLITE_EXPERTS_COMBINE", COMBINE), ("GEMLITE_ACT_SILU", _hip.ACT_SILU)):
        assert f"#define {name} {value}" in header
    # the nested struct is the unfused one, unchanged, behind the two leading words
    F = _hip.ExpertsFusedArgs
    assert F.experts.offset == 8 and F.experts.size == C.sizeof(_hip.ExpertsArgs)
    assert C.sizeof(F) == 8 + C.sizeof(_hip.ExpertsArgs) + 8 + 8 + 8 + 24
    assert gemlite_amd.GemLiteExpertsMLP is X.GemLiteExpertsMLP


@pytest.mark.parametrize("dt", [DType.FP16.value, DType.BF16.value])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("gs", [32, 64, 128, 256])
def test_valid_requests_are_accepted(dt, mode, gs):
    for N, K in ((32, 256), (96, 768), (512, 4352), (1536, 2048)):
        assert query(fused(GLU, N=N, K=K, gs=gs, mode=mode, dt=dt)) == OK, (N, K)
    for N, K in ((16, 256), (48, 768), (2048, 768)):
        for spt in (1, 3, 8, 16):
            assert query(fused(COMBINE, spt, N=N, K=K, gs=gs, mode=mode, dt=dt)) == OK, (N, K, spt)
            assert query(fused(COMBINE, spt, wdt=dt, N=N, K=K, gs=gs, mode=mode, dt=dt)) == OK, (N, K, spt)
    if mode in (1, 3):
        assert query(fused(GLU, gs=gs, mode=mode, dt=dt, scalar_zero=True, bias=False)) == OK
        assert query(fused(COMBINE, 8, gs=gs, mode=mode, dt=dt, scalar_zero=True, bias=False)) == OK
    # fields of the other epilogue are not read
    f = fused(GLU, gs=gs, mode=mode, dt=dt)
    f.weights, f.slots_per_token, f.weights_dtype = None, 0, -1
    assert query(f) == OK
    f = fused(COMBINE, 2, N=48, gs=gs, mode=mode, dt=dt)
    f.activation = 0
    assert query(f) == OK


FUSED_REFUSALS = [
    ("struct_size + 8", GLU, set_("struct_size", C.sizeof(_hip.ExpertsFusedArgs) + 8), BAD_ARG),
    ("struct_size of the nested struct", COMBINE, set_("struct_size", C.sizeof(_hip.ExpertsArgs)), BAD_ARG),
    ("null weights", COMBINE, set_("weights", None), BAD_ARG),
    ("fp32 weights 2-byte aligned", COMBINE, set_("weights", 0x80002), BAD_ARG),
    ("16-bit weights at an odd address", COMBINE, lambda f: (set_("weights_dtype", DType.FP16.value)(f), set_("weights", 0x80001)(f)), BAD_ARG),
    ("slots_per_token 0", COMBINE, set_("slots_per_token", 0), BAD_ARG),
    ("slots_per_token -1", COMBINE, set_("slots_per_token", -1), BAD_ARG),
    ("epilogue 0", GLU, set_("epilogue", 0), UNSUPPORTED),
    ("epilogue 3", COMBINE, set_("epilogue", 3), UNSUPPORTED),
    ("activation 0", GLU, set_("activation", 0), UNSUPPORTED),
    ("activation 2", GLU, set_("activation", 2), UNSUPPORTED),
    ("weights of the other 16-bit type", COMBINE, set_("weights_dtype", DType.BF16.value), UNSUPPORTED),
    ("int32 weights", COMBINE, set_("weights_dtype", DType.INT32.value), UNSUPPORTED),
    ("GLU with N % 32", GLU, set_("experts.layer.N", 784), BAD_SHAPE),
    ("slots_per_token 17", COMBINE, lambda f: (set_("slots_per_token", 17)(f), set_("experts.n_slots", 34)(f)), BAD_SHAPE),
    ("slots_per_token does not divide n_slots", COMBINE, set_("experts.n_slots", 25), BAD_SHAPE),
    # the nested request is refused by its own rules, with its own status
    ("nested K % 256", GLU, set_("experts.layer.K", 2048 + 128), BAD_SHAPE),
    ("nested null ids", COMBINE, set_("experts.ids", None), BAD_ARG),
    ("nested ids dtype", GLU, set_("experts.ids_dtype", DType.INT16.value), UNSUPPORTED),
    ("nested struct_size", COMBINE, set_("experts.struct_size", C.sizeof(_hip.ExpertsArgs) - 4), BAD_ARG),
    ("nested slot count", GLU, set_("experts.n_slots", 65536), BAD_SHAPE),
]


@pytest.mark.parametrize("what,epilogue,change,status", FUSED_REFUSALS, ids=[r[0] for r in FUSED_REFUSALS])
def test_one_refusal_per_fused_rule_and_nested_refusals_come_through(what, epilogue, change, status):
    f = fused(epilogue, 8)
    assert query(f) == OK
    change(f)
    assert query(f) == status, what
    # forward validates first too: a refused request never reaches a device
    assert _hip.load().gemlite_hip_forward_experts_fused(C.byref(f), None) == status, what


def test_a_null_request_is_refused():
    assert _hip.load().gemlite_hip_experts_fused_query(None) == BAD_ARG
    assert _hip.load().gemlite_hip_forward_experts_fused(None, None) == BAD_ARG


# ---- the ops and the modules on CPU tensors -------------------------------------------------------------------------------------------
def test_the_fake_implementations_give_shape_and_dtype_for_both_x_layouts():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ex = GemLiteExperts.from_layers(make_layers(E=3, N=64))
    glu, combine = torch.ops.gemlite.forward_experts_glu, torch.ops.gemlite.forward_experts_combine
    assert "gemlite::forward_experts_glu" in str(glu.default._schema) and "gemlite::forward_experts_combine" in str(combine.default._schema)
    with FakeTensorMode() as mode:
        targs = [mode.from_tensor(t) for t in ex.get_tensor_args()]
        ids = torch.empty((5, 2), dtype=torch.int64)
        for x in (torch.empty((5, 768), dtype=torch.float16), torch.empty((5, 2, 768), dtype=torch.float16)):
            y = glu(x, ids, None, targs, ex.get_meta_args())
            assert tuple(y.shape) == (5, 2, 32) and y.dtype == torch.float16
            for w in (torch.empty((5, 2), dtype=torch.float32), torch.empty((5, 2), dtype=torch.float16)):
                y = combine(x, ids, w, None, targs, ex.get_meta_args())
                assert tuple(y.shape) == (5, 64) and y.dtype == torch.float16
        x = torch.empty((5, 768), dtype=torch.float16)
        with pytest.raises(Exception):
            glu(torch.empty((5, 3, 768), dtype=torch.float16), ids, None, targs, ex.get_meta_args())
        for w in (torch.empty((5, 3)), torch.empty((5,)), torch.empty((2, 5)), torch.empty((5, 2, 1))):
            with pytest.raises(Exception):
                combine(x, ids, w, None, targs, ex.get_meta_args())
        with pytest.raises(Exception):
            combine(x, ids, torch.empty((5, 2), dtype=torch.bfloat16), None, targs, ex.get_meta_args())


def test_from_gate_up_concatenates_each_pair_along_n_and_refuses_mismatches():
    gate, up = make_layers(E=3, N=48, seed=1), make_layers(E=3, N=48, seed=2)
    ex = GemLiteExperts.from_gate_up(gate, up)
    assert (ex.out_features, ex.in_features, ex.num_experts) == (96, 768, 3)
    assert tuple(ex.W_q.shape) == (3, 96, 96) and tuple(ex.scales.shape) == (3, 6, 96) and tuple(ex.bias.shape) == (3, 96)
    assert ex.W_q.is_contiguous() and ex.scales.is_contiguous() and ex.zeros.is_contiguous()
    for i, (g, u) in enumerate(zip(gate, up)):
        for name in ("W_q", "scales", "zeros", "bias"):
            assert torch.equal(getattr(ex, name)[i], torch.cat([getattr(g, name), getattr(u, name)], dim=-1)), (i, name)
        assert ex.expert(i).get_meta_args() == g.get_meta_args()
    assert [int(v) for v in ex.state_dict()["orig_shape"]] == [96, 768]
    # a scalar zero is kept once, no bias stays no bias, del_orig frees both lists
    gate, up = make_layers(E=2, zeros="int", bias=False, seed=1), make_layers(E=2, zeros="int", bias=False, seed=2)
    ex = GemLiteExperts.from_gate_up(gate, up, del_orig=True)
    assert ex.zeros.numel() == 1 and ex.bias is None and all(l.W_q is None for l in gate + up)
    a = make_layers(E=2)
    for other in (make_layers(E=2, gs=64), make_layers(E=2, N=64), make_layers(E=2, bias=False), make_layers(E=2, dtype=torch.bfloat16),
                  make_layers(E=2, K=1024), make_layers(E=3)):
        with pytest.raises(ValueError):
            GemLiteExperts.from_gate_up(a, other)
    with pytest.raises(ValueError):
        GemLiteExperts.from_gate_up([], [])


def make_mlp(E=3, H=256, I=256):
    """hidden H -> [gate; up] 2 I -> hidden H"""
    return GemLiteExpertsMLP.from_layers(make_layers(E=E, N=I, K=H, seed=1), make_layers(E=E, N=I, K=H, seed=2),
                                         make_layers(E=E, N=H, K=I, seed=3))


def test_the_mlp_checks_its_two_halves_and_round_trips_its_state_dict():
    mlp = make_mlp()
    gate_up, down = mlp.gate_up, mlp.down
    assert (gate_up.out_features, gate_up.in_features, down.out_features, down.in_features) == (512, 256, 256, 256)
    assert (mlp.hidden_size, mlp.intermediate_size, mlp.num_experts) == (256, 256, 3)
    narrow = GemLiteExperts.from_gate_up(make_layers(E=3, N=64, K=256, seed=1), make_layers(E=3, N=64, K=256, seed=2))
    with pytest.raises(ValueError, match="2 \\* down.in_features"):
        GemLiteExpertsMLP(narrow, down)
    with pytest.raises(ValueError, match="hidden"):
        GemLiteExpertsMLP(gate_up, GemLiteExperts.from_layers(make_layers(E=3, N=512, K=256)))
    with pytest.raises(ValueError, match="experts"):
        GemLiteExpertsMLP(gate_up, GemLiteExperts.from_layers(make_layers(E=4, N=256, K=256)))
    with pytest.raises(ValueError, match="dtype"):
        GemLiteExpertsMLP(gate_up, GemLiteExperts.from_layers(make_layers(E=3, N=256, K=256, dtype=torch.bfloat16)))
    with pytest.raises(ValueError):
        GemLiteExpertsMLP(gate_up, None)
    sd = mlp.state_dict()
    inner = ["W_q", "bias", "scales", "zeros", "metadata", "orig_shape", "n_experts"]
    assert list(sd.keys()) == ["gate_up." + k for k in inner] + ["down." + k for k in inner]
    assert list(gate_up.state_dict().keys()) == inner
    mlp2 = GemLiteExpertsMLP()
    mlp2.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert (mlp2.hidden_size, mlp2.intermediate_size, mlp2.num_experts) == (256, 256, 3)
    for half in ("gate_up", "down"):
        a, b = getattr(mlp, half), getattr(mlp2, half)
        assert a.get_meta_args() == b.get_meta_args() and (a.out_features, a.in_features) == (b.out_features, b.in_features)
        for name in ("W_q", "bias", "scales", "zeros"):
            assert torch.equal(getattr(a, name), getattr(b, name))


def test_there_is_no_cpu_path_and_domain_refusals_come_in_words():
    mlp = make_mlp()
    gate_up, down = mlp.gate_up, mlp.down
    x, ids, w = torch.zeros(5, 256, dtype=torch.float16), torch.zeros(5, 2, dtype=torch.int64), torch.ones(5, 2)
    with pytest.raises(_hip.GemliteHipError):
        gate_up.forward_glu(x, ids)
    with pytest.raises(_hip.GemliteHipError):
        down.forward_combine(x, ids, w)
    with pytest.raises(_hip.GemliteHipError):
        mlp(x, ids, w)
    with pytest.raises(_hip.GemliteHipError):
        torch.ops.gemlite.forward_experts_glu(x, ids, gate_up.bias, gate_up.get_tensor_args(), gate_up.get_meta_args())
    with pytest.raises(_hip.GemliteHipError):
        torch.ops.gemlite.forward_experts_combine(x, ids, w, down.bias, down.get_tensor_args(), down.get_meta_args())
    odd = GemLiteExperts.from_layers(make_layers(E=2, N=48, K=256))
    with pytest.raises(NotImplementedError, match="N % 32"):
        odd.forward_glu(x, ids)
    with pytest.raises(NotImplementedError, match="top_k > 16"):
        down.forward_combine(x, torch.zeros(5, 17, dtype=torch.int64), torch.ones(5, 17))
    with pytest.raises(NotImplementedError, match="float16"):
        down.forward_combine(x.to(torch.bfloat16), ids, w)
    # forward itself is what it was
    with pytest.raises(_hip.GemliteHipError):
        down(x, ids)
