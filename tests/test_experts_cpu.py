"""gemlite_hip_forward_experts / gemlite_hip_experts_query and gemlite_amd.GemLiteExperts, the parts that need no GPU: symbols, the
domain rules of include/gemlite_hip.h (one refusal per rule, with its status code), and the module on CPU tensors."""
import ctypes as C
import os
import re

import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteExperts, GemLiteLinear, _hip, experts as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, BAD_SHAPE = _hip.OK, _hip.ERR_BAD_ARGUMENT, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_SHAPE


def request(N=768, K=2048, gs=128, mode=3, dt=DType.FP16.value, scalar_zero=False, bias=True):
    """A valid request on stand-in addresses (the query dereferences nothing): 8 experts, 6 slots, 2 per x row."""
    e = _hip.ExpertsArgs()
    e.struct_size = C.sizeof(_hip.ExpertsArgs)
    e.ids_dtype = DType.INT64.value
    a = e.layer
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = -1
    a.x, a.w_q, a.scales, a.zeros, a.out = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.M, a.N, a.K = 1, N, K
    a.W_nbits, a.group_size, a.unpack_mask, a.elements_per_sample, a.w_pack_bits = 4, gs, 15, 8, 32
    a.w_dtype = DType.INT32.value
    a.input_dtype = a.output_dtype = a.meta_dtype = dt
    a.zeros_dtype = DType.INT32.value if scalar_zero else dt
    a.zero_is_scalar = int(scalar_zero)
    a.W_group_mode, a.channel_scale_mode = mode, 0
    a.stride_xm, a.stride_xk, a.stride_wk, a.stride_wn, a.stride_om, a.stride_on = K, 1, N, 1, N, 1
    a.stride_meta_g, a.stride_meta_n = N, 1
    e.ids = 0x60000
    e.bias = 0x70000 if bias else None
    e.n_slots, e.n_experts, e.slots_per_x_row = 6, 8, 2
    e.stride_expert_w, e.stride_expert_meta, e.stride_expert_bias = (K // 8) * N * 4, (K // gs) * N * 2, N * 2
    e.stride_x_row, e.stride_out_slot = K, N
    return e


def query(e):
    return _hip.load().gemlite_hip_experts_query(C.byref(e))


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in ("gemlite_hip_forward_experts", "gemlite_hip_experts_query"):
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
        assert getattr(lib, sym).argtypes[0] == C.POINTER(_hip.ExpertsArgs)
    assert lib.gemlite_hip_abi_version() == 1 and _hip.ABI_VERSION == 1
    assert "typedef struct gemlite_hip_experts_args" in header
    assert gemlite_amd.GemLiteExperts is X.GemLiteExperts


def test_no_kernel_label_was_added_for_the_experts_kernel():
    """gemlite_hip_kernel_name cannot report the experts kernel, so the sources hold no label literal for it."""
    csrc = os.path.join(ROOT, "gemlite_amd", "csrc")
    for f in os.listdir(csrc):
        if f.endswith((".hip", ".inc", ".h")):
            assert not re.search(r'"[a-z0-9_]*experts[a-z0-9_]*_kernel[<"]', open(os.path.join(csrc, f)).read()), f


@pytest.mark.parametrize("dt", [DType.FP16.value, DType.BF16.value])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("gs", [32, 64, 128, 256])
def test_valid_requests_are_accepted(dt, mode, gs):
    for N, K in ((48, 768), (256, 4352), (16, 256), (768, 2048), (32, 14336)):
        assert query(request(N, K, gs, mode, dt)) == OK, (N, K)
    if mode in (1, 3):
        assert query(request(gs=gs, mode=mode, dt=dt, scalar_zero=True)) == OK
    e = request(gs=gs, mode=mode, dt=dt, bias=False)
    e.ids_dtype = DType.INT32.value
    e.n_slots, e.stride_expert_w = 65535, 1 << 33
    assert query(e) == OK


def set_(path, value):
    def f(e):
        obj = e
        *head, last = path.split(".")
        for p in head:
            obj = getattr(obj, p)
        setattr(obj, last, value)
    return f


REFUSALS = [
    # BAD_ARGUMENT: null pointers, struct_size, non-positive counts, misaligned or negative strides
    ("null ids", set_("ids", None), BAD_ARG), ("null x", set_("layer.x", None), BAD_ARG), ("null w_q", set_("layer.w_q", None), BAD_ARG),
    ("null out", set_("layer.out", None), BAD_ARG), ("null scales", set_("layer.scales", None), BAD_ARG),
    ("null zeros", set_("layer.zeros", None), BAD_ARG),
    ("struct_size + 4", set_("struct_size", C.sizeof(_hip.ExpertsArgs) + 4), BAD_ARG),
    ("struct_size - 4", set_("struct_size", C.sizeof(_hip.ExpertsArgs) - 4), BAD_ARG),
    ("layer struct_size", set_("layer.struct_size", C.sizeof(_hip.ForwardArgs) - 4), BAD_ARG),
    ("no slots", set_("n_slots", 0), BAD_ARG), ("no experts", set_("n_experts", 0), BAD_ARG), ("negative experts", set_("n_experts", -1), BAD_ARG),
    ("slots per row 0", set_("slots_per_x_row", 0), BAD_ARG),
    ("w_q 8-byte aligned", set_("layer.w_q", 0x20008), BAD_ARG), ("stride_wk", set_("layer.stride_wk", 770), BAD_ARG),
    ("x 8-byte aligned", set_("layer.x", 0x10008), BAD_ARG), ("x row stride", set_("stride_x_row", 2052), BAD_ARG),
    ("scales 4-byte aligned", set_("layer.scales", 0x30004), BAD_ARG), ("zeros 4-byte aligned", set_("layer.zeros", 0x40004), BAD_ARG),
    ("metadata row stride", set_("layer.stride_meta_g", 770), BAD_ARG),
    ("expert stride w", set_("stride_expert_w", 768 * 256 * 4 + 8), BAD_ARG), ("expert stride meta", set_("stride_expert_meta", 16 * 768 * 2 + 4), BAD_ARG),
    ("expert stride bias", set_("stride_expert_bias", 768 * 2 + 1), BAD_ARG), ("odd bias", set_("bias", 0x70001), BAD_ARG),
    ("negative expert stride", set_("stride_expert_w", -16), BAD_ARG), ("negative out stride", set_("stride_out_slot", -768), BAD_ARG),
    # UNSUPPORTED: dtypes, bit width, modes, ids dtype
    ("fp32 input", set_("layer.input_dtype", DType.FP32.value), UNSUPPORTED), ("int8 input", set_("layer.input_dtype", DType.INT8.value), UNSUPPORTED),
    ("output dtype", set_("layer.output_dtype", DType.BF16.value), UNSUPPORTED), ("meta dtype", set_("layer.meta_dtype", DType.FP32.value), UNSUPPORTED),
    ("zeros dtype", set_("layer.zeros_dtype", DType.FP32.value), UNSUPPORTED),
    ("2 bits", lambda e: (set_("layer.W_nbits", 2)(e), set_("layer.elements_per_sample", 16)(e)), UNSUPPORTED),
    ("8 bits", lambda e: (set_("layer.W_nbits", 8)(e), set_("layer.elements_per_sample", 4)(e)), UNSUPPORTED),
    ("8-bit packing", lambda e: (set_("layer.w_pack_bits", 8)(e), set_("layer.elements_per_sample", 2)(e)), UNSUPPORTED),
    ("channel scales", set_("layer.channel_scale_mode", 1), UNSUPPORTED), ("W_group_mode 0", set_("layer.W_group_mode", 0), UNSUPPORTED),
    ("W_group_mode 5", set_("layer.W_group_mode", 5), UNSUPPORTED),
    ("ids int16", set_("ids_dtype", DType.INT16.value), UNSUPPORTED), ("ids fp32", set_("ids_dtype", DType.FP32.value), UNSUPPORTED),
    ("stride_on", set_("layer.stride_on", 2), UNSUPPORTED),
    # BAD_SHAPE: N, K, group size, slot count
    ("M 2", set_("layer.M", 2), BAD_SHAPE), ("N % 16", set_("layer.N", 776), BAD_SHAPE), ("K % 256", set_("layer.K", 2048 + 128), BAD_SHAPE),
    ("group 16", set_("layer.group_size", 16), BAD_SHAPE), ("group 96", set_("layer.group_size", 96), BAD_SHAPE),
    ("group does not divide K", lambda e: (set_("layer.K", 768)(e), set_("layer.group_size", 512)(e)), BAD_SHAPE),
    ("too many slots", set_("n_slots", 65536), BAD_SHAPE),
    ("weight offsets past 2^32", set_("layer.stride_wk", 1 << 22), BAD_SHAPE),
    ("metadata offsets past 2^32", set_("layer.stride_meta_g", 1 << 28), BAD_SHAPE),
]


@pytest.mark.parametrize("what,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_refusal_per_rule_of_the_domain(what, change, status):
    e = request()
    assert query(e) == OK
    change(e)
    assert query(e) == status, what


def test_a_null_request_and_a_scalar_zero_of_the_wrong_type_are_refused():
    assert _hip.load().gemlite_hip_experts_query(None) == BAD_ARG
    e = request(mode=3, scalar_zero=True)
    e.layer.zeros_dtype = DType.FP16.value
    assert query(e) == UNSUPPORTED
    # forward validates first too: a refused request never reaches a device
    e = request()
    e.n_slots = 0
    assert _hip.load().gemlite_hip_forward_experts(C.byref(e), None) == BAD_ARG


# ---- the module on CPU tensors --------------------------------------------------------------------------------------------------------
def make_layers(E=4, N=48, K=768, gs=128, dtype=torch.float16, zeros="tensor", bias=True, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    layers = []
    for _ in range(E):
        W_q = torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g)
        scales = (torch.rand(N * K // gs, 1, generator=g) * 0.02 + 0.005).to(dtype)
        z = (torch.rand(N * K // gs, 1, generator=g) * 4 + 6).to(dtype) if zeros == "tensor" else 8
        b = ((torch.rand(N, generator=g) - 0.5).to(dtype)) if bias else None
        lin = GemLiteLinear(4, gs, K, N, DType.FP16 if dtype == torch.float16 else DType.BF16, DType.FP16 if dtype == torch.float16 else DType.BF16)
        lin.pack(W_q.to(device), scales.to(device), z.to(device) if zeros == "tensor" else z, None if b is None else b.to(device))
        layers.append(lin)
    return layers


def test_from_layers_stacks_the_tensors_with_the_right_shapes_and_strides():
    layers = make_layers(E=4, N=48, K=768, gs=128)
    ex = GemLiteExperts.from_layers(layers)
    assert tuple(ex.W_q.shape) == (4, 96, 48) and ex.W_q.stride() == (96 * 48, 48, 1) and ex.W_q.dtype == torch.int32
    assert tuple(ex.scales.shape) == (4, 6, 48) and tuple(ex.zeros.shape) == (4, 6, 48) and tuple(ex.bias.shape) == (4, 48)
    assert ex.scales.is_contiguous() and ex.zeros.is_contiguous() and ex.num_experts == 4
    for i, lin in enumerate(layers):
        v = ex.expert(i)
        assert torch.equal(v.W_q, lin.W_q) and torch.equal(v.scales, lin.scales) and torch.equal(v.zeros, lin.zeros) and torch.equal(v.bias, lin.bias)
        assert v.W_q.data_ptr() == ex.W_q[i].data_ptr() and v.get_meta_args() == lin.get_meta_args()  # a view, not a copy
    a = X._static_args(ex.W_q, ex.scales, ex.zeros, ex.bias, ex.get_meta_args())
    assert (a.n_experts, a.stride_expert_w, a.stride_expert_meta, a.stride_expert_bias) == (4, 96 * 48 * 4, 6 * 48 * 2, 48 * 2)
    assert (a.layer.N, a.layer.K, a.layer.M, a.layer.W_group_mode) == (48, 768, 1, 4)
    # one scalar zero is kept once; del_orig frees the layers' tensors
    layers = make_layers(E=3, zeros="int", bias=False)
    ex = GemLiteExperts.from_layers(layers, del_orig=True)
    assert ex.zeros.numel() == 1 and ex.bias is None and all(l.W_q is None for l in layers)
    assert X._static_args(ex.W_q, ex.scales, ex.zeros, None, ex.get_meta_args()).layer.zero_is_scalar == 1


def test_mismatched_layers_and_layers_outside_the_domain_are_refused():
    a = make_layers(E=2)
    with pytest.raises(ValueError):
        GemLiteExperts.from_layers(a + make_layers(E=1, gs=64))
    with pytest.raises(ValueError):
        GemLiteExperts.from_layers(a + make_layers(E=1, N=64))
    with pytest.raises(ValueError):
        GemLiteExperts.from_layers(a + make_layers(E=1, bias=False))
    with pytest.raises(ValueError):
        GemLiteExperts.from_layers(a + make_layers(E=1, dtype=torch.bfloat16))
    with pytest.raises(ValueError):
        GemLiteExperts.from_layers([])
    with pytest.raises(NotImplementedError, match="K % 256"):
        GemLiteExperts.from_layers(make_layers(E=2, K=640))
    with pytest.raises(NotImplementedError, match="N % 16"):
        GemLiteExperts.from_layers(make_layers(E=2, N=40))
    lin8 = GemLiteLinear(8, 128, 768, 48, DType.FP16, DType.FP16)
    lin8.pack(torch.randint(0, 255, (48, 768), dtype=torch.uint8), torch.ones(48 * 6, 1, dtype=torch.float16), torch.ones(48 * 6, 1, dtype=torch.float16))
    with pytest.raises(NotImplementedError, match="4-bit"):
        GemLiteExperts.from_layers([lin8])


def test_state_dict_round_trip():
    ex = GemLiteExperts.from_layers(make_layers(E=3))
    sd = ex.state_dict()
    assert list(sd.keys()) == ["W_q", "bias", "scales", "zeros", "metadata", "orig_shape", "n_experts"]
    assert int(sd["n_experts"]) == 3 and [int(v) for v in sd["orig_shape"]] == [48, 768]
    ex2 = GemLiteExperts()
    ex2.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert ex2.get_meta_args() == ex.get_meta_args() and ex2.num_experts == 3 and (ex2.out_features, ex2.in_features) == (48, 768)
    for name in ("W_q", "bias", "scales", "zeros"):
        assert torch.equal(getattr(ex2, name), getattr(ex, name))
    assert torch.equal(ex2.expert(2).W_q, ex.expert(2).W_q)


def test_the_fake_implementation_gives_the_output_shape_for_both_x_layouts():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ex = GemLiteExperts.from_layers(make_layers(E=3))
    op = torch.ops.gemlite.forward_experts
    assert "gemlite::forward_experts" in str(op.default._schema)
    with FakeTensorMode() as mode:
        targs = [mode.from_tensor(t) for t in ex.get_tensor_args()]
        ids = torch.empty((5, 2), dtype=torch.int64)
        y = op(torch.empty((5, 768), dtype=torch.float16), ids, None, targs, ex.get_meta_args())
        assert tuple(y.shape) == (5, 2, 48) and y.dtype == torch.float16
        y = op(torch.empty((5, 2, 768), dtype=torch.float16), ids, None, targs, ex.get_meta_args())
        assert tuple(y.shape) == (5, 2, 48)
        with pytest.raises(Exception):
            op(torch.empty((5, 3, 768), dtype=torch.float16), ids, None, targs, ex.get_meta_args())
    # and there is no CPU path behind the real one
    with pytest.raises(_hip.GemliteHipError):
        ex(torch.zeros(5, 768, dtype=torch.float16), torch.zeros(5, 2, dtype=torch.int64))
