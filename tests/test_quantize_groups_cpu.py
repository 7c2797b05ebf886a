"""Host side of the grouped INT weight quantiser (gemlite_hip_quantize_groups, WeightQuantizerINT, the *_RTN_INT
processors): the C ABI entry and its validation table (nothing is launched), loud failure on CPU tensors, which classes
have which constructors, and the error bound of the contract on its torch restatement alone."""
import ctypes as C
import os
import re

import pytest
import torch

from gemlite_amd import _hip, helper
from gemlite_amd.quant_utils import WeightQuantizerINT
from tests.quant_int_spec import error_bound, planted_weights, quantize_groups_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16, BF16, INT8 = 0, 1, 2, 4


def test_symbol_is_declared_exported_and_abi_is_1():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    assert re.search(r"\bint\s+gemlite_hip_quantize_groups\s*\(", header)
    assert "gemlite_hip_quantize_groups" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "gemlite_hip_quantize_groups")
    assert lib.gemlite_hip_abi_version() == 1 == _hip.ABI_VERSION


def _args(**kw):
    a = _hip.QuantizeArgs()
    a.struct_size = C.sizeof(_hip.QuantizeArgs)
    a.w, a.q_out, a.scales, a.zeros = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every row below is refused
    a.w_dtype, a.meta_dtype = FP16, FP16
    a.N, a.K, a.ld_w, a.ld_q = 64, 256, 256, 256
    a.W_nbits, a.group_size, a.pack_bits = 4, 64, 32
    a.stride_meta_g, a.stride_meta_n, a.fold_zeros = 64, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return a


VALIDATION = [
    ("null w", dict(w=None), _hip.ERR_BAD_ARGUMENT),
    ("null q_out", dict(q_out=None), _hip.ERR_BAD_ARGUMENT),
    ("null scales", dict(scales=None), _hip.ERR_BAD_ARGUMENT),
    ("null zeros", dict(zeros=None), _hip.ERR_BAD_ARGUMENT),
    ("struct_size", dict(struct_size=C.sizeof(_hip.QuantizeArgs) - 8), _hip.ERR_BAD_ARGUMENT),
    ("N = 0", dict(N=0), _hip.ERR_BAD_ARGUMENT),
    ("K < 0", dict(K=-256), _hip.ERR_BAD_ARGUMENT),
    ("group_size = 0", dict(group_size=0), _hip.ERR_BAD_ARGUMENT),
    ("ld_w < K", dict(ld_w=128), _hip.ERR_BAD_ARGUMENT),
    ("ld_q < K unpacked", dict(pack_bits=0, ld_q=0), _hip.ERR_BAD_ARGUMENT),
    ("3 bits", dict(W_nbits=3), _hip.ERR_UNSUPPORTED),
    ("16 bits", dict(W_nbits=16), _hip.ERR_UNSUPPORTED),
    ("pack_bits 8", dict(pack_bits=8), _hip.ERR_UNSUPPORTED),
    ("pack_bits 64", dict(pack_bits=64), _hip.ERR_UNSUPPORTED),
    ("int8 input", dict(w_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("fp32 metadata", dict(meta_dtype=FP32), _hip.ERR_UNSUPPORTED),
    ("g % 32", dict(group_size=16), _hip.ERR_BAD_SHAPE),
    ("g % 32, 48", dict(group_size=48, K=96 * 4, ld_w=96 * 4), _hip.ERR_BAD_SHAPE),
    ("K % g", dict(group_size=96), _hip.ERR_BAD_SHAPE),
    ("grid.y limit", dict(group_size=32, K=256 * 65536, ld_w=256 * 65536), _hip.ERR_BAD_SHAPE),
]


@pytest.mark.parametrize("what,override,status", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_validation_refuses_before_any_launch(what, override, status):
    lib = _hip.load()
    assert lib.gemlite_hip_quantize_groups(C.byref(_args(**override)), None) == status


def test_null_args_pointer():
    assert _hip.load().gemlite_hip_quantize_groups(None, None) == _hip.ERR_BAD_ARGUMENT


def test_struct_mirror_matches_the_header_layout():
    # 4 + 4 | 8 | 3 x 8 | 4 x 4 | 8 | 8 | 8 + 8 | 8 + 8 | 4 + 4: no padding anywhere
    assert C.sizeof(_hip.QuantizeArgs) == 112
    assert _hip.QuantizeArgs.q_out.offset == 56 and _hip.QuantizeArgs.fold_zeros.offset == 104


def test_cpu_tensors_fail_loudly():
    W = torch.randn(64, 128, dtype=torch.float16)
    with pytest.raises(_hip.GemliteHipError):
        WeightQuantizerINT(4, 64).quantize(W)
    lin = torch.nn.Linear(128, 64, dtype=torch.float16)
    for proc in (helper.A16W4_RTN_INT(group_size=64), helper.A16W2_RTN_INT(), helper.A16W8_RTN_INT(packing_bitwidth=8),
                 helper.A8W4_RTN_INT_dynamic(group_size=64)):
        with pytest.raises(_hip.GemliteHipError):
            proc.from_linear(lin)
    assert lin.weight is not None  # nothing was cleaned up


def test_only_the_new_classes_quantise():
    hqq = [helper.A16Wn, helper.A16Wn_HQQ_INT, helper.A16W8_HQQ_INT, helper.A16W4_HQQ_INT, helper.A16W2_HQQ_INT, helper.A16W1_HQQ_INT,
           helper.A8Wn_HQQ_INT_dynamic, helper.A8W4_HQQ_INT_dynamic, helper.A8W2_HQQ_INT_dynamic]
    for cls in hqq:
        assert not hasattr(cls, "from_linear") and not hasattr(cls, "quantize_weights"), cls.__name__
    new = {helper.A16Wn_RTN_INT: None, helper.A16W8_RTN_INT: 8, helper.A16W4_RTN_INT: 4, helper.A16W2_RTN_INT: 2, helper.A16W1_RTN_INT: 1,
           helper.A8Wn_RTN_INT_dynamic: None, helper.A8W4_RTN_INT_dynamic: 4, helper.A8W2_RTN_INT_dynamic: 2}
    for cls, bits in new.items():
        for name in ("from_linear", "quantize_weights", "from_hqqlinear", "from_weights"):
            assert hasattr(cls, name), (cls.__name__, name)
        assert cls.W_nbits == bits
    assert issubclass(helper.A16W4_RTN_INT, helper.A16Wn_HQQ_INT) and issubclass(helper.A8W4_RTN_INT_dynamic, helper.A8Wn_HQQ_INT_dynamic)
    p = helper.A16W4_RTN_INT(device="cpu", dtype=torch.bfloat16, packing_bitwidth=8, post_scale=False, group_size=128)
    assert (p.device, p.dtype, p.packing_bitwidth, p.post_scale, p.group_size, p.W_nbits) == ("cpu", torch.bfloat16, 8, False, 128, 4)
    assert helper.A16W4_RTN_INT().group_size is None and helper.A8W2_RTN_INT_dynamic(group_size=32).group_size == 32
    assert helper.A16Wn_RTN_INT(W_nbits=2).W_nbits == 2


def test_group_size_that_does_not_divide_raises_value_error_with_the_name():
    from gemlite_amd.quant_utils import check_group_size
    with pytest.raises(ValueError, match="blocks.3.proj"):
        check_group_size(100, 64, "blocks.3.proj")
    with pytest.raises(ValueError):
        check_group_size(128, 48)
    check_group_size(768, 96)


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("g", [32, 128, 512])
def test_error_bound_of_the_contract(T, nbits, g):
    W = planted_weights(24, 1024, g, T, seed=nbits * 1000 + g)
    q, s_r, z_r = quantize_groups_spec(W, nbits, g, T)
    assert torch.isfinite(z_r).all() and torch.isfinite(s_r).all()
    assert int(q.max()) <= 2 ** nbits - 1
    w = W.float().reshape(24, 1024 // g, g)
    deq = (q.float().reshape(24, 1024 // g, g) - z_r.unsqueeze(-1)) * s_r.unsqueeze(-1)
    bound = error_bound(nbits, s_r, z_r, T).unsqueeze(-1)
    excess = ((deq - w).abs() - bound).max().item()
    print(f"max |err| - bound = {excess:.3e}")
    assert excess <= 0.0
    # the planted degenerate groups: scale 1, every code 0, the group dequantises to lo (rounded to T)
    assert (s_r[0, 0] == 1.0) and (s_r[1, 0] == 1.0) and (q[0, :g] == 0).all() and (q[1, :g] == 0).all()
    assert z_r[1, 0] == 0.0
