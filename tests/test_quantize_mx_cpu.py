"""Host side of the block-scaled weight quantiser (gemlite_hip_quantize_mx, WeightQuantizerMXFP, the MXFP / NVFP processors): the torch
restatement of the contract (tests/quant_mx_spec.py) against the reference's torch quantiser and its recorded results, the C ABI entry and
its validation table (nothing is launched), and the CPU routes, which stay on the torch code."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, helper
from gemlite_amd.quant_utils import WeightQuantizerMXFP
from tests.quant_mx_spec import FORMATS, pack_nibbles, planted_weights_mx, quantize_mx_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z = np.load(os.path.join(ROOT, "tests", "golden", "mx.npz"))
FP32, FP16, BF16, INT8 = 0, 1, 2, 4
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}


def _torch_quantiser(W, fmt):
    wq = WeightQuantizerMXFP(compute_dtype=torch.bfloat16, device="cpu")
    q, s = {"mxfp8": lambda: wq.quantize_mxfp8(W, index=True), "mxfp4": lambda: wq.quantize_mxfp4(W, index=True),
            "nvfp4": lambda: wq.quantize_nvfp4(W, index=True)}[fmt]()
    return q.contiguous().view(torch.uint8).reshape(-1), s.contiguous().view(torch.uint8).reshape(-1)


# ------------------------------------------------------------------------------------------------ spec against the reference
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_spec_equals_the_torch_quantiser_on_finite_inputs(fmt, dt, seed):
    W = planted_weights_mx(96, 512, DTYPES[dt], seed)
    el, sb, bad = quantize_mx_spec(W, fmt)
    assert not bad.any()
    q, s = _torch_quantiser(W, fmt)
    nq, ns = int((q != el.reshape(-1)).sum()), int((s != sb.reshape(-1)).sum())
    print(f"{fmt} {dt} seed {seed}: {nq} element bytes, {ns} scale bytes differ")
    assert nq == 0 and ns == 0


@pytest.mark.parametrize("fmt", list(FORMATS))
def test_spec_equals_the_recorded_reference_results(fmt):
    W = torch.from_numpy(Z["wq_in_W"].copy()).view(torch.bfloat16)
    assert tuple(W.shape) == (48, 256)
    el, sb, bad = quantize_mx_spec(W, fmt)
    assert not bad.any()
    assert np.array_equal(el.numpy().reshape(-1), Z[f"wq_{fmt}_q"].reshape(-1))
    assert np.array_equal(sb.numpy().reshape(-1), Z[f"wq_{fmt}_s"].reshape(-1))


def test_spec_rules_on_hand_made_blocks():
    """the planted edges, stated by hand: midpoints take the lower value, a negative zero result is code 0, the scale is clamped, NaN codes"""
    mid = torch.tensor([6.0, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5, 3.5, -3.5, 5.0, -5.0, -6.0])
    W = torch.cat([mid, mid]).reshape(1, 32)
    want = [7, 0, 0, 1, 9, 2, 10, 3, 11, 4, 12, 5, 13, 6, 14, 15]
    for fmt in ("mxfp4", "nvfp4"):
        el, sb, _ = quantize_mx_spec(W, fmt)
        assert el[0, :16].tolist() == want and el[0, 16:].tolist() == want
        assert sb.reshape(-1).tolist() == ([127] if fmt == "mxfp4" else [0x5A, 0x5A])  # 2^0; e4m3(20) = 1.25 * 2^4
    assert pack_nibbles(torch.tensor([[7, 0, 0, 1]], dtype=torch.uint8)).tolist() == [[0x07, 0x10]]
    big = torch.zeros(1, 32)
    big[0, 0], big[0, 1], big[0, 16] = 3000.0, -3000.0, 1e-12
    el, sb, _ = quantize_mx_spec(big, "nvfp4")
    assert sb.reshape(-1).tolist() == [0x7E, 0x00] and el[0, :2].tolist() == [7, 15]  # 448; |q| > 7 stays 7 / 15
    el, sb, _ = quantize_mx_spec(big, "mxfp4")
    assert sb.reshape(-1).tolist() == [127 + 9]  # 3000 / 6 = 500 -> 2^9
    assert quantize_mx_spec(torch.zeros(1, 32), "mxfp8")[1].tolist() == [[97]]  # floored at 2^-30
    one = torch.zeros(1, 64)
    one[0, 0], one[0, 32] = 448.0 * 4, 448.0 * 4 * (1 + 2.0 ** -23)
    assert quantize_mx_spec(one, "mxfp8")[1].tolist() == [[129, 130]]  # mantissa zero: no + 1; one ulp above: + 1
    nan = torch.zeros(2, 32)
    nan[0, 3], nan[1, 20] = float("nan"), float("-inf")
    for fmt, code in (("mxfp8", 0xFF), ("mxfp4", 0xFF), ("nvfp4", 0x7F)):
        el, sb, bad = quantize_mx_spec(nan, fmt)
        assert sb[bad].tolist() == [code, code] and int(bad.sum()) == 2 and (sb[~bad] != code).all()


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbol_is_declared_exported_and_loaded():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    assert re.search(r"\bint\s+gemlite_hip_quantize_mx\s*\(\s*const\s+gemlite_hip_quantize_mx_args\s*\*", header)
    assert "gemlite_hip_quantize_mx" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "gemlite_hip_quantize_mx")
    assert lib.gemlite_hip_abi_version() == 1 == _hip.ABI_VERSION
    assert b"quantize_mx" in lib.gemlite_hip_build_info()


def test_struct_mirror_matches_the_header_layout():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    body = re.search(r"typedef struct gemlite_hip_quantize_mx_args \{(.*?)\} gemlite_hip_quantize_mx_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("void*", "").replace(
        "void *", "").split(",")]
    assert names == [f[0] for f in _hip.QuantizeMxArgs._fields_]
    # 4 + 4 | 8 | 3 x 8 | 4 + 4 | 8 | 8 | 8 | 8 + 8 | 8: no padding anywhere
    assert C.sizeof(_hip.QuantizeMxArgs) == 96
    assert _hip.QuantizeMxArgs.format.offset == 40 and _hip.QuantizeMxArgs.q_out.offset == 48 and _hip.QuantizeMxArgs.reserved.offset == 88


def _args(**kw):
    a = _hip.QuantizeMxArgs()
    a.struct_size = C.sizeof(_hip.QuantizeMxArgs)
    a.w, a.q_out, a.scales = 0x1000, 0x2000, 0x3000  # never dereferenced: every row below is refused
    a.w_dtype, a.N, a.K, a.ld_w = BF16, 64, 256, 256
    a.format, a.pack_nibbles, a.ld_q = 1, 1, 128
    a.stride_scale_g, a.stride_scale_n = 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


VALIDATION = [
    ("null w", dict(w=None), _hip.ERR_BAD_ARGUMENT),
    ("null q_out", dict(q_out=None), _hip.ERR_BAD_ARGUMENT),
    ("null scales", dict(scales=None), _hip.ERR_BAD_ARGUMENT),
    ("struct_size", dict(struct_size=C.sizeof(_hip.QuantizeMxArgs) - 8), _hip.ERR_BAD_ARGUMENT),
    ("struct_size 0", dict(struct_size=0), _hip.ERR_BAD_ARGUMENT),
    ("N = 0", dict(N=0), _hip.ERR_BAD_ARGUMENT),
    ("N < 0", dict(N=-64), _hip.ERR_BAD_ARGUMENT),
    ("K = 0", dict(K=0), _hip.ERR_BAD_ARGUMENT),
    ("K < 0", dict(K=-256), _hip.ERR_BAD_ARGUMENT),
    ("ld_w < K", dict(ld_w=255), _hip.ERR_BAD_ARGUMENT),
    ("ld_q < K/2 packed", dict(ld_q=127), _hip.ERR_BAD_ARGUMENT),
    ("ld_q < K unpacked", dict(pack_nibbles=0, ld_q=255), _hip.ERR_BAD_ARGUMENT),
    ("ld_q < K fp8", dict(format=0, pack_nibbles=0, ld_q=128), _hip.ERR_BAD_ARGUMENT),
    ("format 3", dict(format=3), _hip.ERR_UNSUPPORTED),
    ("format -1", dict(format=-1), _hip.ERR_UNSUPPORTED),
    ("int8 input", dict(w_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("fp8 input", dict(w_dtype=11), _hip.ERR_UNSUPPORTED),
    ("pack_nibbles with mxfp8", dict(format=0, ld_q=256), _hip.ERR_UNSUPPORTED),
    ("pack_nibbles 2", dict(pack_nibbles=2), _hip.ERR_UNSUPPORTED),
    ("K % 32", dict(K=48, ld_w=48), _hip.ERR_BAD_SHAPE),
    ("K % 32, nvfp4 block of 16", dict(format=2, K=16, ld_w=16), _hip.ERR_BAD_SHAPE),
    ("grid.y limit", dict(K=256 * 65536, ld_w=256 * 65536, ld_q=128 * 65536), _hip.ERR_BAD_SHAPE),
]


@pytest.mark.parametrize("what,override,status", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_validation_refuses_before_any_launch(what, override, status):
    assert _hip.load().gemlite_hip_quantize_mx(C.byref(_args(**override)), None) == status


def test_null_args_pointer():
    assert _hip.load().gemlite_hip_quantize_mx(None, None) == _hip.ERR_BAD_ARGUMENT


# ------------------------------------------------------------------------------------------------ CPU routes stay on the torch code
PROCS = {
    "a16w8_mxfp": lambda: helper.A16W8_MXFP(device="cpu", dtype=torch.bfloat16),
    "a16w4_mxfp": lambda: helper.A16W4_MXFP(device="cpu", dtype=torch.float16),
    "a8w8_mxfp_dyn_post": lambda: helper.A8W8_MXFP_dynamic(device="cpu", dtype=torch.bfloat16, post_scale=True),
    "a8w8_mxfp_dyn_micro": lambda: helper.A8W8_MXFP_dynamic(device="cpu", dtype=torch.bfloat16, post_scale=False),
    "a8w4_mxfp_dyn": lambda: helper.A8W4_MXFP_dynamic(device="cpu", dtype=torch.bfloat16, post_scale=False),
    "a4w4_mxfp_dyn": lambda: helper.A4W4_MXFP_dynamic(device="cpu", dtype=torch.bfloat16),
    "a4w4_nvfp_dyn": lambda: helper.A4W4_NVFP_dynamic(device="cpu", dtype=torch.float16),
}


@pytest.mark.parametrize("name", list(PROCS))
def test_cpu_from_linear_is_the_torch_path_with_unchanged_results(name):
    proc = PROCS[name]()
    W = planted_weights_mx(48, 256, torch.bfloat16, seed=5)
    lin = torch.nn.Linear(256, 48, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(W)
    assert not proc._fused(lin.weight.data)
    layer = proc.from_linear(lin, del_orig=False)
    fmt = proc._format()
    el, sb, _ = quantize_mx_spec(W, fmt)
    assert layer.W_q.device.type == "cpu" and lin.weight is not None
    want_q = el if fmt == "mxfp8" else pack_nibbles(el)
    assert torch.equal(layer.W_q.data.view(torch.uint8).t(), want_q)
    assert torch.equal(layer.scales.data.view(torch.uint8), sb)
    assert layer.scales.dtype == (torch.float8_e4m3fn if fmt == "nvfp4" else torch.uint8)
    assert list(layer.state_dict().keys()) == ["W_q", "bias", "scales", "zeros", "metadata", "orig_shape"]


def test_cpu_tensors_and_other_arguments_never_reach_the_kernel():
    from gemlite_amd.quant_utils import _takes_mx_kernel
    W = torch.randn(8, 64, dtype=torch.bfloat16)
    assert not _takes_mx_kernel(W, True)
    wq = WeightQuantizerMXFP(device="cpu")
    q, s = wq.quantize_mxfp4(W, index=True)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (16, 32) and s.dtype == torch.float8_e8m0fnu and tuple(s.shape) == (16, 1)
    q, s = wq.quantize_mxfp8(W, index=True)
    assert q.dtype == torch.float8_e4m3fn and tuple(q.shape) == (16, 32) and s.dtype == torch.float8_e8m0fnu
    q, s = wq.quantize_nvfp4(W, index=True)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (32, 16) and s.dtype == torch.float8_e4m3fn and tuple(s.shape) == (32, 1)
    with pytest.raises(_hip.GemliteHipError):
        wq.quantize_packed(W, "mxfp4")
    with pytest.raises(_hip.GemliteHipError):
        helper.A4W4_MXFP_dynamic(dtype=torch.bfloat16).quantize_weights(W)
