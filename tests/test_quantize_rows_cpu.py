"""Host side of the channel-wise 8-bit weight quantiser (gemlite_hip_quantize_rows, WeightQuantizerRows, the A16W8 / A8W8 processors): the
torch restatement of the contract (tests/quant_rows_spec.py) against the torch sequence the processors ran and the layers they build on
the CPU, the rules by hand, the C ABI entry and its validation table (nothing is launched), and the CPU routes, which stay on torch."""
import ctypes as C
import os
import re

import pytest
import torch

from gemlite_amd import _hip, helper, quant_utils
from gemlite_amd.quant_utils import WeightQuantizerRows, _quantize_rows_torch, _takes_rows_kernel
from tests.quant_rows_spec import FORMATS, RULE_DIFFERS, planted_weights_rows, quantize_rows_spec, row_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16, BF16, INT8 = 0, 1, 2, 4
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
STATE_KEYS = ["W_q", "bias", "scales", "zeros", "metadata", "orig_shape"]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _processors(fmt, dtype, device="cpu"):
    """the A16W8 and the A8W8 processor of a code format, with the fp16 / bf16 compute type a weight of `dtype` gets"""
    qdt = FORMATS[fmt][1]
    cdt = dtype if dtype != torch.float32 else torch.float16
    return (helper.A16W8(device=device, dtype=cdt, fp8=None if fmt == "int8" else qdt),
            helper.A8W8_dynamic(device=device, dtype=cdt, fp8=False if fmt == "int8" else qdt))


# ------------------------------------------------------------------------------------------------ C1: spec against the torch sequence
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("fmt", list(FORMATS))
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_spec_rule0_equals_the_torch_sequence_and_the_cpu_layers(fmt, dt, seed):
    N, K = 40, 160
    W = planted_weights_rows(N, K, DTYPES[dt], seed)
    codes, s = quantize_rows_spec(W, fmt, 0)
    W_q, scales = _quantize_rows_torch(W, FORMATS[fmt][1])
    assert W_q.dtype == FORMATS[fmt][1] and scales.dtype == torch.float32 and tuple(scales.shape) == (N, 1)
    nq, ns = int((_bits(W_q) != codes).sum()), int((_bits(scales) != _bits(s)).sum())
    print(f"{fmt} {dt} seed {seed}: {nq} codes, {ns} scales differ")
    assert nq == 0 and ns == 0
    for proc in _processors(fmt, DTYPES[dt]):
        layer = proc.from_weights(W)
        assert layer.W_q.device.type == "cpu" and tuple(layer.W_q.shape) == (K, N) and tuple(layer.scales.shape) == (1, N)
        assert torch.equal(_bits(layer.W_q.data.t()), codes) and torch.equal(_bits(layer.scales.data.view(N, 1)), _bits(s))


# ------------------------------------------------------------------------------------------------ C2: the rules by hand
def test_spec_rules_on_hand_made_rows():
    i8 = lambda W, rule=0: quantize_rows_spec(torch.tensor(W), "int8", rule)[0].view(torch.int8).tolist()  # noqa: E731
    f8 = lambda W, fmt: quantize_rows_spec(torch.tensor(W), fmt, 0)[0].tolist()  # noqa: E731
    # ties go to the even integer; amax = qmax gives s = 1 under rule 0
    assert i8([[127, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5]]) == [[127, 0, 0, 2, -2, 2, -2]]
    # a negative amax is -127, never -128, under both rules; an all-zero row is all zero
    assert i8([[-5.0, 2.5]]) == [[-127, 64]] and i8([[-5.0, 2.5]], 1) == [[-127, 64]] and i8([[0.0, -0.0]]) == [[0, 0]]
    # the floor: amax / 127 < 1e-6, s is the fp32 nearest to 1e-6 and the data under it still resolves
    codes, s = quantize_rows_spec(torch.tensor([[2.0 ** -14, -2.0 ** -15]]), "int8", 0)
    assert _bits(s).tolist() == [[0x358637BD]] and codes.view(torch.int8).tolist() == [[61, -31]]
    assert _bits(quantize_rows_spec(torch.zeros(1, 3), "e4m3", 1)[1]).tolist() == [[0x358637BD]]
    # e4m3: 448 | 17 -> 16 | 19 -> 20 | 2^-10 -> 0 | 3 * 2^-10 -> 2^-8 (subnormal kept) | -0 keeps its sign | 0 | -17 -> -16 | 1.0625 -> 1 | 1.1875 -> 1.25
    assert f8([[448, 17, 19, 2.0 ** -10, 3 * 2.0 ** -10, -0.0, 0.0, -17, 1.0625, 1.1875]], "e4m3") == [
        [0x7E, 0x58, 0x5A, 0x00, 0x02, 0x80, 0x00, 0xD8, 0x38, 0x3A]]
    # e5m2: 57344 | -0 | 4.5 -> 4 | 5.5 -> 6 | 9 -> 8 | 11 -> 12 | 2^-17 -> 0 | 3 * 2^-17 -> 2^-15
    assert f8([[57344, -0.0, 4.5, 5.5, 9, 11, 2.0 ** -17, 3 * 2.0 ** -17]], "e5m2") == [[0x7B, 0x80, 0x44, 0x46, 0x48, 0x4A, 0x00, 0x02]]
    # the two scale rules differ in the last bit: pinned per format
    pinned = {"int8": (0x3C102041, 0x3C102040), "e4m3": (0x3B5B6DB7, 0x3B5B6DB8), "e5m2": (0x37949249, 0x3794924A)}
    for fmt, (r0, r1) in pinned.items():
        a = torch.tensor([[RULE_DIFFERS[fmt], 0.25]])
        assert _bits(quantize_rows_spec(a, fmt, 0)[1]).item() == r0 and _bits(quantize_rows_spec(a, fmt, 1)[1]).item() == r1
    assert RULE_DIFFERS == {"int8": 1.1171875, "e4m3": 1.5, "e5m2": 1.015625}
    # the scale is rounded once to a 16-bit type; the codes come from the fp32 scale
    W = torch.tensor([[3.0, 1.0, -2.0]])
    codes16, s16 = quantize_rows_spec(W, "int8", 0, torch.bfloat16)
    codes32, s32 = quantize_rows_spec(W, "int8", 0)
    assert s16.dtype == torch.bfloat16 and torch.equal(s16, s32.to(torch.bfloat16)) and torch.equal(codes16, codes32)
    # a non-finite row: a non-finite scale, and no other row notices
    W = torch.tensor([[1.0, float("nan")], [float("-inf"), 2.0], [3.0, -1.5]])
    s = quantize_rows_spec(W, "int8", 1)[1]
    assert torch.isnan(s[0]).all() and torch.isinf(s[1]).all() and torch.equal(s[2], row_scale(torch.tensor([3.0]), "int8", 1))


# ------------------------------------------------------------------------------------------------ C3: C ABI
def test_symbol_is_declared_exported_and_loaded():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    assert re.search(r"\bint\s+gemlite_hip_quantize_rows\s*\(\s*const\s+gemlite_hip_quantize_rows_args\s*\*", header)
    assert "gemlite_hip_quantize_rows" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "gemlite_hip_quantize_rows")
    assert lib.gemlite_hip_abi_version() == 1 == _hip.ABI_VERSION
    assert b"quantize_rows" in lib.gemlite_hip_build_info()
    limits = dict(re.findall(r"#define (GEMLITE_QUANT_ROWS_\w+_MAX_K) (\d+)", header))
    assert int(limits["GEMLITE_QUANT_ROWS_WAVE_MAX_K"]) == _hip.QUANT_ROWS_WAVE_MAX_K
    assert int(limits["GEMLITE_QUANT_ROWS_RESIDENT_MAX_K"]) == _hip.QUANT_ROWS_RESIDENT_MAX_K > _hip.QUANT_ROWS_WAVE_MAX_K


def test_struct_mirror_matches_the_header_layout():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    body = re.search(r"typedef struct gemlite_hip_quantize_rows_args \{(.*?)\} gemlite_hip_quantize_rows_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("void*", "").replace(
        "void *", "").split(",")]
    assert names == [f[0] for f in _hip.QuantizeRowsArgs._fields_]
    # 4 + 4 | 8 | 3 x 8 | 4 + 4 | 8 | 8 | 8 | 8 | 4 + 4: no padding anywhere
    assert C.sizeof(_hip.QuantizeRowsArgs) == 88
    assert _hip.QuantizeRowsArgs.format.offset == 40 and _hip.QuantizeRowsArgs.q_out.offset == 48 and _hip.QuantizeRowsArgs.scale_dtype.offset == 80


def _args(**kw):
    a = _hip.QuantizeRowsArgs()
    a.struct_size = C.sizeof(_hip.QuantizeRowsArgs)
    a.w, a.q_out, a.scales = 0x1000, 0x2000, 0x3000  # never dereferenced: every row below is refused
    a.w_dtype, a.N, a.K, a.ld_w = BF16, 64, 256, 256
    a.format, a.scale_rule, a.ld_q = 0, 1, 256
    a.scale_dtype, a.stride_s = FP32, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


VALIDATION = [
    ("null w", dict(w=None), _hip.ERR_BAD_ARGUMENT),
    ("null q_out", dict(q_out=None), _hip.ERR_BAD_ARGUMENT),
    ("null scales", dict(scales=None), _hip.ERR_BAD_ARGUMENT),
    ("struct_size", dict(struct_size=C.sizeof(_hip.QuantizeRowsArgs) - 8), _hip.ERR_BAD_ARGUMENT),
    ("struct_size 0", dict(struct_size=0), _hip.ERR_BAD_ARGUMENT),
    ("N = 0", dict(N=0), _hip.ERR_BAD_ARGUMENT),
    ("N < 0", dict(N=-64), _hip.ERR_BAD_ARGUMENT),
    ("K = 0", dict(K=0), _hip.ERR_BAD_ARGUMENT),
    ("K < 0", dict(K=-256), _hip.ERR_BAD_ARGUMENT),
    ("ld_w < K", dict(ld_w=255), _hip.ERR_BAD_ARGUMENT),
    ("ld_q < K", dict(ld_q=255), _hip.ERR_BAD_ARGUMENT),
    ("stride_s = 0", dict(stride_s=0), _hip.ERR_BAD_ARGUMENT),
    ("stride_s < 0", dict(stride_s=-1), _hip.ERR_BAD_ARGUMENT),
    ("format 3", dict(format=3), _hip.ERR_UNSUPPORTED),
    ("format -1", dict(format=-1), _hip.ERR_UNSUPPORTED),
    ("scale_rule 2", dict(scale_rule=2), _hip.ERR_UNSUPPORTED),
    ("scale_rule -1", dict(scale_rule=-1), _hip.ERR_UNSUPPORTED),
    ("int8 input", dict(w_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("fp8 input", dict(w_dtype=11), _hip.ERR_UNSUPPORTED),
    ("int8 scales", dict(scale_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("grid limit, resident form", dict(N=1 << 31), _hip.ERR_BAD_SHAPE),
    ("grid limit, wave form", dict(N=1 << 31, K=64, ld_w=64, ld_q=64), _hip.ERR_BAD_SHAPE),
]


@pytest.mark.parametrize("what,override,status", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_validation_refuses_before_any_launch(what, override, status):
    assert _hip.load().gemlite_hip_quantize_rows(C.byref(_args(**override)), None) == status


def test_null_args_pointer():
    assert _hip.load().gemlite_hip_quantize_rows(None, None) == _hip.ERR_BAD_ARGUMENT


# ------------------------------------------------------------------------------------------------ C4: CPU routes stay on torch
PROCS = {
    "A16W8": lambda: helper.A16W8(device="cpu"),
    "A16W8_INT8": lambda: helper.A16W8_INT8(device="cpu", post_scale=True),
    "A16W8_FP8": lambda: helper.A16W8_FP8(device="cpu"),
    "A8W8_dynamic": lambda: helper.A8W8_dynamic(device="cpu", fp32_scale=False),
    "A8W8_int8_dynamic": lambda: helper.A8W8_int8_dynamic(device="cpu"),
    "A8W8_fp8_dynamic": lambda: helper.A8W8_fp8_dynamic(device="cpu"),
}


@pytest.mark.parametrize("name", list(PROCS))
def test_cpu_processors_never_reach_the_kernel(name, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a CPU layer reached gemlite_hip_quantize_rows")

    monkeypatch.setattr(quant_utils, "_quantize_rows", refuse)
    W = planted_weights_rows(24, 96, torch.bfloat16, seed=5)
    lin = torch.nn.Linear(96, 24, bias=True, dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(W)
    proc = PROCS[name]()
    layer = proc.from_linear(lin, del_orig=False)
    assert lin.weight is not None and lin.bias is not None
    fmt = "e4m3" if "FP8" in name or "fp8" in name else "int8"
    codes, s = quantize_rows_spec(W, fmt, 0)
    assert layer.W_q.device.type == "cpu" and torch.equal(_bits(layer.W_q.data.t()), codes)
    want_s = s.to(torch.bfloat16) if name == "A8W8_dynamic" else s
    assert layer.scales.dtype == want_s.dtype and torch.equal(_bits(layer.scales.data.view(-1, 1)), _bits(want_s))
    assert list(layer.state_dict().keys()) == STATE_KEYS
    assert (layer.W_group_mode, layer.channel_scale_mode) == {"A16W8": (2, 0), "A16W8_INT8": (0, 1), "A16W8_FP8": (2, 0)}.get(name, (0, 3))
    proc.from_linear(lin)  # del_orig defaults to True, as in the reference
    assert lin.weight is None and lin.bias is None


def test_inputs_the_kernel_does_not_take_and_the_cpu_quantiser(monkeypatch):
    W = torch.randn(8, 64, dtype=torch.bfloat16)
    assert not _takes_rows_kernel(W, torch.int8, "cpu")
    assert _takes_rows_kernel(W, torch.int8, "cuda:0") and _takes_rows_kernel(W.float(), torch.float8_e5m2, torch.device("cuda", 0))
    assert not _takes_rows_kernel(W, torch.float8_e4m3fnuz, "cuda:0") and not _takes_rows_kernel(W, torch.float8_e5m2fnuz, "cuda:0")
    assert not _takes_rows_kernel(W.t(), torch.int8, "cuda:0") and not _takes_rows_kernel(W.view(2, 4, 64), torch.int8, "cuda:0")
    assert not _takes_rows_kernel(W.double(), torch.int8, "cuda:0") and not _takes_rows_kernel(W[:0], torch.int8, "cuda:0")
    assert _takes_rows_kernel(W[:, 3:40], torch.int8, "cuda:0")  # a view with unit inner stride

    def refuse(*a, **k):
        raise AssertionError("a CPU tensor reached gemlite_hip_quantize_rows")

    monkeypatch.setattr(quant_utils, "_quantize_rows", refuse)
    for fmt, (_, qdt, _, _) in FORMATS.items():
        q, s = WeightQuantizerRows(qdt, device="cpu").quantize(W)
        codes, want = quantize_rows_spec(W, fmt, 0)
        assert q.dtype == qdt and tuple(q.shape) == (8, 64) and s.dtype == torch.float32 and tuple(s.shape) == (8, 1)
        assert torch.equal(_bits(q), codes) and torch.equal(_bits(s), _bits(want))
    q, s = WeightQuantizerRows(torch.int8, device="cpu", fp32_scale=False).quantize(W)
    assert s.dtype == torch.bfloat16 and torch.equal(s, quantize_rows_spec(W, "int8", 0, torch.bfloat16)[1])
    assert WeightQuantizerRows(torch.int8).scale_rule == quant_utils.ROWS_SCALE_RULE and WeightQuantizerRows(torch.int8, scale_rule=0).scale_rule == 0
    with pytest.raises(_hip.GemliteHipError):
        WeightQuantizerRows(torch.int8, device="cpu").dequantize(q, s)
