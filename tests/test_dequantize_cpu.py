"""Host side of the weight dequantiser (gemlite_hip_dequantize, GemLiteLinear.dequantize, the quantisers' dequantize): the torch
restatement of the contract (tests/dequant_spec.py) against the float64 oracles, the C ABI entry and its validation table (nothing is
launched), and the CPU routes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, helper
from gemlite_amd.quant_utils import WeightQuantizerMXFP
from oracle import gemlite_oracle as orc
from oracle import mx_oracle as mxo
from tests import dequant_spec as ds
from tests.quant_int_spec import error_bound, planted_weights, quantize_groups_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16, BF16, FP8E4, INT8, UINT8, INT32 = 0, 1, 2, 3, 4, 5, 6
MXFP8, MXFP4, NVFP4 = 16, 17, 18
U24 = 2.0 ** -24


def _meta(gen, shape, T, lo=-6, hi=6, signed=False):
    """values of T with magnitudes 2^lo .. 2^hi (inside the [2^-20, 2^20] the restatement's exactness assertion covers)"""
    v = torch.exp2(torch.rand(shape, generator=gen) * (hi - lo) + lo)
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=gen) * 2 - 1)
    return v.to(T)


# ------------------------------------------------------------------------------------------------ spec against the float64 oracles
CASES = [(m, zk) for m in (0, 2) for zk in ("none",)] + [(m, zk) for m in (1, 3) for zk in ("scalar", "tensor")] + [(4, "tensor")]


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("w_mode,zeros_kind", CASES)
@pytest.mark.parametrize("chan", [False, True], ids=["", "chan"])
def test_spec_agrees_with_the_float64_oracle(w_mode, zeros_kind, nbits, T, chan):
    N, K, g = 24, 128, 32
    gen = torch.Generator().manual_seed(100 * w_mode + nbits)
    q = torch.randint(0, 2 ** nbits, (N, K), generator=gen).float()
    s = _meta(gen, (K // g, N), T)
    if zeros_kind == "scalar":
        z = torch.tensor([[2 ** (nbits - 1)]], dtype=torch.int32)
    else:
        z = _meta(gen, (K // g, N), T, lo=-4, hi=nbits, signed=w_mode == 4)
    c = _meta(gen, (N,), torch.float32, lo=-8, hi=2) if chan else None
    need_s, need_z = w_mode >= 2, w_mode in (1, 3, 4)
    sN = ds.expand_groups(s, g, K) if need_s else None
    zN = (z.float().reshape(1, 1) if zeros_kind == "scalar" else ds.expand_groups(z, g, K)) if need_z else None
    got = ds.dequant_int_spec(q, sN, zN, c, w_mode, torch.float32).double().numpy()
    want = orc.dequantize(q.t().numpy(), orc.to_f64(s) if need_s else None,
                          (orc.to_f64(z).reshape(-1) if zeros_kind == "scalar" else orc.to_f64(z)) if need_z else None, g, w_mode,
                          zero_is_scalar=zeros_kind == "scalar", meta_code=None).T
    aq = q.double().numpy()
    a_s = sN.double().numpy() if need_s else 1.0
    az = np.abs(zN.double().numpy()) if need_z else 0.0
    ac = np.abs(c.double().numpy()).reshape(-1, 1) if chan else 1.0
    if chan:
        want = want * c.double().numpy().reshape(-1, 1)
    # at most three fp32 roundings, each relative to the magnitudes of its own operands
    bound = 3 * U24 * ((np.abs(aq * a_s) + az) * ac if w_mode == 4 else (aq + az) * np.abs(a_s) * ac)
    err = np.abs(got - want)
    print(f"mode {w_mode} {zeros_kind} {nbits}-bit {T}: max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert np.all(err <= bound)


@pytest.mark.parametrize("fmt", ["mxfp8", "mxfp4", "nvfp4"])
def test_spec_agrees_with_the_block_oracle(fmt):
    N, K = 16, 128
    g = 16 if fmt == "nvfp4" else 32
    gen = torch.Generator().manual_seed(7)
    if fmt == "mxfp8":
        byt = torch.randint(0, 256, (N, K), generator=gen).to(torch.uint8)
        byt[(byt & 0x7F) == 0x7F] = 0x3A  # keep the elements finite
        elem = byt.view(torch.float8_e4m3fn).float()
        assert np.array_equal(elem.numpy(), mxo.fp8_e4m3_decode(byt.numpy()))
    else:
        codes = torch.randint(0, 16, (N, K), generator=gen)
        elem = ds.E2M1[codes]
        assert np.array_equal(elem.numpy(), mxo.FP4_VALUES[codes.numpy()])
    if fmt == "nvfp4":
        sb = torch.randint(0x08, 0x7F, (N, K // g), generator=gen).to(torch.uint8)
    else:
        sb = torch.randint(97, 160, (N, K // g), generator=gen).to(torch.uint8)
    want = mxo.dequant_blocks(elem.numpy(), sb.numpy(), g, e4m3_scales=fmt == "nvfp4")
    got = ds.dequant_mx_spec(elem, sb, g, fmt == "nvfp4", torch.float32).double().numpy()
    assert np.array_equal(got, want)  # a power-of-two scale, or an 11-bit product: exact
    if fmt == "nvfp4":  # the layer's second-level scale: one rounding
        got = ds.dequant_mx_spec(elem, sb, g, True, torch.float32, post_scale=0.05).double().numpy()
        want = want * float(np.float32(0.05))
        assert np.all(np.abs(got - want) <= U24 * np.abs(want))


@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
def test_quantise_then_dequantise_meets_the_quantisers_bound(nbits, T):
    N, K, g = 16, 256, 64
    W = planted_weights(N, K, g, torch.float32, seed=nbits)
    q, s_r, z_r = quantize_groups_spec(W, nbits, g, T)
    back = ds.dequant_int_spec(q.float(), s_r.repeat_interleave(g, dim=1), z_r.repeat_interleave(g, dim=1), None, 3, torch.float32)
    bound = error_bound(nbits, s_r, z_r, T).repeat_interleave(g, dim=1)
    assert torch.all((back - W).abs() <= bound)


def test_folded_zero_is_one_rounding():
    """fp32 metadata: 3 * 0.1f needs 26 bits.  The fma rounds 3 * 0.1f - 0.3f once (a tiny negative number), two steps give exactly 0."""
    q = torch.tensor([[3.0, 1.0]])
    s = torch.tensor([[0.1, 0.1]], dtype=torch.float32)
    z = -torch.tensor([[0.3, 0.3]], dtype=torch.float32)
    fma = ds.dequant_int_spec(q, s, z, None, 4, torch.float32)
    two = q * s + z
    assert two[0, 0].item() == 0.0 and fma[0, 0].item() != 0.0 and abs(fma[0, 0].item()) < 2.0 ** -25
    assert fma[0, 0].item() == float(np.float32(3.0 * float(np.float32(0.1)) - float(np.float32(0.3))))
    assert fma[0, 1].item() == two[0, 1].item()  # 1 * s is exact: no difference there
    with pytest.raises(AssertionError):  # the exactness assertion is live: 2^60 + 1 is not a float64
        ds.fma_once(torch.tensor([1.0]), torch.tensor([2.0 ** 60]), torch.tensor([1.0]))


def test_non_finite_scales_and_overflow():
    elem = ds.E2M1[torch.arange(16)].repeat(2, 2)  # [2, 32]
    sb = torch.tensor([[0xFF], [127]], dtype=torch.uint8)
    out = ds.dequant_mx_spec(elem, sb, 32, False, torch.float16)
    assert torch.isnan(out[0]).all() and torch.equal(out[1].float(), elem[1])  # 0xFF: NaN even for the zero elements
    sb = torch.tensor([[0x7F, 0x38], [0x38, 0xFF]], dtype=torch.uint8)  # e4m3 NaN codes next to 1.0
    out = ds.dequant_mx_spec(elem, sb, 16, True, torch.float32, post_scale=0.05)
    assert torch.isnan(out[0, :16]).all() and torch.isnan(out[1, 16:]).all()
    assert torch.equal(out[0, 16:], elem[0, 16:] * torch.tensor(0.05)) and torch.equal(out[1, :16], elem[1, :16] * torch.tensor(0.05))
    q = torch.tensor([[0.0, 15.0, 1.0, 7.0]])
    s = torch.tensor([[float("nan"), 8192.0, float("inf"), 9359.0]])
    out = ds.dequant_int_spec(q, s, None, None, 2, torch.float16)
    assert torch.isnan(out[0, 0]) and out[0, 1].item() == float("inf") and out[0, 2].item() == float("inf")
    assert out[0, 3].item() == 65504.0  # 65513 is below the midpoint 65520: the largest fp16; 15 * 8192 = 122880 overflows
    assert ds.dequant_int_spec(q, s, None, None, 2, torch.bfloat16)[0, 1].item() == 122880.0


def test_spec_unpacks_like_the_oracle():
    gen = torch.Generator().manual_seed(3)
    for nbits in (8, 4, 2, 1):
        for bits, tdt in ((32, torch.int32), (16, torch.int16), (8, torch.uint8)):
            q = torch.randint(0, 2 ** nbits, (8, 64), generator=gen).to(torch.uint8)
            packed = torch.from_numpy(orc.pack_over_cols(q.numpy(), nbits, bits)).view(tdt)
            assert torch.equal(ds.unpack_words(packed, nbits), q.to(torch.int64))


# ------------------------------------------------------------------------------------------------ C ABI
def test_symbol_is_declared_exported_and_loaded():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    assert re.search(r"\bint\s+gemlite_hip_dequantize\s*\(\s*const\s+gemlite_hip_dequantize_args\s*\*", header)
    assert "gemlite_hip_dequantize" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "gemlite_hip_dequantize")
    assert lib.gemlite_hip_abi_version() == 1 == _hip.ABI_VERSION
    assert b"dequantize" in lib.gemlite_hip_build_info()


def test_struct_mirror_matches_the_header_layout():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    body = re.search(r"typedef struct gemlite_hip_dequantize_args \{(.*?)\} gemlite_hip_dequantize_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip(" *") for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].replace("void*", "").replace(
        "void *", "").split(",")]
    A = _hip.DequantizeArgs
    assert names == [f[0] for f in A._fields_]
    # 4 + 4 | 4 x 8 | 2 x 8 | 5 x 8 | 11 x 4 + 4 | 8: no padding anywhere
    assert C.sizeof(A) == 152
    assert A.w_q.offset == 8 and A.N.offset == 40 and A.ld_out.offset == 88 and A.W_nbits.offset == 96
    assert A.post_scale.offset == 140 and A.reserved.offset == 144
    fwd = dict(_hip.ForwardArgs._fields_)
    for name, ctype in A._fields_:  # the weight fields are the forward struct's, by name and type: Python fills both from one layer
        if name in fwd and name not in ("struct_size", "out"):
            assert fwd[name] is ctype, name


def _args(**kw):
    a = _hip.DequantizeArgs()
    a.struct_size = C.sizeof(_hip.DequantizeArgs)
    a.w_q, a.scales, a.zeros, a.out = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every row below is refused
    a.N, a.K, a.ld_out, a.out_dtype = 64, 256, 256, FP16
    a.W_nbits, a.group_size, a.elements_per_sample, a.w_pack_bits, a.w_dtype = 4, 64, 8, 32, INT32
    a.input_dtype, a.meta_dtype, a.zeros_dtype, a.zero_is_scalar = FP16, FP16, FP16, 0
    a.W_group_mode, a.channel_scale_mode, a.post_scale = 3, 0, 1.0
    a.stride_wk, a.stride_wn, a.stride_meta_g, a.stride_meta_n = 64, 1, 64, 1
    for k, v in kw.items():
        setattr(a, k, v)
    return a


_MX8 = dict(input_dtype=MXFP8, W_nbits=8, elements_per_sample=1, w_pack_bits=0, w_dtype=FP8E4, group_size=32, stride_wk=1, stride_wn=256,
            meta_dtype=UINT8)
_MX4 = dict(input_dtype=MXFP4, W_nbits=4, elements_per_sample=2, w_pack_bits=8, w_dtype=UINT8, group_size=32, stride_wk=1, stride_wn=128,
            meta_dtype=UINT8)
_U8 = dict(W_nbits=8, elements_per_sample=1, w_pack_bits=0, stride_wk=1, stride_wn=256)

VALIDATION = [
    ("null w_q", dict(w_q=None), _hip.ERR_BAD_ARGUMENT),
    ("null out", dict(out=None), _hip.ERR_BAD_ARGUMENT),
    ("struct_size", dict(struct_size=C.sizeof(_hip.DequantizeArgs) - 8), _hip.ERR_BAD_ARGUMENT),
    ("struct_size 0", dict(struct_size=0), _hip.ERR_BAD_ARGUMENT),
    ("N = 0", dict(N=0), _hip.ERR_BAD_ARGUMENT),
    ("N < 0", dict(N=-64), _hip.ERR_BAD_ARGUMENT),
    ("K = 0", dict(K=0), _hip.ERR_BAD_ARGUMENT),
    ("K < 0", dict(K=-256), _hip.ERR_BAD_ARGUMENT),
    ("group_size 0", dict(group_size=0), _hip.ERR_BAD_ARGUMENT),
    ("elements_per_sample 0", dict(elements_per_sample=0), _hip.ERR_BAD_ARGUMENT),
    ("ld_out < K", dict(ld_out=255), _hip.ERR_BAD_ARGUMENT),
    ("mode 3 without scales", dict(scales=None), _hip.ERR_BAD_ARGUMENT),
    ("mode 3 without zeros", dict(zeros=None), _hip.ERR_BAD_ARGUMENT),
    ("mode 4 without zeros", dict(W_group_mode=4, zeros=None), _hip.ERR_BAD_ARGUMENT),
    ("mode 1 without zeros", dict(W_group_mode=1, zeros=None, scales=None), _hip.ERR_BAD_ARGUMENT),
    ("channel scale without scales", dict(W_group_mode=0, channel_scale_mode=1, scales=None, zeros=None), _hip.ERR_BAD_ARGUMENT),
    ("block-scaled without scales", dict(_MX8, scales=None), _hip.ERR_BAD_ARGUMENT),
    ("words that do not hold e codes", dict(elements_per_sample=4), _hip.ERR_BAD_ARGUMENT),
    ("24-bit words", dict(w_pack_bits=24, elements_per_sample=6), _hip.ERR_BAD_ARGUMENT),
    ("int8 result", dict(out_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("fp8 result", dict(out_dtype=FP8E4), _hip.ERR_UNSUPPORTED),
    ("3-bit codes", dict(W_nbits=3, elements_per_sample=10), _hip.ERR_UNSUPPORTED),
    ("W_group_mode 5", dict(W_group_mode=5), _hip.ERR_UNSUPPORTED),
    ("W_group_mode -1", dict(W_group_mode=-1), _hip.ERR_UNSUPPORTED),
    ("channel_scale_mode 4 on an integer layer", dict(channel_scale_mode=4), _hip.ERR_UNSUPPORTED),
    ("64-bit words", dict(w_pack_bits=64, elements_per_sample=16), _hip.ERR_UNSUPPORTED),
    ("e4m3fnuz elements", dict(_U8, w_dtype=12, W_group_mode=0), _hip.ERR_UNSUPPORTED),
    ("e5m2fnuz elements", dict(_U8, w_dtype=13, W_group_mode=0), _hip.ERR_UNSUPPORTED),
    ("int64 elements", dict(_U8, w_dtype=11, W_group_mode=0), _hip.ERR_UNSUPPORTED),
    ("int8 scales", dict(meta_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("int8 tensor zeros", dict(zeros_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("mxfp8 with groups of 64", dict(_MX8, group_size=64), _hip.ERR_UNSUPPORTED),
    ("mxfp8 with e5m2 elements", dict(_MX8, w_dtype=8), _hip.ERR_UNSUPPORTED),
    ("fp8 weights under MXFP4 activations", dict(_MX8, input_dtype=MXFP4), _hip.ERR_UNSUPPORTED),
    ("fp8 weights under NVFP4", dict(_MX8, input_dtype=NVFP4, group_size=16), _hip.ERR_UNSUPPORTED),
    ("nvfp4 with groups of 32", dict(_MX4, input_dtype=NVFP4), _hip.ERR_UNSUPPORTED),
    ("fp4 codes four per 16-bit word", dict(_MX4, elements_per_sample=4, w_pack_bits=16), _hip.ERR_UNSUPPORTED),
    ("2-bit block-scaled", dict(_MX4, W_nbits=2), _hip.ERR_UNSUPPORTED),
    ("K % elements_per_sample", dict(K=260, ld_out=260, W_group_mode=0), _hip.ERR_BAD_SHAPE),
    ("K % group_size", dict(K=320, ld_out=320, group_size=128), _hip.ERR_BAD_SHAPE),
    ("K % group_size, odd group", dict(group_size=24), _hip.ERR_BAD_SHAPE),
    ("K % 32 block-scaled", dict(_MX8, K=48, ld_out=48), _hip.ERR_BAD_SHAPE),
    ("K % 32, nvfp4 block of 16", dict(_MX4, input_dtype=NVFP4, group_size=16, K=16, ld_out=16), _hip.ERR_BAD_SHAPE),
    ("grid.y limit", dict(K=256 * 65536, ld_out=256 * 65536), _hip.ERR_BAD_SHAPE),
    ("grid.x limit", dict(N=(2 ** 31) * 64), _hip.ERR_BAD_SHAPE),
]


@pytest.mark.parametrize("what,override,status", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_validation_refuses_before_any_launch(what, override, status):
    assert _hip.load().gemlite_hip_dequantize(C.byref(_args(**override)), None) == status


def test_null_args_pointer():
    assert _hip.load().gemlite_hip_dequantize(None, None) == _hip.ERR_BAD_ARGUMENT


# ------------------------------------------------------------------------------------------------ CPU routes
def test_cpu_layer_raises_like_forward():
    gen = torch.Generator().manual_seed(1)
    W_q = torch.randint(0, 16, (32, 128), generator=gen).to(torch.uint8)
    s, z = torch.rand(32 * 2, 1, generator=gen).half(), torch.rand(32 * 2, 1, generator=gen).half()
    layer = helper.A16W4_HQQ_INT(device="cpu").from_weights(W_q, s, z, 4, 64)
    assert layer.W_q.device.type == "cpu"
    with pytest.raises(_hip.GemliteHipError):
        layer.dequantize()
    with pytest.raises(_hip.GemliteHipError):
        layer(torch.zeros(1, 128, dtype=torch.float16))


def test_quantiser_level_calls_on_cpu():
    from gemlite_amd.quant_utils import WeightQuantizerINT
    with pytest.raises(_hip.GemliteHipError):  # no CPU fallback
        WeightQuantizerINT(4, 64).dequantize(torch.zeros(8, 64, dtype=torch.uint8), torch.ones(8, 1).half(), torch.ones(8, 1).half())
    wq = WeightQuantizerMXFP(compute_dtype=torch.bfloat16, device="cpu")
    W = torch.randn(8, 64, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    values = ds.E2M1
    for fmt, g in (("mxfp8", 32), ("mxfp4", 32), ("nvfp4", 16)):
        q, s = {"mxfp8": wq.quantize_mxfp8, "mxfp4": wq.quantize_mxfp4, "nvfp4": wq.quantize_nvfp4}[fmt](W, index=True)
        assert wq._dequantize_kernel(q, s, None, torch.float32) is None  # CPU tensors never reach the kernel
        el = values[q.int()] if q.dtype == torch.uint8 else q
        want = el.reshape(-1, g).float() * s.float().reshape(-1, 1)  # the torch code, as it has always been
        for dt in (None, torch.float16, torch.float32):
            got = wq.dequantize(q, s, shape=(8, 64), dtype=dt)
            assert got.dtype == (torch.bfloat16 if dt is None else dt) and tuple(got.shape) == (8, 64)
            assert ds.same(got, want.view(8, 64).to(got.dtype))
        assert tuple(wq.dequantize(q, s).shape) == (8 * 64 // g, g)
        # ... which is the restatement's arithmetic as well
        elem = el.reshape(8, 64).float()
        assert ds.same(ds.dequant_mx_spec(elem, s.view(torch.uint8).reshape(8, 64 // g), g, fmt == "nvfp4", torch.float32), want.view(8, 64))
