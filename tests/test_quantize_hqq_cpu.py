"""Host side of the HQQ zero-point optimiser (gemlite_hip_quantize_groups_hqq, WeightQuantizerHQQ, the *_HQQOPT_INT processors):
the C ABI entry and its validation table (nothing is launched), the struct mirror against the header, which classes exist,
and the two caps of tests/test_quantize_hqq_gpu.py checked where they can be checked without a device: on the float32
restatement (permuted sums, a perturbed power) against the float64 oracle, on that file's inputs."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, helper
from gemlite_amd.quant_utils import WeightQuantizerHQQ, WeightQuantizerINT
from tests.quant_hqq_spec import group_errors64, quantize_hqq_spec, student_t_weights
from tests.quant_int_spec import planted_weights, quantize_groups_spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32, FP16, BF16, INT8 = 0, 1, 2, 4

# shared with tests/test_quantize_hqq_gpu.py -------------------------------------------------------------------------------
# (N, K, g): one full tile | the smallest | ragged N, K no multiple of 256 | channel-wise, the group in the wave's registers |
# a group that does not divide 256 | several tiles both ways | channel-wise, a group the wave walks again per sum
SHAPES = [(64, 256, 64), (1, 32, 32), (80, 384, 128), (16, 512, 512), (64, 768, 96), (200, 1024, 32), (4, 8192, 8192)]
DTYPES = [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)]
ZERO_CAP, ERROR_CAP = 0.03, 1.001  # share of a case's groups whose stored zero may differ from the oracle's | summed error / oracle's


def make_weights(kind: str, N: int, K: int, g: int, in_dt: torch.dtype) -> torch.Tensor:
    if kind == "planted":
        return planted_weights(N, K, g, in_dt, seed=N * 7 + K)
    return student_t_weights(N, K, in_dt, seed=N * 7 + K)


@functools.lru_cache(maxsize=None)
def oracle(kind, N, K, g, in_dt, T, nbits):
    """(W on the CPU, RTN (q, s_r, z_r), float64 oracle (q, s_r, z_r, steps)): computed once, shared, never modified."""
    W = make_weights(kind, N, K, g, in_dt)
    return W, quantize_groups_spec(W, nbits, g, T), quantize_hqq_spec(W, nbits, g, T, dtype=np.float64)


def check_against_oracle(W, g, got, want, label):
    """The two caps: got / want = (q, s_r, z_r) of the code under test / of the float64 oracle.  Prints the figures, then asserts."""
    differ = int((got[2] != want[2]).sum())
    groups = want[2].numel()
    e_got, e_want = float(group_errors64(W, *got, g).sum()), float(group_errors64(W, *want, g).sum())
    print(f"{label}: zeros differ on {differ} / {groups} groups; summed error / oracle's = {e_got / max(e_want, 1e-300):.7f}")
    assert differ <= ZERO_CAP * groups
    assert e_got <= e_want * ERROR_CAP


# ------------------------------------------------------------------------------------------------------------------- C ABI
def test_symbol_is_declared_exported_and_abi_is_1():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    assert re.search(r"\bint\s+gemlite_hip_quantize_groups_hqq\s*\(\s*const\s+gemlite_hip_quantize_hqq_args\s*\*", header)
    assert "gemlite_hip_quantize_groups_hqq" in _hip.EXPORTED_SYMBOLS
    lib = _hip.load()
    assert hasattr(lib, "gemlite_hip_quantize_groups_hqq") and hasattr(lib, "gemlite_hip_quantize_groups")
    assert lib.gemlite_hip_abi_version() == 1 == _hip.ABI_VERSION
    assert re.search(r"#define\s+GEMLITE_HIP_ABI_VERSION\s+1\b", header)
    assert b"quantize_hqq" in lib.gemlite_hip_build_info()


def _args(iters=20, lp_norm=0.7, beta=10.0, kappa=1.01, struct_size=None, **kw):
    h = _hip.QuantizeHqqArgs()
    h.struct_size = C.sizeof(_hip.QuantizeHqqArgs) if struct_size is None else struct_size
    h.iters, h.lp_norm, h.beta, h.kappa = iters, lp_norm, beta, kappa
    a = h.q
    a.struct_size = C.sizeof(_hip.QuantizeArgs)
    a.w, a.q_out, a.scales, a.zeros = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every row below is refused
    a.w_dtype, a.meta_dtype = FP16, FP16
    a.N, a.K, a.ld_w, a.ld_q = 64, 256, 256, 256
    a.W_nbits, a.group_size, a.pack_bits = 4, 64, 32
    a.stride_meta_g, a.stride_meta_n, a.fold_zeros = 64, 1, 0
    for k, v in kw.items():
        setattr(a, k, v)
    return h


BAD_SHAPE_Q = dict(group_size=96)  # a valid optimiser around a bad embedded struct: the RTN export's code comes back
VALIDATION = [
    ("struct_size", dict(struct_size=C.sizeof(_hip.QuantizeHqqArgs) - 8), _hip.ERR_BAD_ARGUMENT),
    ("struct_size of the RTN struct", dict(struct_size=C.sizeof(_hip.QuantizeArgs)), _hip.ERR_BAD_ARGUMENT),
    ("iters < 0", dict(iters=-1), _hip.ERR_BAD_ARGUMENT),
    ("iters > 100", dict(iters=101), _hip.ERR_BAD_ARGUMENT),
    ("lp_norm = 0", dict(lp_norm=0.0), _hip.ERR_BAD_ARGUMENT),
    ("lp_norm < 0", dict(lp_norm=-0.5), _hip.ERR_BAD_ARGUMENT),
    ("lp_norm > 1", dict(lp_norm=1.5), _hip.ERR_BAD_ARGUMENT),
    ("lp_norm nan", dict(lp_norm=float("nan")), _hip.ERR_BAD_ARGUMENT),
    ("beta = 0", dict(beta=0.0), _hip.ERR_BAD_ARGUMENT),
    ("beta < 0", dict(beta=-10.0), _hip.ERR_BAD_ARGUMENT),
    ("beta nan", dict(beta=float("nan")), _hip.ERR_BAD_ARGUMENT),
    ("beta inf", dict(beta=float("inf")), _hip.ERR_BAD_ARGUMENT),
    ("kappa = 0", dict(kappa=0.0), _hip.ERR_BAD_ARGUMENT),
    ("kappa < 0", dict(kappa=-1.01), _hip.ERR_BAD_ARGUMENT),
    ("kappa nan", dict(kappa=float("nan")), _hip.ERR_BAD_ARGUMENT),
    ("bad optimiser before a bad shape", dict(iters=101, **BAD_SHAPE_Q), _hip.ERR_BAD_ARGUMENT),
    # the embedded struct: what gemlite_hip_quantize_groups returns for it (tests/test_quantize_groups_cpu.py has the whole table)
    ("q: struct_size", dict(q_struct_size=104), _hip.ERR_BAD_ARGUMENT),
    ("q: null w", dict(w=None), _hip.ERR_BAD_ARGUMENT),
    ("q: null zeros", dict(zeros=None), _hip.ERR_BAD_ARGUMENT),
    ("q: N = 0", dict(N=0), _hip.ERR_BAD_ARGUMENT),
    ("q: ld_w < K", dict(ld_w=128), _hip.ERR_BAD_ARGUMENT),
    ("q: 3 bits", dict(W_nbits=3), _hip.ERR_UNSUPPORTED),
    ("q: pack_bits 8", dict(pack_bits=8), _hip.ERR_UNSUPPORTED),
    ("q: int8 input", dict(w_dtype=INT8), _hip.ERR_UNSUPPORTED),
    ("q: fp32 metadata", dict(meta_dtype=FP32), _hip.ERR_UNSUPPORTED),
    ("q: g % 32", dict(group_size=16), _hip.ERR_BAD_SHAPE),
    ("q: K % g", BAD_SHAPE_Q, _hip.ERR_BAD_SHAPE),
    ("q: grid.y limit", dict(group_size=32, K=256 * 65536, ld_w=256 * 65536), _hip.ERR_BAD_SHAPE),
    ("q: bad shape with iters = 0", dict(iters=0, **BAD_SHAPE_Q), _hip.ERR_BAD_SHAPE),
]


@pytest.mark.parametrize("what,override,status", VALIDATION, ids=[v[0] for v in VALIDATION])
def test_validation_refuses_before_any_launch(what, override, status):
    override = dict(override)
    q_size = override.pop("q_struct_size", None)
    h = _args(**override)
    if q_size is not None:
        h.q.struct_size = q_size
    lib = _hip.load()
    assert lib.gemlite_hip_quantize_groups_hqq(C.byref(h), None) == status
    # and the embedded struct alone gets the same answer from the RTN export, unless the optimiser's constants were the reason
    if what.startswith("q:"):
        assert lib.gemlite_hip_quantize_groups(C.byref(h.q), None) == status


def test_null_args_pointer():
    assert _hip.load().gemlite_hip_quantize_groups_hqq(None, None) == _hip.ERR_BAD_ARGUMENT


STRUCT_FIELDS = ("struct_size", "iters", "q", "lp_norm", "beta", "kappa", "reserved")


def test_struct_mirror_matches_the_header_layout(tmp_path):
    # 4 + 4 | the RTN struct, 112, unchanged | 3 x 4 + 4: no padding anywhere
    H = _hip.QuantizeHqqArgs
    assert C.sizeof(_hip.QuantizeArgs) == 112 and C.sizeof(H) == 136
    assert [getattr(H, f).offset for f in STRUCT_FIELDS] == [0, 4, 8, 120, 124, 128, 132]
    assert [name for name, _ in H._fields_] == list(STRUCT_FIELDS) and H._fields_[2][1] is _hip.QuantizeArgs
    if shutil.which("gcc") is None:
        return  # the numbers above stand alone; with a C compiler the header itself is asked
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "gemlite_hip.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(gemlite_hip_quantize_hqq_args));\n'
                   + "".join(f'    printf(" %zu", offsetof(gemlite_hip_quantize_hqq_args, {f}));\n' for f in STRUCT_FIELDS)
                   + '    printf(" %zu\\n", sizeof(gemlite_hip_quantize_args));\n    return 0;\n}\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], check=True,
                   capture_output=True)
    out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(H)] + [getattr(H, f).offset for f in STRUCT_FIELDS] + [C.sizeof(_hip.QuantizeArgs)]


# ------------------------------------------------------------------------------------------------------------------ Python
def test_cpu_tensors_fail_loudly():
    W = torch.randn(64, 128, dtype=torch.float16)
    with pytest.raises(_hip.GemliteHipError):
        WeightQuantizerHQQ(4, 64).quantize(W)
    with pytest.raises(_hip.GemliteHipError):
        WeightQuantizerHQQ(4, 64).quantize_packed(W, fold_zeros=True)
    lin = torch.nn.Linear(128, 64, dtype=torch.float16)
    for proc in (helper.A16W4_HQQOPT_INT(group_size=64), helper.A16W1_HQQOPT_INT(), helper.A8W4_HQQOPT_INT_dynamic(group_size=64)):
        with pytest.raises(_hip.GemliteHipError):
            proc.from_linear(lin)
    assert lin.weight is not None  # nothing was cleaned up


def test_classes_keywords_and_the_quantiser_hook():
    new = {helper.A16Wn_HQQOPT_INT: (None, helper.A16Wn_RTN_INT), helper.A16W8_HQQOPT_INT: (8, helper.A16Wn_RTN_INT),
           helper.A16W4_HQQOPT_INT: (4, helper.A16Wn_RTN_INT), helper.A16W2_HQQOPT_INT: (2, helper.A16Wn_RTN_INT),
           helper.A16W1_HQQOPT_INT: (1, helper.A16Wn_RTN_INT), helper.A8Wn_HQQOPT_INT_dynamic: (None, helper.A8Wn_RTN_INT_dynamic),
           helper.A8W4_HQQOPT_INT_dynamic: (4, helper.A8Wn_RTN_INT_dynamic), helper.A8W2_HQQOPT_INT_dynamic: (2, helper.A8Wn_RTN_INT_dynamic)}
    for cls, (bits, parent) in new.items():
        assert issubclass(cls, parent) and issubclass(cls, helper._RTNGroupQuant), cls.__name__
        assert cls.W_nbits == bits
        for name in ("from_linear", "quantize_weights", "from_hqqlinear", "from_weights"):
            assert hasattr(cls, name), (cls.__name__, name)
    # the classes fed from already quantised tensors stay as they were
    for cls in (helper.A16Wn_HQQ_INT, helper.A16W4_HQQ_INT, helper.A8Wn_HQQ_INT_dynamic, helper.A8W4_HQQ_INT_dynamic):
        assert not hasattr(cls, "from_linear") and not hasattr(cls, "quantize_weights"), cls.__name__
    p = helper.A16W4_HQQOPT_INT(device="cpu", dtype=torch.bfloat16, group_size=128, iters=7, lp_norm=1.0, beta=4.0, kappa=1.5)
    q = p._make_quantizer(128, "cpu")
    assert type(q) is WeightQuantizerHQQ and isinstance(q, WeightQuantizerINT)
    assert (q.W_nbits, q.group_size, q.dtype, q.iters, q.lp_norm, q.beta, q.kappa) == (4, 128, torch.bfloat16, 7, 1.0, 4.0, 1.5)
    d = helper.A8W2_HQQOPT_INT_dynamic(group_size=32)._make_quantizer(32, "cpu")
    assert (d.W_nbits, d.iters, d.lp_norm, d.beta, d.kappa) == (2, 20, 0.7, 10.0, 1.01)  # HQQ's defaults
    assert type(helper.A16W4_RTN_INT()._make_quantizer(64, "cpu")) is WeightQuantizerINT
    assert helper.A16Wn_HQQOPT_INT(W_nbits=2).W_nbits == 2 and helper.A16W4_HQQOPT_INT().group_size is None
    for bad in (dict(iters=-1), dict(iters=101), dict(lp_norm=0.0), dict(lp_norm=1.5), dict(beta=0.0), dict(kappa=float("nan"))):
        with pytest.raises(ValueError, match="WeightQuantizerHQQ"):
            WeightQuantizerHQQ(4, 64, **bad)


def test_patch_model_names_the_new_processors_for_the_old_ones():
    net = torch.nn.Sequential(torch.nn.Linear(64, 64))
    with pytest.raises(NotImplementedError, match="HQQOPT_INT"):
        helper.patch_model(net, "cpu", helper.A16W4_HQQ_INT())
    assert "HQQOPT_INT" in helper.patch_model.__doc__


# ------------------------------------------------------------------------------------------- the caps, where they can be checked
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("kind", ["planted", "student_t"])
@pytest.mark.parametrize("N,K,g", SHAPES, ids=[f"{n}x{k}g{g}" for n, k, g in SHAPES])
def test_float32_restatement_stays_within_the_caps(N, K, g, kind, nbits):
    for in_dt, T in DTYPES:
        W, rtn, want = oracle(kind, N, K, g, in_dt, T, nbits)
        perm = np.random.default_rng(g + nbits).permutation(g)
        got = quantize_hqq_spec(W, nbits, g, T, dtype=np.float32, perm=perm, pow_ulp=4)
        assert torch.equal(got[1], rtn[1]) and torch.equal(want[1], rtn[1])  # the scale is RTN's
        check_against_oracle(W, g, got[:3], want[:3], f"{N}x{K} g{g} {kind} {nbits} bits {in_dt}")
        # and the guarantee: no group of the oracle (or of the restatement) ends worse than RTN, up to the fp32 sums compared
        e_rtn = group_errors64(W, *rtn, g)
        for out in (got, want):
            assert (group_errors64(W, *out[:3], g) <= e_rtn * (1 + 2 * g * 2.0 ** -24)).all()


def test_zero_iterations_is_rtn_and_the_oracle_gains_what_the_issue_measured():
    N, K, g = 64, 256, 64
    W = student_t_weights(N, K, torch.float16, seed=1)
    q0, s0, z0 = quantize_groups_spec(W, 4, g, torch.float16)
    q, s, z, steps = quantize_hqq_spec(W, 4, g, torch.float16, iters=0)
    assert torch.equal(q, q0) and torch.equal(s, s0) and torch.equal(z, z0) and not steps.any()
    for nbits, gg, below in ((4, 64, 0.98), (2, 64, 0.95), (1, 32, 0.60)):  # measured while designing: 0.96 / 0.91 / 0.50
        rtn = quantize_groups_spec(W, nbits, gg, torch.float16)
        opt = quantize_hqq_spec(W, nbits, gg, torch.float16)
        ratio = float(group_errors64(W, *opt[:3], gg).sum() / group_errors64(W, *rtn, gg).sum())
        print(f"{nbits} bits g{gg}: HQQ / RTN error = {ratio:.4f}")
        assert ratio < below
