"""Bias inside the launch, host side (no GPU): the C ABI extension (gemlite_hip_forward_ext and the _ex / _bias_fused entry points), what
the planner answers for which request, the capture-group rule with a bias as one more read span, and the host logic of both call paths
with the library stubbed out.  Nothing is dereferenced, so the addresses are made up."""
import ctypes as C

import pytest
import torch

from gemlite_amd import _hip, core
from tests.test_abi_bounds_cpu import build_layer, plan_args
from tests.test_capture_groups_cpu import K, N, OUT_A, SHIFT_B, _args, _b

FP32, FP16, BF16 = 0, 1, 2
BIAS_A = 0x1500000000
BIAS_B = BIAS_A + SHIFT_B
GEMLITE_TF_GEMV_ROUND3_DECODE = 4096


def _ext(bias, dt=FP16):
    return _hip.forward_ext(bias, dt)


def _fused(a, e):
    return _hip.load().gemlite_hip_bias_fused(C.byref(a), C.byref(e) if e is not None else None)


def _name(a, e=None):
    return _hip.load().gemlite_hip_kernel_name_ex(C.byref(a), C.byref(e) if e is not None else None)


def test_the_new_symbols_exist_and_are_bound():
    lib = _hip.load()
    for sym in ("gemlite_hip_forward_ex", "gemlite_hip_bias_fused", "gemlite_hip_kernel_name_ex", "gemlite_hip_capture_group_compatible_ex"):
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
        assert getattr(lib, sym).argtypes is not None, sym
    assert C.sizeof(_hip.ForwardExt) == 16 and _hip.BIAS_NOT_ADDED == 1
    assert core.FUSE_BIAS is True


@pytest.mark.parametrize("dt", [FP16, BF16], ids=["fp16", "bf16"])
def test_the_decode_kernel_adds_the_bias_itself(dt):
    a = _args(dt=dt)
    assert _name(a) == b"gemv_w4_decode3_kernel<tile16,16w>"
    assert _fused(a, _ext(BIAS_A, dt)) == 1
    assert _name(a, _ext(BIAS_A, dt)) == b"gemv_w4_decode3_kernel<tile16,16w,bias>"


@pytest.mark.parametrize("dt", [FP16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("M", [2, 16, 17, 33, 64])
def test_the_rows_kernel_adds_the_bias_itself(M, dt):
    a = _args(dt=dt)
    a.M = M
    if M <= 4:
        a.tuning[0] = 9  # GEMLITE_T0_ROWS_KERNEL (2 .. 4 rows default to the matrix-core GEMV)
    plain = _name(a)
    assert plain.startswith(b"gemm_w4_rows_kernel<")
    assert _fused(a, _ext(BIAS_A, dt)) == 1
    assert _name(a, _ext(BIAS_A, dt)) == plain[:-1] + b",bias>"


def test_requests_the_library_leaves_to_the_caller():
    a = _args()
    assert _fused(a, _ext(BIAS_A, FP32)) == 0                     # an fp32 bias
    assert _fused(a, _ext(BIAS_A, BF16)) == 0                     # not the output's type
    assert _fused(_args(dt=BF16), _ext(BIAS_A, FP16)) == 0
    assert _fused(a, _ext(BIAS_A + 1, FP16)) == 0                 # not 2-byte aligned
    big = _args()
    big.M = 256                                                   # a tile kernel
    assert _hip.load().gemlite_hip_query(C.byref(big)) == 0 and _fused(big, _ext(BIAS_A)) == 0
    assert _name(big, _ext(BIAS_A)) == _name(big)
    forced = _args()
    forced.tuning[3] = GEMLITE_TF_GEMV_ROUND3_DECODE              # the round-3 decode kernel: no biased form
    assert _name(forced) == b"gemv_w4_decode_kernel<tile16,16w>" and _fused(forced, _ext(BIAS_A)) == 0
    probe = _args()
    probe.tuning[3] = 4                                           # GEMLITE_TF_TIMELINE: the probe keeps the two launches
    assert _fused(probe, _ext(BIAS_A)) == 0
    lin = build_layer(dict(kind="a8w8i", N=512, K=1024))          # A8W8
    for M in (1, 16):
        a8 = plan_args(lin, M)
        assert _hip.load().gemlite_hip_query(C.byref(a8)) == 0
        assert _fused(a8, _ext(BIAS_A, a8.output_dtype)) == 0


def test_without_a_bias_the_extension_changes_nothing():
    for a in (_args(), _args(dt=BF16), _b()):
        for M in (1, 8, 256):
            a.M = M
            plain = _hip.load().gemlite_hip_kernel_name(C.byref(a))
            assert _name(a, None) == plain and _name(a, _ext(None)) == plain
            assert _fused(a, None) == 0 and _fused(a, _ext(None)) == 0


def test_bad_arguments_are_refused():
    lib = _hip.load()
    a = _args()
    e = _ext(BIAS_A)
    e.struct_size = 8
    assert _fused(a, e) == _hip.ERR_BAD_ARGUMENT and _name(a, e) == b"invalid"
    assert lib.gemlite_hip_forward_ex(C.byref(a), C.byref(e), None) == _hip.ERR_BAD_ARGUMENT
    assert lib.gemlite_hip_bias_fused(None, C.byref(_ext(BIAS_A))) == _hip.ERR_BAD_ARGUMENT
    a.struct_size = 8
    assert _fused(a, _ext(BIAS_A)) == _hip.ERR_BAD_ARGUMENT


# ---- the capture-group rule: a fused bias is one more read span -----------------------------------------------------------------------
def _ok(a, ea, b, eb):
    lib = _hip.load()
    p = lambda e: C.byref(e) if e is not None else None  # noqa: E731
    ab = lib.gemlite_hip_capture_group_compatible_ex(C.byref(a), p(ea), C.byref(b), p(eb))
    assert ab == lib.gemlite_hip_capture_group_compatible_ex(C.byref(b), p(eb), C.byref(a), p(ea)), "the rule is symmetric"
    return ab == 1


def test_two_biased_launches_with_disjoint_buffers_join():
    assert _ok(_args(), _ext(BIAS_A), _b(), _ext(BIAS_B))
    assert _ok(_args(), _ext(BIAS_A), _b(), _ext(BIAS_A))           # a shared bias is a read on both sides
    assert _ok(_args(dt=BF16), _ext(BIAS_A, BF16), _b(dt=BF16), _ext(BIAS_B, BF16))


def test_a_biased_and_an_unbiased_launch_do_not_join():
    assert not _ok(_args(), _ext(BIAS_A), _b(), None)
    assert not _ok(_args(), _ext(BIAS_A), _b(), _ext(None))
    assert not _ok(_args(), _ext(BIAS_A), _b(), _ext(BIAS_B, FP32))  # a bias the launch does not add: an unbiased launch
    assert _ok(_args(), None, _b(), None) and _ok(_args(), _ext(None), _b(), None)
    lib = _hip.load()
    assert lib.gemlite_hip_capture_group_compatible(C.byref(_args()), C.byref(_b())) == 1  # the old entry: both unbiased


def test_an_output_on_the_other_launchs_bias_does_not_join():
    assert not _ok(_args(), _ext(BIAS_A), _b(out=BIAS_A + 2 * (N - 1)), _ext(BIAS_B))  # B's first output element = A's LAST bias element
    assert _ok(_args(), _ext(BIAS_A), _b(out=BIAS_A + 2 * N), _ext(BIAS_B))            # B's output begins where A's bias ends
    assert not _ok(_args(), _ext(BIAS_A), _b(out=BIAS_A - 2 * N + 2), _ext(BIAS_B))    # B's last output element = A's first bias element
    assert _ok(_args(), _ext(BIAS_A), _b(out=BIAS_A - 2 * N), _ext(BIAS_B))            # B's output ends exactly at A's bias's first byte
    assert not _ok(_args(), _ext(BIAS_A), _b(), _ext(OUT_A))                           # dependent THROUGH the bias: bias_B is out_A
    assert not _ok(_args(), _ext(BIAS_A), _b(), _ext(OUT_A - 2 * (N - 1)))                  # ... its LAST element is out_A's first
    assert _ok(_args(), _ext(BIAS_A), _b(), _ext(OUT_A - 2 * N))
    assert _ok(_args(), _ext(BIAS_A), _b(), _ext(OUT_A + 2 * N))


# ---- host logic with the library stubbed out ------------------------------------------------------------------------------------------
class _StubLib:
    def __init__(self, answer):
        self.answer, self.asked = answer, 0

    def gemlite_hip_bias_fused(self, a, e):
        self.asked += 1
        return self.answer


def _python_path(monkeypatch, answer, fuse):
    """core._forward_impl on CPU tensors with the launch replaced by zeros: (what the launch was given as bias, result, stub)"""
    lin = build_layer(dict(kind="wn", N=512, K=1024, nbits=4, gs=128, tdt=torch.float16))
    bias = torch.arange(512, dtype=torch.float32).to(torch.float16)
    stub = _StubLib(answer)
    seen = []

    def fake_matmul(x, W_q, scales, zeros, scales_x, meta_args, matmul_type, tuning=None, raw_x=False, bias=None):
        seen.append(bias)
        out = torch.zeros((x.shape[0], W_q.shape[1]), dtype=x.dtype)
        if bias is not None:
            out += 1000  # (stands for "the kernel added it")
        return out

    monkeypatch.setattr(core, "_hip_matmul", fake_matmul)
    monkeypatch.setattr(core._hip, "load", lambda: stub)
    monkeypatch.setattr(core, "_AUTOLOAD_DONE", True)
    monkeypatch.setattr(core, "FUSE_BIAS", fuse)
    core._FUSED_BIAS_ANSWERS.clear()
    x = torch.zeros(1, 1024, dtype=torch.float16)
    y = core._forward_impl(x, bias, lin.get_tensor_args(), lin.get_meta_args(), -1)
    y2 = core._forward_impl(x, bias, lin.get_tensor_args(), lin.get_meta_args(), -1)
    core._FUSED_BIAS_ANSWERS.clear()
    assert torch.equal(y, y2)
    return seen, y, bias, stub


def test_python_path_adds_the_bias_itself_when_the_library_answers_0(monkeypatch):
    seen, y, bias, stub = _python_path(monkeypatch, 0, True)
    assert seen == [None, None] and torch.equal(y[0], bias)
    assert stub.asked == 1, "the answer is cached per layer / shape / epoch"


def test_python_path_hands_the_bias_down_when_the_library_answers_1(monkeypatch):
    seen, y, bias, stub = _python_path(monkeypatch, 1, True)
    assert all(s is bias for s in seen) and torch.equal(y[0], torch.full((512,), 1000.0, dtype=torch.float16))
    assert stub.asked == 1


def test_with_the_switch_off_the_library_is_never_asked(monkeypatch):
    seen, y, bias, stub = _python_path(monkeypatch, 1, False)
    assert seen == [None, None] and torch.equal(y[0], bias) and stub.asked == 0


def test_a_new_tuning_epoch_asks_again(monkeypatch):
    lin = build_layer(dict(kind="wn", N=512, K=1024, nbits=4, gs=128, tdt=torch.float16))
    stub = _StubLib(0)
    monkeypatch.setattr(core._hip, "load", lambda: stub)
    monkeypatch.setattr(core, "_AUTOLOAD_DONE", True)
    core._FUSED_BIAS_ANSWERS.clear()
    x, bias = torch.zeros(1, 1024, dtype=torch.float16), torch.zeros(512, dtype=torch.float16)
    W_q, scales, zeros = lin.get_tensor_args()
    ask = lambda b=bias: core._library_adds_bias(x, W_q, scales, zeros, b, lin.get_meta_args(), -1)  # noqa: E731
    assert ask() is False and ask() is False and stub.asked == 1
    monkeypatch.setattr(core, "_CACHE_EPOCH", [core._CACHE_EPOCH[0] + 1])
    assert ask() is False and stub.asked == 2
    # biases the host never asks about: fp32, another type than x, not [N], not contiguous
    for b in (bias.float(), bias.to(torch.bfloat16), torch.zeros(1, 512, dtype=torch.float16), torch.zeros(1024, dtype=torch.float16)[::2]):
        assert ask(b) is False
    assert stub.asked == 2
    core._FUSED_BIAS_ANSWERS.clear()


class _StubFast:
    def __init__(self):
        self.calls = []

    def forward(self, *args):
        self.calls.append(args)
        return None  # "take the Python path"


@pytest.mark.parametrize("fuse", [True, False])
def test_the_fast_path_is_told_the_switch_and_falls_back_to_the_python_add(monkeypatch, fuse):
    """The C++ path gets core.FUSE_BIAS with every call (with False it never hands a bias to the library and adds it itself); when it
    declines the call, the Python path runs — here with a stub answer of 0, so its own add."""
    lin = build_layer(dict(kind="wn", N=512, K=1024, nbits=4, gs=128, tdt=torch.float16))
    bias = torch.arange(512, dtype=torch.float32).to(torch.float16)
    lin.bias = bias
    fast, stub = _StubFast(), _StubLib(0)
    monkeypatch.setattr(core, "_FAST", fast)
    monkeypatch.setattr(core, "FUSE_BIAS", fuse)
    monkeypatch.setattr(core, "_AUTOLOAD_DONE", True)
    monkeypatch.setattr(core._hip, "load", lambda: stub)
    monkeypatch.setattr(core, "_hip_matmul", lambda x, W_q, *a, bias=None, **k: torch.zeros((x.shape[0], W_q.shape[1]), dtype=x.dtype))
    core._FUSED_BIAS_ANSWERS.clear()
    lin.__dict__["_fast"] = ("capsule", lin.W_q, lin.scales, lin.zeros, bias)
    y = lin.forward_auto_no_warmup(torch.zeros(1, 1024, dtype=torch.float16))
    core._FUSED_BIAS_ANSWERS.clear()
    assert len(fast.calls) == 1 and len(fast.calls[0]) == 9 and fast.calls[0][5] is bias and fast.calls[0][8] is fuse
    assert torch.equal(y[0], bias) and stub.asked == (1 if fuse else 0)
