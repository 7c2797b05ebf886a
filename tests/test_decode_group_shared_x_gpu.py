"""The SHARED-X form of the grouped M = 1 decode kernel (gemv_decode.hip, gemv_w4_decode3_group_kernel with SX = true): a group
whose members all read the same x stages the pair dwords and the per-unit sums of x in LDS once per block, and an item is four
requests and three LDS reads.  ONE x tensor is passed to every member here.  Every comparison is BIT-EXACT (torch.equal) against the eager
output of the same layer on the same x; outputs are pre-filled with NaN before the replay; every case asserts through
gemlite_hip_capture_group_last_form() that the shared-x form ran (form 2) or, where stated, that it did not (form 1)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, core
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_cpu import kernel_name, plan_args
from tests.test_capture_groups_gpu import DEV, ROOT, _capture, _gmax, _replay, _x
from tests.test_decode_group_stream_gpu import _grid_y
from tests.test_decode_group_waves_gpu import KERNEL, _layer_own_zero, _member
from tests.test_fused_bias_gpu import _eager_unfused
from tests.test_fused_bias_gpu import _layer as _biased_layer

pytestmark = pytest.mark.gpu
F16, B16 = torch.float16, torch.bfloat16
DTYPES = pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
PER_WAVE_X, SHARED_X = 1, 2


def _form():
    return _hip.load().gemlite_hip_capture_group_last_form()


@functools.lru_cache(maxsize=None)
def _shared_x(K, tdt):
    return _x(K, tdt, seed=8800 + K % 991)


@functools.lru_cache(maxsize=None)
def _want(N, K, tdt, i):
    """Eager output of member i of the (N, K, tdt) pool of tests/test_decode_group_waves_gpu.py on the shared x.  Computed once, never written."""
    y = _member(N, K, tdt, i)[0](_shared_x(K, tdt)).clone()
    torch.cuda.synchronize()
    return y


def _check(outs, want, what):
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} of {len(want)} ({what})"


def _run_group(N, K, members, tdt=F16, form=SHARED_X):
    assert members <= _gmax(), "a build with a lower member limit runs other groups than these cases describe"
    lins = [_member(N, K, tdt, i)[0] for i in range(members)]
    want = [_want(N, K, tdt, i) for i in range(members)]
    x = _shared_x(K, tdt)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == members and joined == members - 1, (seen, joined)
    assert _form() == form, _form()
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    _check(outs, want, f"N={N} K={K} {tdt}")
    return g, lins, outs


@DTYPES
@pytest.mark.parametrize("members", [2, 3, 5, 9, 16], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("K", [256, 512, 768, 4096, 4352], ids=lambda k: f"K{k}")
def test_item_counts_in_one_block(K, members, tdt):
    """N = 4096: grid.y = 1, one block holds every member (8, 5, 3, 1, 1 waves per layer).  Two members keep the per-wave-x form by the rule
    on the member count (staging costs more than it saves there) and are still bit-exact; blocks of two layers in the shared-x form:
    test_blocks_of_one_launch_hold_different_numbers_of_layers.  K = 256 .. 4352 is 1, 2, 3, 16 and 17 chunks: the
    ring's three peeled tails, virtual waves without a chunk, a virtual wave with two chunks; 16, 32, 48, 256 and 272 staged units (one
    to five staging waves, the last one of K = 256 / 768 / 4352 with 16 of its 64 lanes past the last unit)."""
    assert _grid_y(4096, members) == 1
    _run_group(4096, K, members, tdt, form=PER_WAVE_X if members == 2 else SHARED_X)


def test_staging_of_688_units_and_43_chunks():
    """K = 11008, 3 members: 688 units under the block's 1024 threads (ten full staging waves, one of 48 lanes, five that stage nothing);
    43 chunks over five waves per layer."""
    assert _grid_y(4096, 3) == 1
    _run_group(4096, 11008, 3)


def test_staging_by_every_wave_idle_ones_included():
    """K = 16128, 3 members: the largest K of one staging trip the planner gives this kernel at this width (K = 16384 goes to
    gemv_wn_kernel).  1008 units: every wave of the block stages, the last with 48 lanes — wave 15 too, which has no layer and no item
    (five waves per layer) and still loads, stages units 960 .. 1007 and meets the barrier.  63 chunks, 99.4 KiB of dynamic LDS."""
    assert _grid_y(4096, 3) == 1
    assert _hip.load().gemlite_hip_capture_group_shared_x_lds_bytes(16128) == 65536 + 1008 * 36
    _run_group(4096, 16128, 3)


@pytest.mark.parametrize("members", [3, 16], ids=lambda m: f"m{m}")
def test_the_second_staging_trip(members):
    """K = 16640 at N = 4096 reaches this kernel: 1040 units, so threads 0 .. 15 stage a second unit (u + 1024) behind the same counted
    wait (the planner sends odd multiples of 256 up to 32512 here: never a third trip); 65 chunks.  Three members: five waves per layer, wave 15 has no layer and no item and still stages units 960 .. 1023."""
    assert _grid_y(4096, members) == 1
    _run_group(4096, 16640, members)


@pytest.mark.parametrize("N,members", [(1024, 7), (1024, 16), (256, 16)], ids=lambda v: str(v))
def test_blocks_of_one_launch_hold_different_numbers_of_layers(N, members):
    """64 tiles, grid.y = 4: blocks of 2, 2, 2, 1 layers and of 4 each; 16 tiles, grid.y = 16: one layer per block, every block stages x."""
    assert _grid_y(N, members) == (4 if N == 1024 else 16)
    _run_group(N, 4096, members)


@DTYPES
@pytest.mark.parametrize("zeros_kind,w_mode", [("tensor", 4), ("int", 3), ("none", 2)], ids=["scales+zeros", "scalar-zero", "no-zero"])
def test_one_group_per_metadata_mode(zeros_kind, w_mode, tdt):
    """Five members on one x, K = 768.  Scalar zero: every member has ANOTHER zero point (3, 5, 7, 9, 11), read once per wave from the wave's own
    layer.  No zeros / a scalar zero: the loop variant that keeps the metadata selects (it stages x on its own)."""
    N, K = 4096, 768
    lins = [_layer_own_zero(N, K, tdt, 700 + i, zeros_kind, 3 + 2 * i) for i in range(5)]
    assert lins[0].W_group_mode == w_mode
    assert kernel_name(plan_args(lins[0], 1)).startswith(KERNEL)
    x = _shared_x(K, tdt)
    want = [lin(x).clone() for lin in lins]
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 5 and joined == 4 and _form() == SHARED_X
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    _check(outs, want, f"{zeros_kind}, {tdt}")


@DTYPES
def test_biased_group(tdt):
    """Four biased members (four waves each) on one x: the bias is added in the shared-x form's epilogue; compared with the matmul launch followed by torch's add."""
    N, K, members = 4096, 768, 4
    lins = []
    for i in range(members):
        bias = torch.randn(N, generator=torch.Generator().manual_seed(40 + i))
        lins.append(_biased_layer(N, K, tdt, seed=60 + i, bias=bias.to(tdt).to(DEV)))
    x = _shared_x(K, tdt)
    assert kernel_name(plan_args(lins[0], 1)).startswith(KERNEL)
    want = _eager_unfused(lins, x)  # a matmul launch, then torch's add
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == members and joined == members - 1 and _form() == SHARED_X
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    _check(outs, want, f"biased {tdt}")


@DTYPES
def test_biased_group_keeps_both_roundings_in_the_tie_columns(tdt):
    """The inputs of tests/test_fused_bias_gpu.py::test_special_bias_values_and_both_roundings — acc = 1 + half an ulp, bias a quarter —
    in a shared-x group of three."""
    N, K, members = 4096, 512, 3
    t = 2.0 ** -11 if tdt == F16 else 2.0 ** -8
    lins = []
    for i in range(members):
        W_q, scales, zeros = O.gen_data(N, K, 4, 128, seed=5 + i, np_float=np.float16)
        W_q[:, :2] = 1
        scales[:] = 1
        zeros[:] = 0
        bias = torch.full((N,), t / 2, dtype=torch.float32)
        bias[N // 2:] = torch.randn(N // 2, generator=torch.Generator().manual_seed(i))
        lins.append(_biased_layer(N, K, tdt, seed=5 + i, bias=bias.to(tdt).to(DEV), arrays=(W_q, scales, zeros)))
    x = torch.zeros(1, K, dtype=tdt, device=DEV)
    x[0, 0], x[0, 1] = 1.0, t
    try:
        want = _eager_unfused(lins, x)  # a matmul launch, then torch's add
        one = torch.ones((), dtype=tdt)
        for w in want:
            assert bool((w[0, :N // 2].cpu() == one).all()), "two roundings give exactly 1 in the tie columns (one rounding: 1 + ulp)"
        g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
        assert seen == members and joined == members - 1 and _form() == SHARED_X
        for o in outs:
            o.fill_(float("nan"))
        _replay(g, 2)
        _check(outs, want, f"tie columns {tdt}")
    finally:
        core.FUSE_BIAS = True


@DTYPES
def test_replay_follows_the_shared_x_rewritten_in_place(tdt):
    """x is staged from memory in every launch: after x is rewritten in place, a replay gives every layer's eager output on the new x."""
    N, K, members = 4096, 4096, 6
    lins = [_member(N, K, tdt, i)[0] for i in range(members)]
    x = _shared_x(K, tdt).clone()
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == members and joined == members - 1 and _form() == SHARED_X
    _replay(g, 1)
    _check(outs, [_want(N, K, tdt, i) for i in range(members)], "first x")
    x.copy_(_x(K, tdt, seed=777))
    want = [lin(x).clone() for lin in lins]
    torch.cuda.synchronize()
    assert not torch.equal(want[0], _want(N, K, tdt, 0))
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 1)
    _check(outs, want, "rewritten x")


@pytest.mark.parametrize("odd", [1, 4], ids=["second", "last"])
def test_a_member_with_another_x_puts_the_group_on_the_per_wave_form(odd):
    """Five members; member `odd` reads a tensor of its own (equal VALUES in another allocation would do: the rule compares pointers).  The
    group is rewritten to the per-wave-x form at that join and stays there; every layer is still bit-exact."""
    N, K, tdt, members = 4096, 768, F16, 5
    lins = [_member(N, K, tdt, i)[0] for i in range(members)]
    x, x_odd = _shared_x(K, tdt), _member(N, K, tdt, odd)[1]
    want = [_member(N, K, tdt, i)[2] if i == odd else _want(N, K, tdt, i) for i in range(members)]
    g, outs, seen, joined = _capture(lambda: [lin(x_odd if i == odd else x) for i, lin in enumerate(lins)])
    assert seen == members and joined == members - 1
    assert _form() == PER_WAVE_X
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    _check(outs, want, f"member {odd} on its own x")


_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
from gemlite_amd import _hip
from tests.test_capture_groups_gpu import _layer, _x, _eager, _capture, _replay
lins = [_layer(4096, 768, 128, torch.float16, seed=120 + i) for i in range(4)]
x = _x(768, torch.float16, seed=15)
want = _eager(lins, x)
g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
form = _hip.load().gemlite_hip_capture_group_last_form()
for o in outs:
    o.fill_(float("nan"))
_replay(g)
print("RESULT", seen, joined, form, _hip.load().gemlite_hip_capture_group_form(4, 1, 768), all(torch.equal(o, w) for o, w in zip(outs, want)))
"""


def test_the_switch_keeps_a_shared_x_group_on_the_per_wave_form():
    """GEMLITE_HIP_CAPTURE_GROUP_SHARED_X=0 in a fresh process (the switch is read once): four members on one x still become one launch,
    of the per-wave-x form, equal to eager."""
    env = dict(os.environ, GEMLITE_HIP_CAPTURE_GROUP_SHARED_X="0")
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert line[1:] == ["4", "3", "1", "1", "True"], line


@pytest.mark.parametrize("amp", [1e-3, 1e-4], ids=["1e-3", "1e-4"])
def test_small_magnitude_fp16_activations(amp):
    """Shared x at |x| ~ amp in fp16 (products and staged pair dwords deep in fp16's subnormal range): three members, bit-equal to the
    eager layer and within the bound of tests/test_gpu_parity.py::test_small_magnitude_fp16_activations_on_the_decode_kernels of the
    float64 oracle (4e-4 of mean |y|: the rounding of the output alone, plus the output's quantum 2^-24 where mean |y| nears it)."""
    from tests.test_gpu_parity import _oracle_from_layer
    N, K, members = 4096, 4096, 3
    lins = [_member(N, K, F16, i)[0] for i in range(members)]
    x = torch.from_numpy((np.random.default_rng(7).standard_normal((1, K)) * amp).astype(np.float16)).to(DEV)
    want = [lin(x).clone() for lin in lins]
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == members and joined == members - 1 and _form() == SHARED_X
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    _check(outs, want, f"amp {amp}")
    for i, (lin, o) in enumerate(zip(lins, outs)):
        y_or = _oracle_from_layer(lin, x)
        rel = float(np.abs(o.float().cpu().numpy().astype(np.float64) - y_or).mean() / np.abs(y_or).mean())
        print(f"small-x amp={amp} layer {i}: rel={rel:.3e}")
        assert rel < 4e-4 + 2.0 ** -25 / np.abs(y_or).mean(), (amp, i, rel)
