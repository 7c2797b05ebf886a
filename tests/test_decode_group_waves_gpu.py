"""The grouped M = 1 decode kernel gives every layer of a block its own waves (gemv_decode.hip, gemv_w4_decode3_group_kernel, unbiased /
biased): block (tile, y) holds LB layers at once, 16 / LB waves each, a wave walks a contiguous run of the single-layer
kernel's waves ("virtual waves") through a two-buffer ring of counted requests, and the block has one barrier.  Every comparison is
BIT-EXACT (torch.equal) against the eager output of the same layer; outputs are pre-filled with NaN before the replay, so a layer that
was skipped shows; every case names the kernel the planner gives its layers."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_cpu import kernel_name, plan_args
from tests.test_capture_groups_gpu import DEV, _capture, _gmax, _layer, _replay, _x
from tests.test_decode_group_stream_gpu import _grid_y
from tests.test_fused_bias_gpu import _eager_unfused
from tests.test_fused_bias_gpu import _layer as _biased_layer

pytestmark = pytest.mark.gpu
F16, B16 = torch.float16, torch.bfloat16
KERNEL = "gemv_w4_decode3_kernel<"


@functools.lru_cache(maxsize=None)
def _member(N, K, tdt, i):
    """Member i of the (N, K, tdt) pool: (layer, its own x, its eager output).  Built once, shared by every case, never written."""
    lin = _layer(N, K, 128, tdt, seed=9000 + 31 * i + (N + K) % 997)
    assert kernel_name(plan_args(lin, 1)).startswith(KERNEL)
    x = _x(K, tdt, seed=9500 + i)
    want = lin(x).clone()
    torch.cuda.synchronize()
    return lin, x, want


def _run_group(N, K, members, tdt=F16):
    assert members <= _gmax(), "a build with a lower member limit runs other groups than these cases describe"
    lins, xs, want = zip(*[_member(N, K, tdt, i) for i in range(members)])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in zip(lins, xs)])
    assert seen == members and joined == members - 1, (seen, joined)
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} of {members} (N={N} K={K} {tdt})"
    return g, lins, xs, outs


@pytest.mark.parametrize("members", [2, 3, 4, 5, 6, 7, 8, 9, 15, 16], ids=lambda m: f"m{m}")
@pytest.mark.parametrize("K", [512, 4352], ids=lambda k: f"K{k}")
def test_waves_per_layer_in_one_block(K, members):
    """N = 4096 is the narrowest width with grid.y = 1 on 256 CUs: one block holds every member, 8, 5, 4, 3, 2, 2, 2, 1, 1, 1 waves per
    layer (5 and 3 leave a wave idle, 9 and 15 leave seven and one).  K = 512: 2 chunks, 14 virtual waves of a layer write zeros.
    K = 4352: 17 chunks, virtual wave 0 holds two."""
    assert _grid_y(4096, members) == 1
    _run_group(4096, K, members)


@pytest.mark.parametrize("K", [256 * n for n in range(1, 8)], ids=lambda k: f"K{k}")
def test_ring_tail_with_one_wave_per_layer(K):
    """16 members in one block: a wave's item list is its layer's K / 256 chunks, 1 .. 7 — the ring's peeled tails (1, 2, 3 items
    left) with no, one and two trips of the steady-state loop in front.  (The planner gives every one of these K to this kernel.)"""
    assert _grid_y(4096, 16) == 1
    _run_group(4096, K, 16)


def test_ring_tail_with_43_chunks_over_five_waves_per_layer():
    """K = 11008, 3 members: waves own 3, 3, 3, 3, 4 virtual waves of 3 or 2 chunks each: 9, 9, 8, 6 and 8 items."""
    assert _grid_y(4096, 3) == 1
    _run_group(4096, 11008, 3)


@pytest.mark.parametrize("N,members", [(1024, 7), (1024, 13), (1024, 16), (256, 16)], ids=lambda v: str(v))
def test_blocks_of_one_launch_hold_different_numbers_of_layers(N, members):
    """64 tiles, grid.y = 4: the blocks hold 2, 2, 2, 1 layers, then 4, 3, 3, 3, then 4, 4, 4, 4.  16 tiles: grid.y = 16, one layer per
    block, all 16 waves on it — the single-layer split."""
    assert _grid_y(N, members) == (4 if N == 1024 else 16)
    _run_group(N, 4096, members)


@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
def test_replay_follows_an_x_rewritten_in_place(tdt):
    """Every member has its own x (as in every case here); member 2's is rewritten between two replays."""
    g, lins, xs, outs = _run_group(4096, 4096, 6, tdt=tdt)
    old = xs[2].clone()
    try:
        xs[2].copy_(_x(4096, tdt, seed=777))
        want2 = lins[2](xs[2]).clone()
        torch.cuda.synchronize()
        assert not torch.equal(want2, _member(4096, 4096, tdt, 2)[2])
        for o in outs:
            o.fill_(float("nan"))
        _replay(g, 1)
        for i, o in enumerate(outs):
            assert torch.equal(o, want2 if i == 2 else _member(4096, 4096, tdt, i)[2]), f"layer {i}"
    finally:
        xs[2].copy_(old)  # the pool's inputs stay what the pooled outputs were computed from
        torch.cuda.synchronize()


def _layer_own_zero(N, K, tdt, seed, zeros_kind, zero_point):
    """As tests/test_decode_group_stream_gpu.py::_layer_mode, with the integer zero point of the "int" kind given by the caller."""
    W_q, scales, zeros = O.gen_data(N, K, 4, 128, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, 128, K, N, code, code)
    s = torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV)
    z = {"tensor": torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV), "int": zero_point, "none": None}[zeros_kind]
    lin.pack(torch.from_numpy(W_q).to(DEV), s, z, None, fma_mode=True)
    return lin


@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("zeros_kind,w_mode", [("tensor", 4), ("int", 3), ("none", 2)], ids=["scales+zeros", "scalar-zero", "no-zero"])
def test_one_group_per_metadata_mode(zeros_kind, w_mode, tdt):
    """Five members, three waves each and one idle.  Scalar zero: read once per wave from the wave's own layer — every member has
    ANOTHER zero point (3, 5, 7, 9, 11), so a wave that read a neighbour's gives a wrong row.  No zeros / a scalar zero: the loop variant
    that keeps the metadata selects, and requests that go to the weight buffer instead."""
    N, K = 4096, 768
    lins = [_layer_own_zero(N, K, tdt, 700 + i, zeros_kind, 3 + 2 * i) for i in range(5)]
    assert lins[0].W_group_mode == w_mode
    assert kernel_name(plan_args(lins[0], 1)).startswith(KERNEL)
    xs = [_x(K, tdt, seed=71 + i) for i in range(5)]
    want = [lin(x).clone() for lin, x in zip(lins, xs)]
    torch.cuda.synchronize()
    if zeros_kind == "int":  # the zero point matters: the same layer and x with its neighbour's zero point gives another row
        other = _layer_own_zero(N, K, tdt, 700, zeros_kind, 5)
        assert not torch.equal(other(xs[0]), want[0])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in zip(lins, xs)])
    assert seen == 5 and joined == 4
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} ({zeros_kind}, {tdt})"


@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
def test_biased_group_keeps_both_roundings_in_the_tie_columns(tdt):
    """The inputs of tests/test_fused_bias_gpu.py::test_special_bias_values_and_both_roundings — acc = 1 + half an ulp, bias a quarter —
    in a group of three (five waves per layer; waves 0 .. 2 finish a layer each and ask for its bias element before the barrier)."""
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
    assert kernel_name(plan_args(lins[0], 1)).startswith(KERNEL)
    try:
        want = _eager_unfused(lins, x)  # a matmul launch, then torch's add
        one = torch.ones((), dtype=tdt)
        for w in want:
            assert bool((w[0, :N // 2].cpu() == one).all()), "two roundings give exactly 1 in the tie columns (one rounding: 1 + ulp)"
        g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
        assert seen == members and joined == members - 1
        for o in outs:
            o.fill_(float("nan"))
        _replay(g, 2)
        for i, (o, w) in enumerate(zip(outs, want)):
            assert torch.equal(o, w), f"layer {i}"
    finally:
        core.FUSE_BIAS = True


@pytest.mark.parametrize("N,members", [(4096, 7), (1024, 13)], ids=["one-block", "grid-y"])
def test_adjacent_outputs_of_one_allocation_between_guard_bytes(N, members):
    """The outs are adjacent rows of ONE allocation between 0xFF guard bytes: a store into another member's row shows as a wrong
    row, a store outside every out as a changed guard byte."""
    K, tdt, guard = 4096, F16, 512
    lins, xs, want = zip(*[_member(N, K, tdt, i) for i in range(members)])
    buf = torch.empty(guard + members * N + guard, dtype=tdt, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    lib = _hip.load()
    calls = []
    for i, (lin, x) in enumerate(zip(lins, xs)):
        a = plan_args(lin, 1, x=x.data_ptr(), out=buf[guard + i * N:].data_ptr(), stride_xm=K, stride_om=N)
        assert kernel_name(a).startswith(KERNEL) and lib.gemlite_hip_workspace_bytes(C.byref(a)) == 0
        calls.append(a)

    def step():
        st = torch.cuda.current_stream().cuda_stream
        for a in calls:
            assert lib.gemlite_hip_forward(C.byref(a), st) == 0
        return None

    g, _, seen, joined = _capture(step)
    assert seen == members and joined == members - 1
    buf.view(torch.uint8).fill_(0xFF)
    _replay(g, 2)
    raw = buf.view(torch.int16)
    assert bool((raw[:guard] == -1).all()) and bool((raw[guard + members * N:] == -1).all()), "a store outside every member's out"
    for i, w in enumerate(want):
        assert torch.equal(buf[guard + i * N: guard + (i + 1) * N].view(1, N), w), f"layer {i}"
