"""The grouped M = 1 decode kernel streams the layers of a capture group through one resident block per tile (gemv_decode.hip,
gemv_w4_decode3_group_kernel): a layer loop with a ring of chunk buffers, grid (N / 16, Y).  Every comparison is BIT-EXACT (torch.equal)
against the eager output of the same layer; outputs are pre-filled with NaN before the replay, so a skipped layer shows."""
import ctypes as C

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip
from oracle import gemlite_oracle as O
from tests.test_abi_bounds_cpu import kernel_name, plan_args
from tests.test_capture_groups_gpu import DEV, _capture, _eager, _gmax, _layer, _replay, _x

pytestmark = pytest.mark.gpu
RING = 2  # must match DECODE3_RING of gemlite_amd/csrc/gl_common.h (a -DDECODE3_RING=3 build wants 3 here)


def _grid_y(N, members):
    """grid.y a launch on THIS device gets: the exported rule with the device's CU count in place of 256."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return max(1, min(cus // (N // 16), members))


def _run_group(N, K, members, tdt=torch.float16, gs=128, seed=0, own_x=False):
    lins = [_layer(N, K, gs, tdt, seed=seed + i) for i in range(members)]
    xs = [_x(K, tdt, seed=seed + 100 + (i if own_x else 0)) for i in range(members)]
    if not own_x:
        xs = [xs[0]] * members
    want = [lin(x).clone() for lin, x in zip(lins, xs)]
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in zip(lins, xs)])
    assert seen == members and joined == min(members, _gmax()) - 1, (seen, joined)
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} of {members} (N={N} K={K} {tdt})"
    return g, lins, xs, outs


@pytest.mark.parametrize("members", sorted({2, 3, RING + 1, RING + 2}) + ["max"], ids=lambda m: f"m{m}")
def test_member_counts_against_the_ring_in_one_block(members):
    members = _gmax() if members == "max" else min(members, _gmax())
    assert _grid_y(4096, members) == 1
    _run_group(4096, 4096, members, seed=200)


@pytest.mark.parametrize("K", [2048, 4096, 4352, 11008], ids=lambda k: f"K{k}")
def test_chunks_per_wave(K):
    """nch_total = K / 256: 8 (half the waves hold no row), 16 (one item per wave and layer), 17 (wave 0 holds two), 43."""
    _run_group(4096, K, 5, seed=300)


@pytest.mark.parametrize("members", [7, 3, 4], ids=lambda m: f"m{m}")
def test_narrow_layers_split_over_grid_y(members):
    """64 tiles: 7 members run as grid.y = 4 (blocks hold 2, 2, 2, 1 layers); 3 and 4 members as grid.y = members."""
    assert _grid_y(1024, members) == min(4, members)
    _run_group(1024, 4096, members, seed=400)


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_every_member_has_its_own_x(tdt):
    _run_group(4096, 4096, 6, tdt=tdt, seed=500, own_x=True)


def test_replay_follows_a_new_x_written_in_place():
    g, lins, xs, outs = _run_group(4096, 4096, 5, seed=600)
    x_new = _x(4096, torch.float16, seed=777)
    want_new = _eager(lins, x_new)
    xs[0].copy_(x_new)
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 1)
    for i, (o, w) in enumerate(zip(outs, want_new)):
        assert torch.equal(o, w), f"layer {i}"


def _layer_mode(N, K, gs, tdt, seed, zeros_kind):
    """scales + zeros (W_group_mode 4), "int": scales and ONE integer zero point (3, zero_is_scalar), "none": scales only (2)."""
    W_q, scales, zeros = O.gen_data(N, K, 4, gs, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, gs, K, N, code, code)
    s = torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV)
    z = {"tensor": torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV), "int": 7, "none": None}[zeros_kind]
    lin.pack(torch.from_numpy(W_q).to(DEV), s, z, None, fma_mode=True)
    return lin


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("zeros_kind,w_mode", [("tensor", 4), ("int", 3), ("none", 2)], ids=["scales+zeros", "scalar-zero", "no-zero"])
def test_one_group_per_metadata_mode(zeros_kind, w_mode, tdt):
    lins = [_layer_mode(4096, 4096, 128, tdt, 700 + i, zeros_kind) for i in range(5)]
    assert lins[0].W_group_mode == w_mode
    assert kernel_name(plan_args(lins[0], 1)).startswith("gemv_w4_decode3_kernel")
    x = _x(4096, tdt, seed=71)
    want = _eager(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 5 and joined == 4
    for o in outs:
        o.fill_(float("nan"))
    _replay(g, 2)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} ({zeros_kind}, {tdt})"


@pytest.mark.parametrize("N,members", [(4096, 5), (1024, 7)], ids=["one-block", "grid-y"])
def test_adjacent_outputs_of_one_allocation_and_the_guard_bytes_around_them(N, members):
    """Every member has its own x; the outs are adjacent rows of ONE allocation between 0xFF guard bytes: a store into another
    member's row shows as a wrong row, a store outside every out as a changed guard byte."""
    K, tdt, guard = 4096, torch.float16, 512
    lins = [_layer(N, K, 128, tdt, seed=800 + i) for i in range(members)]
    xs = [_x(K, tdt, seed=850 + i) for i in range(members)]
    want = [lin(x).clone() for lin, x in zip(lins, xs)]
    torch.cuda.synchronize()
    buf = torch.empty(guard + members * N + guard, dtype=tdt, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    lib = _hip.load()
    calls = []
    for i, (lin, x) in enumerate(zip(lins, xs)):
        a = plan_args(lin, 1, x=x.data_ptr(), out=buf[guard + i * N:].data_ptr(), stride_xm=K, stride_om=N)
        assert kernel_name(a).startswith("gemv_w4_decode3_kernel") and lib.gemlite_hip_workspace_bytes(C.byref(a)) == 0
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


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_members_of_six_magnitudes_and_one_with_a_nan_keep_to_themselves(tdt):
    """The per-wave-x form: every member has its own x, one activation profile of test_magnitude_range_gpu each (amplitude 1e-4 beside
    amplitude 10 in one block), and member 2 carries a NaN.  Every member, the poisoned one included, equals its eager launch as raw bits."""
    from tests.test_magnitude_range_gpu import PROFILES, profile_row
    N = K = 4096
    members = min(6, _gmax())
    lins = [_layer(N, K, 128, tdt, seed=900 + i) for i in range(members)]
    rng = np.random.default_rng(9)
    xs = [torch.from_numpy(profile_row(PROFILES[i], K, rng)).to(tdt).view(1, K).to(DEV) for i in range(members)]
    xs[2][0, 1234] = float("nan")
    want = [lin(x).clone() for lin, x in zip(lins, xs)]
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(want[2]).any()) and all(bool(torch.isfinite(w).all()) for i, w in enumerate(want) if i != 2)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in zip(lins, xs)])
    assert seen == members and joined == members - 1
    assert _hip.load().gemlite_hip_capture_group_last_form() == 1  # per-wave x
    for o in outs:
        o.zero_()
    _replay(g, 2)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o.view(torch.int16), w.view(torch.int16)), f"member {i} ({PROFILES[i]})"
