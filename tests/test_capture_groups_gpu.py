"""Capture-time grouping of the M = 1 decode kernel on the GPU (gemlite_amd/csrc/capture_group.hip): back-to-back independent
`layer(x)` calls of one stream capture become one grouped launch.  Every comparison is BIT-EXACT (torch.equal) against the eager
output of the same layer, and the library's counters say how many calls joined a node instead of adding one."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip
from oracle import gemlite_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gmax():
    return _hip.load().gemlite_hip_capture_group_max()


def _stats():
    seen, joined = C.c_uint64(0), C.c_uint64(0)
    _hip.load().gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    return seen.value, joined.value


def _layer(N, K, gs, tdt, seed):
    W_q, scales, zeros = O.gen_data(N, K, 4, gs, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, gs, K, N, code, code)
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV),
             torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV), None, fma_mode=True)
    return lin


def _x(K, tdt, seed):
    return torch.from_numpy(O.gen_x(1, K, seed=seed)).to(tdt).to(DEV)


def _capture(step):
    """Warm `step` up on a side stream (workspace, launch templates), capture it there, and report what the capture did:
    (graph, what step() returned under capture, decode launches seen, launches joined)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    seen0, joined0 = _stats()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        outs = step()
    seen1, joined1 = _stats()
    return g, outs, seen1 - seen0, joined1 - joined0


def _replay(g, times=3):
    for _ in range(times):
        g.replay()
    torch.cuda.synchronize()


def _eager(lins, x):
    ys = [lin(x).clone() for lin in lins]
    torch.cuda.synchronize()
    return ys


@pytest.mark.parametrize("tdt", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
def test_eight_independent_layers_become_one_launch(tdt):
    lins = [_layer(4096, 4096, 128, tdt, seed=10 + i) for i in range(8)]
    x = _x(4096, tdt, seed=3)
    want = _eager(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 8 and joined == min(8, _gmax()) - 1
    for o in outs:
        o.zero_()
    _replay(g, 3)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i}"


def test_more_layers_than_a_group_holds_split_into_two_nodes():
    n = _gmax() + 3
    lins = [_layer(4096, 4096, 128, torch.float16, seed=30 + i) for i in range(n)]
    x = _x(4096, torch.float16, seed=4)
    want = _eager(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == n and joined == _gmax() + 1  # (GMAX - 1) + 2
    _replay(g)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i}"


def test_replays_follow_a_new_x():
    lins = [_layer(4096, 4096, 128, torch.float16, seed=50 + i) for i in range(4)]
    x = _x(4096, torch.float16, seed=5)
    x_new = _x(4096, torch.float16, seed=6)
    want, want_new = _eager(lins, x), _eager(lins, x_new)
    assert not torch.equal(want[0], want_new[0])
    g, outs, _, joined = _capture(lambda: [lin(x) for lin in lins])
    assert joined == min(4, _gmax()) - 1
    _replay(g, 1)
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
    x.copy_(x_new)
    _replay(g, 1)
    for o, w in zip(outs, want_new):
        assert torch.equal(o, w)


def test_a_dependent_chain_is_captured_node_for_node():
    lin1 = _layer(4096, 4096, 128, torch.float16, seed=60)
    lin2 = _layer(4096, 4096, 128, torch.float16, seed=61)
    x = _x(4096, torch.float16, seed=7)
    want = lin2(lin1(x)).clone()
    torch.cuda.synchronize()
    g, out, seen, joined = _capture(lambda: lin2(lin1(x)))
    assert seen == 2 and joined == 0
    _replay(g)
    assert torch.equal(out, want)


def test_a_torch_op_between_two_independent_calls_keeps_them_apart():
    lin1 = _layer(4096, 4096, 128, torch.float16, seed=62)
    lin2 = _layer(4096, 4096, 128, torch.float16, seed=63)
    x = _x(4096, torch.float16, seed=8)
    want = _eager([lin1, lin2], x)

    def step():
        y1 = lin1(x)
        t = x * 2
        y2 = lin2(x)
        return y1, y2, t

    g, (y1, y2, t), seen, joined = _capture(step)
    assert seen == 2 and joined == 0
    _replay(g)
    assert torch.equal(y1, want[0]) and torch.equal(y2, want[1]) and torch.equal(t, x * 2)


def test_a_freed_output_block_may_be_reused_by_the_next_call():
    lin1 = _layer(4096, 4096, 128, torch.float16, seed=64)
    lin2 = _layer(4096, 4096, 128, torch.float16, seed=65)
    x = _x(4096, torch.float16, seed=9)
    want = _eager([lin2], x)[0]

    def step():
        y1 = lin1(x)
        del y1
        return lin2(x)

    g, y2, seen, joined = _capture(step)
    assert seen == 2 and joined in (0, 1)  # 0 when the allocator hands y1's block to y2: the outputs overlap
    _replay(g)
    assert torch.equal(y2, want)


def test_only_identical_neighbours_join():
    f16, b16 = torch.float16, torch.bfloat16
    spec = [(4096, 4096, 128, f16), (4096, 4096, 128, f16),     # joins
            (4096, 11008, 128, f16), (4096, 11008, 128, f16),   # another shape: new node, then joins
            (4096, 4096, 64, f16),                              # another group size
            (4096, 4096, 128, b16), (4096, 4096, 128, b16),     # another dtype: new node, then joins
            (4096, 4096, 128, f16),                             # back to the first kind, alone
            (11008, 4096, 128, f16), (11008, 4096, 128, f16)]   # a shape another GEMV kernel runs: never grouped
    lins = [_layer(N, K, gs, tdt, seed=70 + i) for i, (N, K, gs, tdt) in enumerate(spec)]
    xs = {(K, tdt): _x(K, tdt, seed=11) for (_, K, _, tdt) in spec}
    pairs = [(lin, xs[(K, tdt)]) for lin, (_, K, _, tdt) in zip(lins, spec)]
    want = [lin(x).clone() for lin, x in pairs]
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in pairs])
    assert seen == 8 and joined == 3
    _replay(g)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i} {spec[i]}"


def test_long_k_layers_group_like_the_square_ones():
    lins = [_layer(4096, 11008, 128, torch.float16, seed=90 + i) for i in range(8)]
    x = _x(11008, torch.float16, seed=12)
    want = _eager(lins, x)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 8 and joined == min(8, _gmax()) - 1
    _replay(g)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o, w), f"layer {i}"


def test_eager_calls_leave_the_counters_alone():
    lins = [_layer(4096, 4096, 128, torch.float16, seed=100 + i) for i in range(3)]
    x = _x(4096, torch.float16, seed=13)
    before = _stats()
    a = _eager(lins, x)
    b = _eager(lins, x)
    assert _stats() == before
    for p, q in zip(a, b):
        assert torch.equal(p, q)


_CHILD = r"""
import ctypes as C, sys, torch
sys.path.insert(0, {root!r})
from tests.test_capture_groups_gpu import _layer, _x, _eager, _capture, _replay, _gmax
lins = [_layer(4096, 4096, 128, torch.float16, seed=110 + i) for i in range(4)]
x = _x(4096, torch.float16, seed=14)
want = _eager(lins, x)
g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
_replay(g)
print("RESULT", _gmax(), seen, joined, all(torch.equal(o, w) for o, w in zip(outs, want)))
"""


def test_the_kill_switch_turns_grouping_off():
    env = dict(os.environ, GEMLITE_HIP_NO_CAPTURE_GROUPS="1")
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert line[1:] == ["1", "0", "0", "True"], line  # limit 1, nothing counted, nothing joined, equal to eager
