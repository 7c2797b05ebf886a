"""Capture-time grouping of the few-row rows kernel on the GPU (gemlite_amd/csrc/capture_group.hip, gemm_wn_rows_group.hip): back-to-back
independent `layer(x)` calls with 2 .. 64 rows in one stream capture become one launch of gemm_w4_rows_group_kernel, grid (tiles, members).
Every comparison is BIT-EXACT (torch.equal) against the eager output of the same layer, outputs are zeroed before the replays, and the
library's counters say how many calls joined a node instead of adding one.

Shapes, the smallest at which the kernel's branches still differ: 272 x 512 (17 tiles: no XCD pair map; 2 chunks: six of the eight waves
own none; 2-bit: one chunk), 256 x 4096 (16 tiles: the pair map, beside grid.y > 1; 16 chunks), 288 x 1024 with tuning (9, 2, 0, 0)
(the two-column-tile form).  The small shapes are forced onto the rows kernel (tuning[0] = 9) and ASSERT the kernel name."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from oracle import gemlite_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, B16 = torch.float16, torch.bfloat16
FORCE = (9, 0, 0, 0)      # GEMLITE_T0_ROWS_KERNEL
FORCE_NT2 = (9, 2, 0, 0)  # ... with two column tiles per block


@pytest.fixture(autouse=True)
def _switch_back():
    yield
    core.FUSE_BIAS = True
    core.TUNING_OVERRIDE = None


def _gmax():
    return _hip.load().gemlite_hip_capture_group_max()


def _stats():
    seen, joined = C.c_uint64(0), C.c_uint64(0)
    _hip.load().gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    return seen.value, joined.value


_LAYERS = {}


def _layer(N, K, tdt=F16, seed=0, nbits=4, gs=128, bias=False):
    """A packed layer (bias: a random one, or none); layers are built once per process, shared by the tests and never changed"""
    key = (N, K, tdt, seed, nbits, gs, bias)
    if key not in _LAYERS:
        W_q, scales, zeros = O.gen_data(N, K, nbits, gs, seed=seed, np_float=np.float16)
        code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
        lin = GemLiteLinear(nbits, gs, K, N, code, code)
        b = (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.5).to(tdt).to(DEV) if bias else None
        lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV),
                 torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV), b, fma_mode=True)
        _LAYERS[key] = lin
    return _LAYERS[key]


def _x(M, K, tdt, seed):
    return torch.from_numpy(O.gen_x(M, K, seed=seed)).to(tdt).to(DEV)


def _name(lin, x):
    """the kernel the library plans for the unbiased launch of layer(x) under the current core.TUNING_OVERRIDE"""
    W_q, scales, zeros = lin.get_tensor_args()
    a = core._call_args(x, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, 0x1000, (W_q.shape[1], 1))
    return _hip.load().gemlite_hip_kernel_name(C.byref(a)).decode()


def _rows_or_skip(lin, x, nbits=4):
    """Forced cases assert the rows kernel; the default-planned ones may find the planner routing elsewhere"""
    name, prefix = _name(lin, x), f"gemm_w{nbits}_rows_kernel<"
    if core.TUNING_OVERRIDE is not None:
        assert name.startswith(prefix), name
    elif not name.startswith(prefix):
        pytest.skip(f"PLANNER ROUTES ELSEWHERE: {name} instead of {prefix}: this case checks nothing")
    return name


def _capture(step):
    """Warm `step` up on a side stream, capture it there: (graph, what step() returned, launches seen, launches joined)"""
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


def _eager(pairs, fuse=True):
    core.FUSE_BIAS = fuse
    try:
        ys = [lin(x).clone() for lin, x in pairs]
    finally:
        core.FUSE_BIAS = True
    torch.cuda.synchronize()
    return ys


def _replay_and_compare(g, outs, want, times=3):
    for o in outs:
        o.zero_()
    for _ in range(times):
        g.replay()
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert o.shape == w.shape and torch.equal(o, w), f"member {i}"


# ---- 1. n independent layers on one x are one node ------------------------------------------------------------------------------------
# (N, K, tuning, M, gs, nbits, dtype, members; -1 = the member limit): every M, group size, bit width, dtype, shape and n at least once
CASES = [
    (272, 512, FORCE, 2, 128, 4, F16, 2),
    (272, 512, FORCE, 17, 64, 4, B16, 3),
    (272, 512, FORCE, 16, 32, 4, F16, -1),
    (272, 512, FORCE, 17, 64, 2, F16, 2),
    (256, 4096, FORCE, 33, 128, 4, F16, -1),
    (256, 4096, FORCE, 64, 128, 2, B16, 3),
    (256, 4096, FORCE, 17, 32, 4, B16, 2),
    (256, 4096, FORCE, 64, 64, 4, F16, 3),
    (288, 1024, FORCE_NT2, 33, 128, 4, F16, 3),
    (288, 1024, FORCE_NT2, 64, 128, 4, B16, -1),
    (288, 1024, FORCE_NT2, 17, 64, 4, F16, 2),
    (1024, 4096, None, 16, 128, 4, F16, 4),
    (4096, 4096, None, 8, 128, 4, F16, 3),
]


def _case_id(c):
    N, K, tun, M, gs, nbits, tdt, n = c
    return f"{N}x{K}{'_nt2' if tun == FORCE_NT2 else ('' if tun else '_default')}_M{M}_g{gs}_w{nbits}_{'fp16' if tdt == F16 else 'bf16'}_n{'max' if n < 0 else n}"


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_independent_layers_on_one_x_become_one_node(case):
    N, K, tun, M, gs, nbits, tdt, n = case
    n = _gmax() if n < 0 else n
    core.TUNING_OVERRIDE = tun
    lins = [_layer(N, K, tdt, seed=10 + i, nbits=nbits, gs=gs) for i in range(n)]
    x = _x(M, K, tdt, seed=3)
    name = _rows_or_skip(lins[0], x, nbits)
    mt = (M + 15) // 16
    assert name.endswith(f"<{16 * mt}x{32 if tun == FORCE_NT2 else 16}>"), name
    want = _eager([(lin, x) for lin in lins])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == n and joined == min(n, _gmax()) - 1
    assert _hip.load().gemlite_hip_capture_group_last_form() == 3
    _replay_and_compare(g, outs, want)


# ---- 2. more layers than a group holds ------------------------------------------------------------------------------------------------
def test_more_layers_than_a_group_holds_split_into_two_nodes():
    core.TUNING_OVERRIDE = FORCE
    n = _gmax() + 3
    lins = [_layer(272, 512, F16, seed=10 + i) for i in range(n)]
    x = _x(16, 512, F16, seed=4)
    _rows_or_skip(lins[0], x)
    want = _eager([(lin, x) for lin in lins])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == n and joined == _gmax() + 1  # (GMAX - 1) + 2
    _replay_and_compare(g, outs, want)


# ---- 3. every member its own x and out, adjacent slices between guard bytes -----------------------------------------------------------
def _launch(lin, x, out, bias=None):
    """One library call with the caller's output buffer (what core._hip_matmul does, minus the allocation)"""
    W_q, scales, zeros = lin.get_tensor_args()
    a = core._call_args(x, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, out.data_ptr(), (out.stride(0), out.stride(1)))
    stream = _hip.current_stream_handle(x.device)
    ws = _hip.workspace(x.device, stream, 0)
    a.workspace, a.workspace_bytes = ws.data_ptr(), ws.numel()
    ext = _hip.forward_ext(bias.data_ptr(), gemlite_amd.dtypes.TORCH_TO_DTYPE[bias.dtype].value) if bias is not None else None
    rc = _hip.load().gemlite_hip_forward_ex(C.byref(a), C.byref(ext) if ext is not None else None, stream)
    assert rc == 0, rc


@pytest.mark.parametrize("N,K,M,biased", [(272, 512, 17, False), (256, 4096, 33, True)], ids=["272x512_M17", "256x4096_M33_bias"])
def test_members_with_their_own_x_and_out_between_guard_bytes(N, K, M, biased):
    """A member table indexed off by one reads a neighbour's x or writes a neighbour's out (or the guard)."""
    core.TUNING_OVERRIDE = FORCE
    n, guard = 5, 256  # guard: 16-bit elements on either side
    lins = [_layer(N, K, F16, seed=10 + i, bias=biased) for i in range(n)]
    xbuf = torch.full((2 * guard + n * M * K,), -1, dtype=torch.int16, device=DEV).view(F16)
    obuf = torch.full((2 * guard + n * M * N,), -1, dtype=torch.int16, device=DEV).view(F16)
    xs = [xbuf[guard + i * M * K: guard + (i + 1) * M * K].view(M, K) for i in range(n)]
    outs = [obuf[guard + i * M * N: guard + (i + 1) * M * N].view(M, N) for i in range(n)]
    for i, x in enumerate(xs):
        x.copy_(_x(M, K, F16, seed=20 + i))
    _rows_or_skip(lins[0], xs[0])
    want = _eager(list(zip(lins, xs)), fuse=False)
    assert not torch.equal(want[0], want[1])
    xbuf_before = xbuf.view(torch.int16).clone()

    def step():
        for lin, x, o in zip(lins, xs, outs):
            _launch(lin, x, o, lin.bias if biased else None)
        return outs

    g, _, seen, joined = _capture(step)
    assert seen == n and joined == n - 1
    _replay_and_compare(g, outs, want)
    raw = obuf.view(torch.int16)
    assert bool((raw[:guard] == -1).all()) and bool((raw[-guard:] == -1).all()), "a store outside the members' outputs"
    assert torch.equal(xbuf.view(torch.int16), xbuf_before)


@pytest.mark.parametrize("N,K,M,tdt", [(272, 512, 17, F16), (256, 4096, 33, B16)], ids=["272x512_M17_fp16", "256x4096_M33_bf16"])
def test_members_of_five_magnitudes_and_one_with_a_nan_keep_to_themselves(N, K, M, tdt):
    """Every member has its own x, all rows of one activation profile of test_magnitude_range_gpu (amplitude 1e-4 beside amplitude 10 in
    one launch), and one row of member 2 carries a NaN.  Every member, the poisoned one included, equals its eager launch as raw bits."""
    from tests.test_magnitude_range_gpu import PROFILES, profile_row
    core.TUNING_OVERRIDE = FORCE
    n = 5
    lins = [_layer(N, K, tdt, seed=10 + i) for i in range(n)]
    rng = np.random.default_rng(M)
    xs = [torch.from_numpy(np.stack([profile_row(PROFILES[i], K, rng) for _ in range(M)])).to(tdt).to(DEV) for i in range(n)]
    xs[2][M // 2, K // 3] = float("nan")
    _rows_or_skip(lins[0], xs[0])
    want = _eager(list(zip(lins, xs)))
    bad = ~torch.isfinite(want[2]).all(dim=1)
    assert bad.tolist() == [m == M // 2 for m in range(M)] and all(bool(torch.isfinite(w).all()) for i, w in enumerate(want) if i != 2)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in zip(lins, xs)])
    assert seen == n and joined == n - 1
    for o in outs:
        o.zero_()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for i, (o, w) in enumerate(zip(outs, want)):
        assert torch.equal(o.view(torch.int16), w.view(torch.int16)), f"member {i} ({PROFILES[i]})"


# ---- 4. a replay follows a new x ------------------------------------------------------------------------------------------------------
def test_replays_follow_a_new_x():
    core.TUNING_OVERRIDE = FORCE
    lins = [_layer(272, 512, F16, seed=10 + i) for i in range(4)]
    x, x_new = _x(33, 512, F16, seed=5), _x(33, 512, F16, seed=6)
    _rows_or_skip(lins[0], x)
    want, want_new = _eager([(lin, x) for lin in lins]), _eager([(lin, x_new) for lin in lins])
    assert not torch.equal(want[0], want_new[0])
    g, outs, _, joined = _capture(lambda: [lin(x) for lin in lins])
    assert joined == min(4, _gmax()) - 1
    _replay_and_compare(g, outs, want, times=1)
    x.copy_(x_new)
    _replay_and_compare(g, outs, want_new, times=1)


# ---- 5. / 6. what must stay apart -----------------------------------------------------------------------------------------------------
def test_a_dependent_chain_is_captured_node_for_node():
    core.TUNING_OVERRIDE = FORCE
    lin1, lin2 = _layer(512, 512, F16, seed=60), _layer(512, 512, F16, seed=61)
    x = _x(16, 512, F16, seed=7)
    _rows_or_skip(lin1, x)
    want = lin2(lin1(x)).clone()
    torch.cuda.synchronize()
    g, out, seen, joined = _capture(lambda: lin2(lin1(x)))
    assert seen == 2 and joined == 0
    _replay_and_compare(g, [out], [want])


def test_a_torch_op_between_two_independent_calls_keeps_them_apart():
    core.TUNING_OVERRIDE = FORCE
    lin1, lin2 = _layer(272, 512, F16, seed=10), _layer(272, 512, F16, seed=11)
    x = _x(16, 512, F16, seed=8)
    _rows_or_skip(lin1, x)
    want = _eager([(lin1, x), (lin2, x)])

    def step():
        y1 = lin1(x)
        t = x * 2
        y2 = lin2(x)
        return y1, y2, t

    g, (y1, y2, t), seen, joined = _capture(step)
    assert seen == 2 and joined == 0
    _replay_and_compare(g, [y1, y2, t], want + [x * 2])


# ---- 7. biased layers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,K,M,tdt,nbits", [(272, 512, 17, F16, 4), (256, 4096, 64, B16, 2)], ids=["272x512_M17_w4_fp16", "256x4096_M64_w2_bf16"])
def test_four_biased_layers_are_one_node_and_equal_matmul_then_add(N, K, M, tdt, nbits):
    core.TUNING_OVERRIDE = FORCE
    lins = [_layer(N, K, tdt, seed=10 + i, nbits=nbits, bias=True) for i in range(4)]
    x = _x(M, K, tdt, seed=3)
    _rows_or_skip(lins[0], x, nbits)
    want = _eager([(lin, x) for lin in lins], fuse=False)
    assert not torch.equal(want[0], want[0] - lins[0].bias), "the bias is in"
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 4 and joined == min(4, _gmax()) - 1
    _replay_and_compare(g, outs, want)


def test_biased_unbiased_biased_neighbours_are_three_nodes():
    core.TUNING_OVERRIDE = FORCE
    lins = [_layer(272, 512, F16, seed=10, bias=True), _layer(272, 512, F16, seed=11), _layer(272, 512, F16, seed=12, bias=True)]
    x = _x(16, 512, F16, seed=8)
    _rows_or_skip(lins[1], x)
    want = _eager([(lin, x) for lin in lins], fuse=False)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 3 and joined == 0
    _replay_and_compare(g, outs, want)


def test_a_layer_whose_bias_is_the_previous_output_does_not_join():
    core.TUNING_OVERRIDE = FORCE
    lin1, lin2 = _layer(272, 512, F16, seed=10, bias=True), _layer(272, 512, F16, seed=11)
    x = _x(16, 512, F16, seed=7)
    _rows_or_skip(lin2, x)

    def step():
        y1 = lin1(x)
        y2 = core._forward_impl(x, y1[0], lin2.get_tensor_args(), lin2.get_meta_args(), -1)  # dependent THROUGH the bias
        return y1, y2

    core.FUSE_BIAS = False
    y1w, y2w = (y.clone() for y in step())
    core.FUSE_BIAS = True
    torch.cuda.synchronize()
    g, outs, seen, joined = _capture(step)
    assert seen == 2 and joined == 0
    _replay_and_compare(g, outs, [y1w, y2w])


# ---- 8. both families in one capture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Ms,joins", [((1, 8, 8), 1), ((8, 1, 1), 1), ((8, 16), 0)], ids=["M1_M8_M8", "M8_M1_M1", "M8_M16"])
def test_the_two_families_never_mix(Ms, joins):
    """Default planning on one shape: M = 1 runs the decode kernel, M = 8 / 16 the rows kernel (the same function, another M)."""
    N = K = 4096
    lins = [_layer(N, K, F16, seed=10 + i) for i in range(len(Ms))]
    xs = {M: _x(M, K, F16, seed=30 + M) for M in set(Ms)}
    for M in set(Ms):
        if M == 1:
            if not _name(lins[0], xs[1]).startswith("gemv_w4_decode3_kernel<"):
                pytest.skip("PLANNER ROUTES ELSEWHERE: M = 1 does not run the decode kernel")
        else:
            _rows_or_skip(lins[0], xs[M])
    pairs = [(lin, xs[M]) for lin, M in zip(lins, Ms)]
    want = _eager(pairs)
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin, x in pairs])
    assert seen == len(Ms) and joined == joins
    _replay_and_compare(g, outs, want)


# ---- 9. launches with row blocks ------------------------------------------------------------------------------------------------------
def test_launches_with_row_blocks_stay_their_own():
    core.TUNING_OVERRIDE = FORCE
    lins = [_layer(272, 512, F16, seed=10 + i) for i in range(2)]
    x = _x(80, 512, F16, seed=9)
    assert _rows_or_skip(lins[0], x).endswith("<64x16>")  # 80 rows: two row blocks along grid.y
    want = _eager([(lin, x) for lin in lins])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    assert seen == 2 and joined == 0
    _replay_and_compare(g, outs, want)


# ---- 10. the switch of this family ----------------------------------------------------------------------------------------------------
def _switch_step():
    """The step of the switch test (parent and child): (seen, joined, checksum of the outputs, equal to eager) of three forced rows layers,
    then the joins of three M = 1 decode layers"""
    core.TUNING_OVERRIDE = FORCE
    lins = [_layer(272, 512, F16, seed=10 + i) for i in range(3)]
    x = _x(17, 512, F16, seed=3)
    assert _name(lins[0], x).startswith("gemm_w4_rows_kernel<")
    want = _eager([(lin, x) for lin in lins])
    g, outs, seen, joined = _capture(lambda: [lin(x) for lin in lins])
    _replay_and_compare(g, outs, want)
    digest = hashlib.sha256(b"".join(o.cpu().numpy().tobytes() for o in outs)).hexdigest()
    core.TUNING_OVERRIDE = None
    dl = [_layer(512, 4096, F16, seed=40 + i) for i in range(3)]
    x1 = _x(1, 4096, F16, seed=4)
    assert _name(dl[0], x1).startswith("gemv_w4_decode3_kernel<")
    want1 = _eager([(lin, x1) for lin in dl])
    g1, outs1, seen1, joined1 = _capture(lambda: [lin(x1) for lin in dl])
    _replay_and_compare(g1, outs1, want1)
    return seen, joined, digest, joined1


_CHILD = r"""
import sys
sys.path.insert(0, {root!r})
from tests.test_rows_groups_gpu import _switch_step
print("RESULT", *_switch_step())
"""


def test_the_rows_switch_keeps_only_this_family_ungrouped():
    seen, joined, digest, joined1 = _switch_step()
    assert (seen, joined, joined1) == (3, min(3, _gmax()) - 1, min(3, _gmax()) - 1)
    env = dict(os.environ, GEMLITE_HIP_CAPTURE_GROUP_ROWS="0")
    out = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    line = [l for l in out.stdout.splitlines() if l.startswith("RESULT")][-1].split()
    assert line[2] == "0", line                  # no rows launch joined
    assert line[3] == digest, line               # the same bytes as the grouped run
    assert line[4] == str(joined1), line         # the M = 1 family still groups
