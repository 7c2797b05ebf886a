"""gemlite_hip_experts_topk on the GPU against the float64 restatement (tests/experts_topk_spec.py): ids bit for bit wherever the key is
exact, weights within a measured bound, the exact relations between two launches, non-finite rows, guard bands, graph replay, and the
router in front of the expert MLP."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gemlite_amd import ExpertsRouter, GemLiteExperts, GemLiteExpertsMLP, _hip, experts_topk
from gemlite_amd.dtypes import TORCH_TO_DTYPE
from tests import experts_topk_spec as spec
from tests.test_experts_cpu import make_layers

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256
# The largest relative error of an fp32 weight against the float64 restatement over test_ids_are_exact_and_weights_lie_within_the_bound
# and test_sigmoid_with_a_selection_bias (|logit| <= 16, E up to 1024) measured on an MI355X: 2.94e-7 (softmax over all experts, E = 128; softmax
# with renormalize 1.7e-7, sigmoid with renormalize 1.9e-7 with a bias and 1.4e-7 without, plain sigmoid 1.1e-7).  The bound is 4 x that —
# the order of the lane sums and the exponential's last bits are free — and stays below 1e-4 ((E + |l|max) 2^-24 at E = 1024 is 6e-5).
WEIGHT_RTOL = 4 * 2.94e-7
T_MAX = 257
MODES = (("softmax", True), ("softmax", False), ("sigmoid", True), ("sigmoid", False))


def ks_of(E):
    return sorted({min(k, E) for k in (1, 2, 8, min(E, 64))})


@functools.lru_cache(maxsize=None)
def logits_of(E, dtype):
    """(the CPU tensor, its copy on the GPU): T_MAX tie-free rows, |l| <= 16; never modified."""
    cpu = spec.tie_free_logits(T_MAX, E, dtype, seed=E + 1)
    return cpu, cpu.to(DEV)


@functools.lru_cache(maxsize=None)
def want_of(E, dtype, k, scoring, renorm):
    return spec.topk(logits_of(E, dtype)[0], k, scoring, renorm)


def rel_err(w, want):
    w = w.detach().cpu().double().numpy().reshape(want.shape)
    return float(np.max(np.abs(w - want) / np.abs(want)))


def same_ids(ids, want):
    return np.array_equal(ids.detach().cpu().numpy().reshape(want.shape).astype(np.int64), want)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 128, 160, 1024])
def test_ids_are_exact_and_weights_lie_within_the_bound(E, dtype):
    _, l = logits_of(E, dtype)
    worst = {}
    for k in ks_of(E):
        for scoring, renorm in MODES:
            want_ids, want_w = want_of(E, dtype, k, scoring, renorm)
            for T in (1, 4, 5, T_MAX):
                ids, w = experts_topk(l[:T], k, scoring, renorm)
                assert ids.dtype == torch.int32 and w.dtype == torch.float32 and tuple(ids.shape) == tuple(w.shape) == (T, k)
                assert same_ids(ids, want_ids[:T]), (E, k, scoring, renorm, T)
                ids64, w2 = experts_topk(l[:T], k, scoring, renorm, ids_dtype=torch.int64)
                assert ids64.dtype == torch.int64 and torch.equal(ids64, ids.long()) and torch.equal(w2, w)
                err = rel_err(w, want_w[:T])
                worst[(scoring, renorm)] = max(worst.get((scoring, renorm), 0.0), err)
    print(f"experts_topk E={E} {dtype}: largest relative weight error per mode {worst}")
    assert max(worst.values()) <= WEIGHT_RTOL, worst


def tie_rows(E, dtype):
    """Rows full of ties: all equal; a tie across every k-th / (k+1)-th place (a few distinct values); -inf; signed zeros."""
    g = torch.Generator().manual_seed(E)
    rows = [torch.full((E,), 0.75), torch.zeros(E), -torch.zeros(E)]
    few = torch.tensor([-1.0, 0.0, 0.5, 2.0])
    rows += [few[torch.randint(0, 4, (E,), generator=g)] for _ in range(3)]
    for k in ks_of(E):  # exactly k - 1 experts above a plateau that spans the k-th and the following places
        r = torch.full((E,), 1.0)
        r[torch.randperm(E, generator=g)[:max(k - 1, 0)]] = 3.0
        rows.append(r)
    r = few[torch.randint(0, 4, (E,), generator=g)].clone()
    r[torch.randperm(E, generator=g)[:E // 2]] = float("-inf")
    rows += [r, torch.full((E,), float("-inf"))]
    z = torch.zeros(E)
    z[::2] = -0.0
    rows.append(z)
    return torch.stack(rows).to(dtype)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("E", [1, 63, 65, 160, 1024])
def test_ties_go_to_the_lower_index_and_minus_infinity_ranks_last(E, dtype):
    cpu = tie_rows(E, dtype)
    l = cpu.to(DEV)
    for k in ks_of(E):
        for scoring in ("softmax", "sigmoid"):
            want_ids, _ = spec.topk(cpu, k, scoring, True)
            for idt in (torch.int32, torch.int64):
                ids, _ = experts_topk(l, k, scoring, True, ids_dtype=idt)
                assert same_ids(ids, want_ids), (E, k, scoring, idt)
    # an all-equal row selects 0 .. k - 1 with equal weights
    ids, w = experts_topk(l[:1], ks_of(E)[-1])
    assert ids[0].tolist() == list(range(ks_of(E)[-1])) and bool((w == w[0, 0]).all())


@pytest.mark.parametrize("E,seed", [(64, 0), (160, 0), (256, 14)])
def test_sigmoid_with_a_selection_bias(E, seed):
    cpu = spec.grid_logits(9, E, torch.float16, seed)
    bias = spec.eighths_bias(E, seed)
    key = np.sort(spec.keys(cpu, "sigmoid", bias), axis=-1)
    gap = float(np.diff(key, axis=-1).min())
    print(f"experts_topk sigmoid + bias E={E}: smallest float64 key gap {gap:.3e}")
    assert gap >= 1e-5  # the fp32 key error is about 4e-7: the selection is decided
    l, b = cpu.to(DEV), bias.to(DEV)
    worst = 0.0
    for k in ks_of(E):
        for renorm in (True, False):
            for scale in (1.0, 2.5):
                want_ids, want_w = spec.topk(cpu, k, "sigmoid", renorm, scale, bias)
                ids, w = experts_topk(l, k, "sigmoid", renorm, scale, b)
                assert same_ids(ids, want_ids), (E, k, renorm)
                worst = max(worst, rel_err(w, want_w))
    print(f"experts_topk sigmoid + bias E={E}: largest relative weight error {worst:.3e}")
    assert worst <= WEIGHT_RTOL
    # the bias decides who is selected and never enters a weight
    ids0, w0 = experts_topk(l, 8, "sigmoid", False, 1.0, None)
    ids1, w1 = experts_topk(l, 8, "sigmoid", False, 1.0, b)
    assert not torch.equal(ids0, ids1)
    no_bias_at_ids1 = np.take_along_axis(spec.sigmoid64(spec.to_f64(cpu)), ids1.cpu().numpy().astype(np.int64), axis=-1)
    assert rel_err(w1, no_bias_at_ids1) <= WEIGHT_RTOL and same_ids(ids0, spec.topk(cpu, 8, "sigmoid", False)[0])


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_exact_relations_between_two_launches(dtype):
    for E, k in ((65, 8), (160, 6), (1024, 64)):
        _, l = logits_of(E, dtype)
        l = l[:21]
        b = spec.eighths_bias(E, 3).to(DEV)
        for scoring, renorm, bias in (("softmax", True, None), ("softmax", False, None), ("sigmoid", True, b), ("sigmoid", False, None)):
            ids, w = experts_topk(l, k, scoring, renorm, 1.0, bias)
            # 16-bit weights are the fp32 weights rounded once
            for wdt in (torch.float16, torch.bfloat16):
                ids16, w16 = experts_topk(l, k, scoring, renorm, 1.0, bias, weights_dtype=wdt)
                assert w16.dtype == wdt and torch.equal(ids16, ids) and torch.equal(w16, w.to(wdt)), (E, scoring, wdt)
            # a padded row stride, a sliced inner dimension and a 3-d batch give the bits of the contiguous call
            wide = torch.full((21, E + 7), 99.0, dtype=dtype, device=DEV)
            wide[:, 3:E + 3] = l
            for view in (wide[:, 3:E + 3], torch.stack([l, l], -1)[..., 0], l.reshape(3, 7, E)):
                ids_v, w_v = experts_topk(view, k, scoring, renorm, 1.0, bias)
                assert torch.equal(ids_v.reshape(21, k), ids) and torch.equal(w_v.reshape(21, k), w), (E, scoring)
            # scale = 2 doubles exactly; int64 ids are the int32 ids
            ids2, w2 = experts_topk(l, k, scoring, renorm, 2.0, bias, ids_dtype=torch.int64)
            assert torch.equal(w2, w * 2) and torch.equal(ids2, ids.long())


def check_ids_safe(ids, E):
    i = ids.detach().cpu().long()
    assert bool(((i >= 0) & (i < E)).all()), "an id outside [0, E)"
    assert all(len(set(r.tolist())) == i.shape[-1] for r in i.reshape(-1, i.shape[-1])), "a repeated id in one token"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32], ids=["fp16", "bf16", "fp32"])
@pytest.mark.parametrize("E", [64, 160, 1024])
def test_non_finite_rows_give_distinct_ids_in_range_and_leave_the_other_rows_alone(E, dtype):
    inf, nan = float("inf"), float("nan")
    cpu = logits_of(E, dtype)[0][:12].clone()
    g = torch.Generator().manual_seed(5)
    cpu[1] = nan                                            # all NaN
    cpu[3, torch.randperm(E, generator=g)[:E // 3]] = nan  # NaN among numbers
    cpu[5, torch.randperm(E, generator=g)[:3]] = inf        # +inf: softmax gives inf - inf
    cpu[6] = -inf
    cpu[8, ::2], cpu[8, 1::2] = inf, nan
    big = torch.finfo(dtype).max if dtype == torch.float16 else 6e4
    cpu[10] = (torch.rand(E, generator=g) * 2 - 1) * big   # the largest fp16 logits: l - max stays finite, nothing overflows
    bad = [1, 3, 5, 6, 8]
    clean = cpu.clone()
    clean[bad] = 0.0
    l, lc = cpu.to(DEV), clean.to(DEV)
    b = (torch.randn(E, generator=g) * 0.1).to(DEV)
    bn = b.clone()
    bn[::5] = nan
    bn[1::7] = inf
    good = [r for r in range(12) if r not in bad]
    for k in ks_of(E):
        for scoring, renorm, bias in (("softmax", True, None), ("softmax", False, None), ("sigmoid", True, None), ("sigmoid", True, b),
                                      ("sigmoid", False, bn)):
            ids, w = experts_topk(l, k, scoring, renorm, 1.0, bias)
            check_ids_safe(ids, E)
            if bias is None:  # the key is exact: the pinned order holds on these rows too
                assert same_ids(ids, spec.topk(cpu, k, scoring, renorm)[0]), (E, k, scoring)
            ids_c, w_c = experts_topk(lc, k, scoring, renorm, 1.0, bias)
            assert torch.equal(ids[good], ids_c[good]) and torch.equal(w[good], w_c[good]), (E, k, scoring)
            if bias is not bn:
                assert bool(torch.isfinite(w[good]).all())
    # row 10: fp32 arithmetic on the largest logits stays finite and sums to one
    _, w = experts_topk(l[10:11], ks_of(E)[-1], "softmax", True)
    assert abs(float(w.sum()) - 1.0) < 1e-5


def c_call(l2, k, scoring, renorm, scale, bias, ids_view, w_view):
    t = _hip.ExpertsTopkArgs()
    t.struct_size = C.sizeof(_hip.ExpertsTopkArgs)
    t.logits_dtype, t.ids_dtype, t.weights_dtype = (TORCH_TO_DTYPE[v.dtype].value for v in (l2, ids_view, w_view))
    t.scoring, t.renormalize, t.scale = {"softmax": 0, "sigmoid": 1}[scoring], int(renorm), scale
    t.logits, t.ids, t.weights = l2.data_ptr(), ids_view.data_ptr(), w_view.data_ptr()
    t.bias = None if bias is None else bias.data_ptr()
    t.n_tokens, t.n_experts, t.top_k, t.stride_logits_token = l2.shape[0], l2.shape[1], k, l2.stride(0)
    rc = _hip.load().gemlite_hip_experts_topk(C.byref(t), _hip.current_stream_handle(l2.device))
    assert rc == _hip.OK, _hip.status_string(rc)


@pytest.mark.parametrize("idt,wdt", [(torch.int32, torch.float32), (torch.int64, torch.float16), (torch.int32, torch.bfloat16),
                                     (torch.int64, torch.float32)])
def test_guard_bands_around_both_outputs_stay_intact(idt, wdt):
    for E, k, T in ((1, 1, 1), (63, 2, 5), (65, 8, 257), (160, 64, 4), (1024, 64, 5), (1024, 1, 257)):
        _, l = logits_of(E, torch.float16)
        l = l[:T]
        for scoring, renorm in (("softmax", True), ("sigmoid", False)):
            ids_buf = torch.full((T * k + 2 * GUARD,), -77, dtype=idt, device=DEV)
            w_buf = torch.full((T * k + 2 * GUARD,), 7.25, dtype=wdt, device=DEV)
            c_call(l, k, scoring, renorm, 1.0, None, ids_buf[GUARD:], w_buf[GUARD:])
            torch.cuda.synchronize()
            for buf, canary in ((ids_buf, -77), (w_buf, 7.25)):
                assert bool((buf[:GUARD] == canary).all()) and bool((buf[-GUARD:] == canary).all()), (E, k, T, "written outside the output")
            ids, w = experts_topk(l, k, scoring, renorm, ids_dtype=idt, weights_dtype=wdt)
            assert torch.equal(ids_buf[GUARD:-GUARD].view(T, k), ids) and torch.equal(w_buf[GUARD:-GUARD].view(T, k), w)


def test_a_captured_call_follows_the_logits_of_every_replay():
    E, k, T = 128, 8, 5
    b = spec.eighths_bias(E, 1).to(DEV)
    l = logits_of(E, torch.bfloat16)[1][:T].clone()
    for scoring, bias in (("softmax", None), ("sigmoid", b)):
        experts_topk(l, k, scoring, True, 1.0, bias)  # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ids, w = experts_topk(l, k, scoring, True, 1.0, bias)
        for i in range(3):
            l.copy_(spec.tie_free_logits(T, E, torch.bfloat16, seed=100 + i).to(DEV))  # rewritten in place
            graph.replay()
            torch.cuda.synchronize()
            eager_ids, eager_w = experts_topk(l, k, scoring, True, 1.0, bias)
            assert torch.equal(ids, eager_ids) and torch.equal(w, eager_w), (scoring, i)
            if bias is None:
                assert same_ids(ids, spec.topk(l, k, scoring, True)[0])


@functools.lru_cache(maxsize=None)
def small_mlp():
    n = 8
    gate = make_layers(E=n, N=256, K=256, bias=False, device=DEV)
    up = make_layers(E=n, N=256, K=256, bias=False, seed=1, device=DEV)
    down = make_layers(E=n, N=256, K=256, bias=False, seed=2, device=DEV)
    return GemLiteExpertsMLP(GemLiteExperts.from_gate_up(gate, up), GemLiteExperts.from_layers(down))


@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_the_routed_mlp_is_the_mlp_on_the_routers_ids_and_weights(scoring):
    mlp = small_mlp()
    g = torch.Generator().manual_seed(11)
    bias = spec.eighths_bias(8, 2) if scoring == "sigmoid" else None
    router = ExpertsRouter(2, scoring, True, 1.0 if scoring == "softmax" else 2.5, bias).to(DEV)
    assert router.bias is None or router.bias.device.type == "cuda"
    for T in (1, 18):
        x = (torch.randn(T, 256, generator=g) * 0.5).half().to(DEV)
        logits = torch.randn(T, 8, generator=g).half().to(DEV)
        ids, w = experts_topk(logits, 2, scoring, True, router.scale, router.bias)
        assert ids.dtype == torch.int32 and w.dtype == torch.float32
        r_ids, r_w = router(logits)
        assert torch.equal(r_ids, ids) and torch.equal(r_w, w)
        assert torch.equal(mlp.forward_routed(x, logits, router), mlp(x, ids, w))
        assert torch.equal(mlp.forward_batched_fused_routed(x, logits, router), mlp.forward_batched_fused(x, ids, w))
        # weights in the activation type are taken too
        r16 = ExpertsRouter(2, scoring, True, router.scale, bias, weights_dtype=torch.float16).to(DEV)
        assert torch.equal(mlp.forward_routed(x, logits, r16), mlp(x, ids, w.half()))


def test_a_row_of_nan_logits_reaches_the_output_through_the_ordinary_path():
    mlp = small_mlp()
    g = torch.Generator().manual_seed(12)
    x = (torch.randn(6, 256, generator=g) * 0.5).half().to(DEV)
    logits = torch.randn(6, 8, generator=g).half().to(DEV)
    clean = mlp.forward_batched_fused_routed(x, logits, ExpertsRouter(2))
    logits[2] = float("nan")
    router = ExpertsRouter(2)
    ids, w = router(logits)
    check_ids_safe(ids, 8)
    assert ids[2].tolist() == [0, 1] and bool(torch.isnan(w[2]).all())
    keep = [0, 1, 3, 4, 5]
    for out in (mlp.forward_routed(x, logits, router), mlp.forward_batched_fused_routed(x, logits, router)):
        torch.cuda.synchronize()
        assert bool(torch.isnan(out[2]).all())  # the NaN weights of the row, on experts 0 and 1
        assert bool(torch.isfinite(out[keep]).all())
    assert torch.equal(mlp.forward_batched_fused_routed(x, logits, router)[keep], clean[keep])
