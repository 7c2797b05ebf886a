"""The HQQ zero-point optimiser on the GPU: gemlite_hip_quantize_groups_hqq.  iters = 0 against the RTN launch
byte for byte; exact, oracle-free properties of every output; the two caps against the float64 oracle of
tests/quant_hqq_spec.py; that it actually gains over RTN; both output forms, views, guard bands, determinism, graph capture;
degenerate and non-finite groups; the *_HQQOPT_INT processors and patch_model.  Shapes are the smallest that reach each path.

Figures of the run this file was written against are in DESIGN §2.1a; every test prints its own before it asserts."""
import ctypes as C
import math

import pytest
import torch

from gemlite_amd import GemLiteLinear, _hip, helper
from gemlite_amd.bitpack import pack_weights_over_cols
from gemlite_amd.dtypes import TORCH_TO_DTYPE
from gemlite_amd.quant_utils import WeightQuantizerHQQ
from tests.quant_hqq_spec import group_errors64, quantize_hqq_spec, student_t_weights
from tests.quant_int_spec import quantize_groups_spec
from tests.test_quantize_groups_gpu import _same_layer
from tests.test_quantize_hqq_cpu import DTYPES, SHAPES, check_against_oracle, make_weights, oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RAGGED = (80, 384, 128)
SHAPE_IDS = [f"{n}x{k}g{g}" for n, k, g in SHAPES]
HQQ = (20, 0.7, 10.0, 1.01)


def launch(W, nbits, g, T, pack_bits, q, ld_q, scales, zeros, stride_g, stride_n, fold=False, hqq=HQQ):
    """Raw C ABI call: W any 2-D view with unit inner stride; q / scales / zeros tensors (or views) written in place.
    hqq = (iters, lp_norm, beta, kappa), or None for gemlite_hip_quantize_groups."""
    h = _hip.QuantizeHqqArgs()
    h.struct_size = C.sizeof(_hip.QuantizeHqqArgs)
    a = h.q
    a.struct_size = C.sizeof(_hip.QuantizeArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, W.shape[0], W.shape[1], W.stride(0)
    a.W_nbits, a.group_size, a.pack_bits, a.meta_dtype = nbits, g, pack_bits, TORCH_TO_DTYPE[T].value
    a.q_out, a.ld_q, a.scales, a.zeros = q.data_ptr(), ld_q, scales.data_ptr(), zeros.data_ptr()
    a.stride_meta_g, a.stride_meta_n, a.fold_zeros = stride_g, stride_n, int(fold)
    if hqq is None:
        rc = _hip.load().gemlite_hip_quantize_groups(C.byref(a), _hip.current_stream_handle(W.device))
    else:
        h.iters, h.lp_norm, h.beta, h.kappa = hqq
        rc = _hip.load().gemlite_hip_quantize_groups_hqq(C.byref(h), _hip.current_stream_handle(W.device))
    assert rc == 0, _hip.status_string(rc)


def unfused(W, nbits, g, T, hqq=HQQ):
    N, K = W.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=W.device)
    s = torch.empty((N * (K // g), 1), dtype=T, device=W.device)
    z = torch.empty_like(s)
    launch(W, nbits, g, T, 0, q, K, s, z, 1, K // g, hqq=hqq)
    return q, s, z


def fused(W, nbits, g, T, fold, hqq=HQQ):
    N, K = W.shape
    q = torch.empty((K * nbits // 32, N), dtype=torch.int32, device=W.device)
    s = torch.empty((K // g, N), dtype=T, device=W.device)
    z = torch.empty_like(s)
    launch(W, nbits, g, T, 32, q, 0, s, z, N, 1, fold, hqq=hqq)
    return q, s, z


def same(a, b):
    return all(x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------- iters = 0
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("N,K,g", SHAPES, ids=SHAPE_IDS)
def test_zero_iterations_is_the_rtn_launch_byte_for_byte(N, K, g, nbits):
    for in_dt, T in DTYPES:
        W = make_weights("planted", N, K, g, in_dt).to(DEV)
        hq = (0, 0.7, 10.0, 1.01)
        assert same(unfused(W, nbits, g, T, hqq=hq), unfused(W, nbits, g, T, hqq=None))
        for fold in (False, True):
            assert same(fused(W, nbits, g, T, fold, hqq=hq), fused(W, nbits, g, T, fold, hqq=None))


# ------------------------------------------------------------------------------------- exact properties, and the oracle
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("in_dt,T", DTYPES, ids=["fp16", "bf16", "fp32-fp16"])
@pytest.mark.parametrize("N,K,g", SHAPES, ids=SHAPE_IDS)
def test_outputs_are_consistent_no_worse_than_rtn_and_within_the_caps_of_the_oracle(N, K, g, in_dt, T, nbits):
    G, qmax = K // g, float(2 ** nbits - 1)
    for kind in ("planted", "student_t"):
        W, rtn, want = oracle(kind, N, K, g, in_dt, T, nbits)
        q, s, z = WeightQuantizerHQQ(nbits, g, dtype=T).quantize(W.to(DEV))
        assert q.dtype == torch.uint8 and q.shape == (N, K) and s.shape == z.shape == (N * G, 1) and s.dtype == z.dtype == T
        q, s, z = q.cpu(), s.cpu().float().view(N, G), z.cpu().float().view(N, G)
        # the scale is RTN's, bit for bit
        assert torch.equal(s, rtn[1])
        # the codes are the rounding against the zero the kernel returned (torch fp32: one division, one addition, as the layer's contract)
        w = W.float().view(N, G, g)
        codes = torch.clamp(torch.round(w / s.unsqueeze(-1) + z.unsqueeze(-1)), 0.0, qmax).to(torch.uint8).view(N, K)
        assert torch.equal(q, codes)
        # no group is worse than RTN (float64 error of the outputs; the factor is the fp32 summation bound of the two compared means)
        e, e_rtn = group_errors64(W, q, s, z, g), group_errors64(W, *rtn, g)
        worst = float((e - e_rtn * (1 + 2 * g * 2.0 ** -24)).max())
        print(f"{kind}: max over groups of error - RTN's bound = {worst:.3e}; summed error / RTN's = {float(e.sum() / e_rtn.sum().clamp_min(1e-300)):.4f}")
        assert worst <= 0.0
        check_against_oracle(W, g, (q, s, z), want[:3], f"{N}x{K} g{g} {kind} {nbits} bits {in_dt}")


# (nbits, shape): the group sizes the oracle's 0.96 / 0.91 / 0.50 were measured at (4 bits g64, 2 bits g64, 1 bit g32)
GAINS = [(4, (64, 256, 64)), (2, (64, 256, 64)), (1, (200, 1024, 32))]


@pytest.mark.parametrize("nbits,shape", GAINS, ids=["4bit-g64", "2bit-g64", "1bit-g32"])
def test_gains_over_rtn_on_heavy_tailed_weights(nbits, shape):
    N, K, g = shape
    T = torch.float16
    W, rtn, want = oracle("student_t", N, K, g, T, T, nbits)
    q, s, z = WeightQuantizerHQQ(nbits, g).quantize(W.to(DEV))
    e = float(group_errors64(W, q, s.float().view(N, -1), z.float().view(N, -1), g).sum())
    e_rtn, e_or = float(group_errors64(W, *rtn, g).sum()), float(group_errors64(W, *want[:3], g).sum())
    print(f"{nbits} bits g{g}: kernel / RTN = {e / e_rtn:.4f} (oracle / RTN = {e_or / e_rtn:.4f})")
    assert e < 0.99 * e_rtn


def test_lp_norm_one_takes_the_branch_without_a_power():
    N, K, g, nbits, T = 64, 256, 64, 4, torch.float16
    W = student_t_weights(N, K, T, seed=3)
    want = quantize_hqq_spec(W, nbits, g, T, iters=30, lp_norm=1.0, beta=50.0, kappa=1.05)
    q, s, z = WeightQuantizerHQQ(nbits, g, iters=30, lp_norm=1.0, beta=50.0, kappa=1.05).quantize(W.to(DEV))
    got = (q.cpu(), s.cpu().float().view(N, -1), z.cpu().float().view(N, -1))
    check_against_oracle(W, g, got, want[:3], "lp_norm = 1")
    assert (group_errors64(W, *got, g) <= group_errors64(W, *quantize_groups_spec(W, nbits, g, T), g) * (1 + 2 * g * 2.0 ** -24)).all()


# --------------------------------------------------------------------------------------------------------------- layouts
@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N,K,g", [RAGGED, (64, 768, 96), (16, 512, 512), (200, 1024, 32)], ids=["ragged", "g96", "channelwise", "g32"])
def test_fused_equals_unfused(N, K, g, T, nbits):
    W = student_t_weights(N, K, T, seed=5).to(DEV)
    q, s, z = unfused(W, nbits, g, T)
    packed, e = pack_weights_over_cols(q, W_nbits=nbits, packing_bitwidth=32, transpose=True)
    for fold in (False, True):
        qp, sp, zp = fused(W, nbits, g, T, fold)
        assert torch.equal(qp, packed)
        assert torch.equal(sp, s.view(N, -1).t())
        want_z = (-z.float() * s.float()).to(T) if fold else z
        assert torch.equal(zp, want_z.view(N, -1).t())


@pytest.mark.parametrize("in_dt", [torch.float16, torch.float32], ids=["fp16", "fp32"])
@pytest.mark.parametrize("N,K,g", [RAGGED, (64, 768, 96)], ids=["ragged", "g96"])
def test_view_of_a_larger_matrix(N, K, g, in_dt):
    big = student_t_weights(N + 3, K + 72, in_dt, seed=7).to(DEV)
    view = big[2:2 + N, 1:1 + K]  # ld_w > K, first element one element past an aligned address
    assert view.stride(0) > K and view.data_ptr() % 16 != 0
    assert same(unfused(view, 4, g, torch.float16), unfused(view.clone(), 4, g, torch.float16))
    assert same(fused(view, 4, g, torch.float16, True), fused(view.clone(), 4, g, torch.float16, True))


@pytest.mark.parametrize("pack_bits", [0, 32])
def test_guard_bands(pack_bits):
    N, K, g = RAGGED
    nbits, T, G = 4, torch.float16, K // g
    W = student_t_weights(N, K, torch.float16, seed=9).to(DEV)
    if pack_bits == 32:
        qbuf = torch.full((K // 8 + 4, N), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(-1)
        qwin = qbuf[2 * N + 3: 2 * N + 3 + (K // 8) * N]  # the packed form is contiguous: a window at an odd word offset
        ld_q, sg, sn = 0, N + 5, 1
        sbuf = torch.full((G + 2, N + 5), 7.0, dtype=T, device=DEV)
        zbuf = torch.full((G + 2, N + 5), 9.0, dtype=T, device=DEV)
        swin, zwin = sbuf[1:1 + G, 3:3 + N], zbuf[1:1 + G, 3:3 + N]
        want_q, want_s, want_z = fused(W, nbits, g, T, True)
        want_q = want_q.view(-1)
    else:
        qbuf = torch.full((N + 2, K + 24), 0xA5, dtype=torch.uint8, device=DEV)
        qwin = qbuf[1:1 + N, 5:5 + K]  # ld_q > K, unaligned start
        ld_q, sg, sn = K + 24, 1, G + 3
        sbuf = torch.full((N + 2, G + 3), 7.0, dtype=T, device=DEV)
        zbuf = torch.full((N + 2, G + 3), 9.0, dtype=T, device=DEV)
        swin, zwin = sbuf[1:1 + N, 2:2 + G], zbuf[1:1 + N, 2:2 + G]
        want_q, want_s, want_z = unfused(W, nbits, g, T)
        want_s, want_z = want_s.view(N, G), want_z.view(N, G)
    before = [t.clone() for t in (qbuf, sbuf, zbuf)]
    launch(W, nbits, g, T, pack_bits, qwin, ld_q, swin, zwin, sg, sn, fold=pack_bits == 32)
    torch.cuda.synchronize()
    assert torch.equal(qwin, want_q) and torch.equal(swin, want_s) and torch.equal(zwin, want_z)
    for buf, win, old in ((qbuf, qwin, before[0]), (sbuf, swin, before[1]), (zbuf, zwin, before[2])):
        outside = torch.ones_like(buf, dtype=torch.bool)
        torch.as_strided(outside, win.shape, win.stride(), win.storage_offset()).fill_(False)
        assert torch.equal(buf[outside], old[outside])


@pytest.mark.parametrize("N,K,g", [RAGGED, (64, 768, 96)], ids=["ragged", "g96"])
def test_deterministic_and_independent_of_the_place_in_the_grid(N, K, g):
    W = student_t_weights(N, K, torch.bfloat16, seed=11).to(DEV)
    first = fused(W, 2, g, torch.bfloat16, True)
    assert same(first, fused(W, 2, g, torch.bfloat16, True))
    q, s, z = unfused(W, 2, g, torch.bfloat16)
    assert same((q, s, z), unfused(W, 2, g, torch.bfloat16))
    # the same rows further down a taller matrix, the same groups further along a wider one: the same bits
    tall = torch.cat([torch.zeros(70, K, dtype=W.dtype, device=DEV), W])
    qt, st, zt = unfused(tall, 2, g, torch.bfloat16)
    assert torch.equal(qt[70:], q) and torch.equal(st.view(N + 70, -1)[70:], s.view(N, -1)) and torch.equal(zt.view(N + 70, -1)[70:], z.view(N, -1))
    shift = g * 256 // math.gcd(g, 256)  # one whole span of the block
    wide = torch.cat([torch.zeros(N, shift, dtype=W.dtype, device=DEV), W], dim=1).contiguous()
    qw, sw, zw = unfused(wide, 2, g, torch.bfloat16)
    assert torch.equal(qw[:, shift:], q) and torch.equal(sw.view(N, -1)[:, shift // g:], s.view(N, -1))
    assert torch.equal(zw.view(N, -1)[:, shift // g:], z.view(N, -1))


def test_capturable_and_replays_with_the_same_bits():
    N, K, g = RAGGED
    nbits, T = 4, torch.float16
    W = student_t_weights(N, K, torch.float16, seed=13).to(DEV)
    want = fused(W, nbits, g, T, True)
    q = torch.zeros_like(want[0])
    s, z = torch.zeros_like(want[1]), torch.zeros_like(want[2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch(W, nbits, g, T, 32, q, 0, s, z, N, 1, True)
    assert not q.any() and not s.any()  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert same((q, s, z), want)


# ----------------------------------------------------------------------------------------------------- degenerate groups
def _special_rows(g):
    k = torch.arange(g, dtype=torch.float32)
    return [torch.full((g,), -0.731),          # constant, non-zero
            torch.zeros(g),                      # all zero
            (k % 16) * 2.0 ** -3,                # on the 4-bit grid: s_r = 2^-3, z = 0, E(z0) = 0
            torch.tensor([0.0, -0.0] * (g // 2))]


@pytest.mark.parametrize("g", [32, 96], ids=["lanes", "wave"])
def test_groups_with_no_error_come_out_as_rtn(g):
    nbits, T = 4, torch.float16
    rows = _special_rows(g)
    live = student_t_weights(len(rows), g, T, seed=2).float()  # a second group per row that does move
    W = torch.cat([torch.stack(rows), live], dim=1).to(T).to(DEV)
    got, rtn = unfused(W, nbits, g, T), unfused(W, nbits, g, T, hqq=None)
    n = len(rows)
    assert torch.equal(got[0][:, :g], rtn[0][:, :g])
    assert torch.equal(got[1].view(n, 2), rtn[1].view(n, 2))
    assert torch.equal(got[2].view(n, 2)[:, 0], rtn[2].view(n, 2)[:, 0])
    assert (rtn[1].view(n, 2)[2, 0] == 2.0 ** -3) and (rtn[1].view(n, 2)[[0, 1, 3], 0] == 1.0).all()


@pytest.mark.parametrize("N,K,g", [(64, 256, 64), (64, 768, 96), (4, 8192, 8192)], ids=["lanes", "wave", "walked"])
def test_non_finite_weights_stay_in_their_group(N, K, g):
    nbits, T = 4, torch.float16
    clean = student_t_weights(N, K, T, seed=4)
    want = [t.cpu() for t in unfused(clean.to(DEV), nbits, g, T)]
    G = K // g
    for bad in (float("nan"), float("inf"), float("-inf")):
        W = clean.clone()
        r, j = N // 2, G // 2
        W[r, j * g + 5] = bad
        W[r, j * g + g - 1] = bad
        q, s, z = [t.cpu() for t in unfused(W.to(DEV), nbits, g, T)]  # (completes: the copy back is the synchronisation)
        keep = torch.ones(N, G, dtype=torch.bool)
        keep[r, j] = False
        assert torch.equal(s.view(N, G)[keep], want[1].view(N, G)[keep]) and torch.equal(z.view(N, G)[keep], want[2].view(N, G)[keep])
        assert torch.equal(q.view(N, G, g)[keep], want[0].view(N, G, g)[keep])


# ------------------------------------------------------------------------------------------------------------ processors
def test_a16w4_layer_equals_from_weights_of_the_quantiser():
    N, K, g = 256, 512, 64
    torch.manual_seed(3)
    lin = torch.nn.Linear(K, N, bias=True, device=DEV, dtype=torch.float16)
    W, b = lin.weight.data.clone(), lin.bias.data.clone()
    layer = helper.A16W4_HQQOPT_INT(group_size=g).from_linear(lin)
    W_q, scales, zeros = WeightQuantizerHQQ(4, g).quantize(W)
    want = helper.A16W4_HQQ_INT().from_weights(W_q, scales, zeros, 4, g, bias=b)
    assert layer.group_size == g and layer.W_nbits == 4 and layer.W_q.element_size() == 4
    _same_layer(layer, want)
    for M in (1, 8):
        x = (torch.randn(M, K, device=DEV) / 10).to(torch.float16)
        assert torch.equal(layer(x), want(x)), f"M = {M}"
    deq = (W_q.float().view(N, K // g, g) - zeros.float().view(N, K // g, 1)) * scales.float().view(N, K // g, 1)
    got = layer.dequantize(torch.float32)
    # the layer holds the folded zero z' = rT(-z s): q s + z' is (q - z) s up to the rounding of z' to fp16, |z s| 2^-11 per group
    bound = (zeros.float().abs() * scales.float()).view(N, K // g, 1) * 2.0 ** -11 * (1 + 2.0 ** -8)
    assert ((got.view(N, K // g, g) - deq).abs() <= bound).all()
    plain = WeightQuantizerHQQ(4, g).dequantize(W_q, scales, zeros, dtype=torch.float32)  # unfolded: (q - z) s itself
    assert torch.allclose(plain, deq.view(N, K), rtol=2.0 ** -22, atol=0)
    # it is not the RTN layer, and other keywords reach the launch
    rtn = helper.A16W4_RTN_INT(group_size=g).quantize_weights(W, b)
    assert not torch.equal(rtn.zeros, layer.zeros)
    zero_iters = helper.A16W4_HQQOPT_INT(group_size=g, iters=0).quantize_weights(W, b)
    _same_layer(zero_iters, rtn)


def test_a8w4_dynamic_and_other_packing_build_and_run():
    N, K, g = 128, 256, 64
    torch.manual_seed(4)
    lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=torch.float16)
    W = lin.weight.data.clone()
    layer = helper.A8W4_HQQOPT_INT_dynamic(group_size=g).from_linear(lin, del_orig=False)
    want = helper.A8W4_HQQ_INT_dynamic().from_weights(*WeightQuantizerHQQ(4, g).quantize(W), 4, g)
    _same_layer(layer, want)
    x = (torch.randn(4, K, device=DEV) / 10).to(torch.float16)
    y = layer(x)
    assert y.shape == (4, N) and torch.isfinite(y).all() and torch.equal(y, want(x))
    ref = x.float() @ W.float().t()
    assert float((y.float() - ref).abs().mean() / ref.abs().mean()) < 0.2  # 4-bit weights x fp8 activations: the right matrix
    pack8 = helper.A16W4_HQQOPT_INT(group_size=g, packing_bitwidth=8).quantize_weights(W)
    _same_layer(pack8, helper.A16W4_HQQ_INT(packing_bitwidth=8).from_weights(*WeightQuantizerHQQ(4, g).quantize(W), 4, g))


def test_patch_model():
    torch.manual_seed(5)
    net = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64)).to(device=DEV, dtype=torch.float16)
    first = torch.nn.Linear(256, 128).to(device=DEV, dtype=torch.float16)
    first.load_state_dict(net[0].state_dict())
    helper.patch_model(net, DEV, helper.A16W4_HQQOPT_INT(), group_size=32)
    assert isinstance(net[0], GemLiteLinear) and isinstance(net[2], GemLiteLinear)
    assert net[0].group_size == 32 and net[2].group_size == 32
    _same_layer(net[0], helper.A16W4_HQQOPT_INT(group_size=32).from_linear(first))
    assert net(torch.randn(3, 256, device=DEV, dtype=torch.float16)).shape == (3, 64)
    bad = torch.nn.Sequential(torch.nn.Linear(256, 64), torch.nn.Linear(100, 64)).to(device=DEV, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"^1 \("):
        helper.patch_model(bad, DEV, helper.A16W4_HQQOPT_INT(), group_size=64)
