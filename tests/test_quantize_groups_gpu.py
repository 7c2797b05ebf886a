"""The grouped INT weight quantiser on the GPU: gemlite_hip_quantize_groups against the torch restatement of its contract
(tests/quant_int_spec.py) bit for bit, both output forms, views, guard bands, graph capture, and the layers the *_RTN_INT
processors / patch_model / warmup build from it.  Shapes are the smallest that reach each path of the kernel."""
import ctypes as C
import functools

import pytest
import torch

from gemlite_amd import GemLiteLinear, _hip, helper
from gemlite_amd.bitpack import pack_weights_over_cols
from gemlite_amd.dtypes import TORCH_TO_DTYPE
from gemlite_amd.quant_utils import WeightQuantizerINT
from tests.quant_int_spec import folded_zeros_spec, planted_weights, quantize_groups_spec

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (N, K, g): one full tile | the smallest | ragged N, K no multiple of 256 | channel-wise, group longer than a tile |
# a group that does not divide 256 | several tiles both ways
SHAPES = [(64, 256, 64), (1, 32, 32), (80, 384, 128), (16, 512, 512), (64, 768, 96), (200, 1024, 32)]
DTYPES = [(torch.float16, torch.float16), (torch.bfloat16, torch.bfloat16), (torch.float32, torch.float16)]
RAGGED = (80, 384, 128)


def launch(W, nbits, g, T, pack_bits, q, ld_q, scales, zeros, stride_g, stride_n, fold=False):
    """Raw C ABI call: W any 2-D view with unit inner stride; q / scales / zeros tensors (or views) written in place."""
    a = _hip.QuantizeArgs()
    a.struct_size = C.sizeof(_hip.QuantizeArgs)
    a.w, a.w_dtype, a.N, a.K, a.ld_w = W.data_ptr(), TORCH_TO_DTYPE[W.dtype].value, W.shape[0], W.shape[1], W.stride(0)
    a.W_nbits, a.group_size, a.pack_bits, a.meta_dtype = nbits, g, pack_bits, TORCH_TO_DTYPE[T].value
    a.q_out, a.ld_q, a.scales, a.zeros = q.data_ptr(), ld_q, scales.data_ptr(), zeros.data_ptr()
    a.stride_meta_g, a.stride_meta_n, a.fold_zeros = stride_g, stride_n, int(fold)
    rc = _hip.load().gemlite_hip_quantize_groups(C.byref(a), _hip.current_stream_handle(W.device))
    assert rc == 0, _hip.status_string(rc)


def unfused(W, nbits, g, T):
    N, K = W.shape
    q = torch.empty((N, K), dtype=torch.uint8, device=W.device)
    s = torch.empty((N * (K // g), 1), dtype=T, device=W.device)
    z = torch.empty_like(s)
    launch(W, nbits, g, T, 0, q, K, s, z, 1, K // g)
    return q, s, z


def fused(W, nbits, g, T, fold):
    N, K = W.shape
    q = torch.empty((K * nbits // 32, N), dtype=torch.int32, device=W.device)
    s = torch.empty((K // g, N), dtype=T, device=W.device)
    z = torch.empty_like(s)
    launch(W, nbits, g, T, 32, q, 0, s, z, N, 1, fold)
    return q, s, z


@functools.lru_cache(maxsize=None)
def reference(N, K, g, in_dt, T, nbits):
    """(W on the CPU, spec codes, spec scales, spec zeros): computed once, shared, never modified."""
    W = planted_weights(N, K, g, in_dt, seed=N * 7 + K)
    return (W,) + quantize_groups_spec(W, nbits, g, T)


@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("in_dt,T", DTYPES, ids=["fp16", "bf16", "fp32-fp16"])
@pytest.mark.parametrize("N,K,g", SHAPES, ids=[f"{n}x{k}g{g}" for n, k, g in SHAPES])
def test_matches_the_restatement(N, K, g, in_dt, T, nbits):
    W, q_ref, s_ref, z_ref = reference(N, K, g, in_dt, T, nbits)
    q, s, z = WeightQuantizerINT(nbits, g, dtype=T).quantize(W.to(DEV))
    assert q.dtype == torch.uint8 and q.shape == (N, K) and s.shape == z.shape == (N * K // g, 1) and s.dtype == z.dtype == T
    assert torch.equal(s.cpu().float().view(N, K // g), s_ref)
    assert torch.equal(z.cpu().float().view(N, K // g), z_ref)
    assert torch.equal(q.cpu(), q_ref)


def test_special_groups():
    g, nbits, T = 32, 4, torch.float16
    k = torch.arange(g, dtype=torch.float32)
    rows = [torch.full((g,), -0.731),                      # constant, non-zero
            torch.zeros(g),                                  # all zero
            0.01 + 2e-5 * k,                                 # distinct fp16 values, range 6.2e-4 < 15 * 2^-14
            torch.tensor([0.0, -0.0] * (g // 2)),            # both zeros, nothing else
            torch.cat([torch.tensor([0.0, -0.0]), 0.01 * k[2:]]),  # both zeros at the low end of a live group
            torch.cat([torch.tensor([0.0, 15 * 2.0 ** -3]), (k[:g - 2] % 15 + 0.5) * 2.0 ** -3])]  # exact ties: s_r = 2^-3
    W = torch.stack(rows).to(torch.float16)
    q_ref, s_ref, z_ref = quantize_groups_spec(W, nbits, g, T)
    assert s_ref[5, 0] == 2.0 ** -3 and z_ref[5, 0] == 0.0
    # half to even decides: (k + 0.5) -> k for even k, k + 1 for odd k
    want = torch.tensor([(j % 15) + ((j % 15) & 1) for j in range(g - 2)], dtype=torch.uint8)
    assert torch.equal(q_ref[5, 2:], want)
    q, s, z = WeightQuantizerINT(nbits, g, dtype=T).quantize(W.to(DEV))
    assert torch.equal(q.cpu(), q_ref)
    assert torch.equal(s.cpu().float().view(6, 1), s_ref) and torch.equal(z.cpu().float().view(6, 1), z_ref)
    assert (s_ref[:4, 0] == 1.0).all() and (q_ref[:4] == 0).all() and W[2].unique().numel() == g


@pytest.mark.parametrize("nbits", [8, 4, 2, 1])
@pytest.mark.parametrize("T", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("N,K,g", [RAGGED, (64, 768, 96), (16, 512, 512)], ids=["ragged", "g96", "channelwise"])
def test_fused_equals_unfused(N, K, g, T, nbits):
    W = planted_weights(N, K, g, T, seed=5).to(DEV)
    q, s, z = unfused(W, nbits, g, T)
    packed, e = pack_weights_over_cols(q, W_nbits=nbits, packing_bitwidth=32, transpose=True)
    for fold in (False, True):
        qp, sp, zp = fused(W, nbits, g, T, fold)
        assert torch.equal(qp, packed)
        assert torch.equal(sp, s.view(N, -1).t())
        want_z = (-z.float() * s.float()).to(T) if fold else z
        assert torch.equal(zp, want_z.view(N, -1).t())
    _, s_ref, z_ref = quantize_groups_spec(W, nbits, g, T)
    assert torch.equal(zp.float().cpu().t(), folded_zeros_spec(s_ref, z_ref, T))


@pytest.mark.parametrize("in_dt", [torch.float16, torch.float32], ids=["fp16", "fp32"])
def test_view_of_a_larger_matrix(in_dt):
    N, K, g = RAGGED
    big = (torch.randn(N + 3, K + 72, device=DEV) * 0.05).to(in_dt)
    view = big[2:2 + N, 1:1 + K]  # ld_w > K, first element one element past an aligned address
    assert view.stride(0) > K and view.data_ptr() % 16 != 0
    for a, b in zip(unfused(view, 4, g, torch.float16), unfused(view.clone(), 4, g, torch.float16)):
        assert torch.equal(a, b)
    for a, b in zip(fused(view, 4, g, torch.float16, True), fused(view.clone(), 4, g, torch.float16, True)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("pack_bits", [0, 32])
def test_guard_bands(pack_bits):
    N, K, g = RAGGED
    nbits, T, G = 4, torch.float16, K // g
    W = planted_weights(N, K, g, torch.float16, seed=9).to(DEV)
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
        # mark the window through a view of the mask with the window's own geometry
        torch.as_strided(outside, win.shape, win.stride(), win.storage_offset()).fill_(False)
        assert torch.equal(buf[outside], old[outside])


def test_deterministic():
    N, K, g = RAGGED
    W = planted_weights(N, K, g, torch.bfloat16, seed=11).to(DEV)
    for a, b in zip(fused(W, 2, g, torch.bfloat16, True), fused(W, 2, g, torch.bfloat16, True)):
        assert torch.equal(a, b)
    for a, b in zip(unfused(W, 2, g, torch.bfloat16), unfused(W, 2, g, torch.bfloat16)):
        assert torch.equal(a, b)


def _kernel_nodes(graph: torch.cuda.CUDAGraph) -> int:
    """Kernel nodes of a captured graph, asked of the HIP runtime this process already uses (hipGraphGetNodes / hipGraphNodeGetType)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = C.CDLL(path)
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    raw = C.c_void_p(int(graph.raw_cuda_graph()))
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(raw, None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(raw, nodes, C.byref(n)) == 0
    kinds = []
    for node in nodes:
        t = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(t)) == 0
        kinds.append(t.value)
    assert len(kinds) == sum(1 for t in kinds if t == 0), f"node types {kinds}"  # 0 = hipGraphNodeTypeKernel: nothing but kernels
    return len(kinds)


def test_capturable_one_kernel_node():
    N, K, g = RAGGED
    nbits, T = 4, torch.float16
    W = planted_weights(N, K, g, torch.float16, seed=13).to(DEV)
    want = fused(W, nbits, g, T, True)
    q = torch.zeros_like(want[0])
    s, z = torch.zeros_like(want[1]), torch.zeros_like(want[2])
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph):
        launch(W, nbits, g, T, 32, q, 0, s, z, N, 1, True)
    assert _kernel_nodes(graph) == 1
    assert not q.any() and not s.any()  # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(q, want[0]) and torch.equal(s, want[1]) and torch.equal(z, want[2])


# ----------------------------------------------------------------------------------------------- layers
def _same_layer(a: GemLiteLinear, b: GemLiteLinear):
    for name in ("W_q", "scales", "zeros", "bias"):
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is not None:
            assert ta.dtype == tb.dtype and ta.shape == tb.shape and ta.stride() == tb.stride(), name
            assert torch.equal(ta, tb), name
    assert a.get_meta_args() == b.get_meta_args()
    assert torch.equal(a.metadata, b.metadata) and torch.equal(a.orig_shape, b.orig_shape)


def _same_outputs(a, b, K, dtype):
    for M in (1, 16):
        x = (torch.randn(M, K, device=DEV) / 10).to(dtype)
        assert torch.equal(a(x), b(x)), f"M = {M}"


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("case", ["a16w4", "a16w2", "a8w4", "a16w4_pack8"])
def test_layer_equals_from_weights_of_quantize(case, dtype):
    N, K, g = 256, 512, 128
    torch.manual_seed(3)
    lin = torch.nn.Linear(K, N, bias=True, device=DEV, dtype=dtype)
    W, b = lin.weight.data.clone(), lin.bias.data.clone()
    if case == "a16w4":
        new, old, nbits = helper.A16W4_RTN_INT(group_size=g), helper.A16W4_HQQ_INT(), 4
    elif case == "a16w2":
        new, old, nbits = helper.A16W2_RTN_INT(group_size=g), helper.A16W2_HQQ_INT(), 2
    elif case == "a8w4":
        new, old, nbits = helper.A8W4_RTN_INT_dynamic(group_size=g), helper.A8W4_HQQ_INT_dynamic(), 4
    else:
        new, old, nbits = helper.A16W4_RTN_INT(group_size=g, packing_bitwidth=8), helper.A16W4_HQQ_INT(packing_bitwidth=8), 4
    layer = new.from_linear(lin)
    want = old.from_weights(*WeightQuantizerINT(nbits, g).quantize(W), nbits, g, bias=b)
    assert layer.group_size == g and layer.W_nbits == nbits
    assert layer.W_q.element_size() == (1 if case == "a16w4_pack8" else 4)
    _same_layer(layer, want)
    _same_outputs(layer, want, K, dtype)


def test_channelwise_group_takes_the_fused_route_too():
    N, K = 128, 512
    torch.manual_seed(4)
    lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=torch.float16)
    W = lin.weight.data.clone()
    layer = helper.A16W4_RTN_INT(group_size=K).from_linear(lin)
    want = helper.A16W4_HQQ_INT().from_weights(*WeightQuantizerINT(4, K).quantize(W), 4, K)
    _same_layer(layer, want)
    _same_outputs(layer, want, K, torch.float16)


def test_patch_model_and_warmup():
    torch.manual_seed(5)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.body = torch.nn.Sequential(torch.nn.Linear(256, 128), torch.nn.ReLU(), torch.nn.Linear(128, 64))
            self.lm_head = torch.nn.Linear(64, 32)

        def forward(self, x):
            return self.lm_head(self.body(x))

    net = Net().to(device=DEV, dtype=torch.float16)
    first = torch.nn.Linear(256, 128).to(device=DEV, dtype=torch.float16)
    first.load_state_dict(net.body[0].state_dict())
    helper.patch_model(net, DEV, helper.A16W4_RTN_INT(), group_size=128)
    assert isinstance(net.body[0], GemLiteLinear) and isinstance(net.body[2], GemLiteLinear)
    assert net.body[0].group_size == 128 and net.body[2].group_size == 128
    assert type(net.lm_head) is torch.nn.Linear
    _same_layer(net.body[0], helper.A16W4_RTN_INT(group_size=128).from_linear(first))
    assert net(torch.randn(3, 256, device=DEV, dtype=torch.float16)).shape == (3, 32)
    # a processor built with a group size keeps it
    net2 = torch.nn.Sequential(torch.nn.Linear(256, 64)).to(device=DEV, dtype=torch.float16)
    helper.patch_model(net2, DEV, helper.A16W4_RTN_INT(group_size=64), group_size=128)
    assert net2[0].group_size == 64
    assert helper.warmup(helper.A16W4_RTN_INT(), shapes=[(256, 512)], batch_sizes=[1, 16], group_size=128) is None
    bad = torch.nn.Sequential(torch.nn.Linear(100, 64)).to(device=DEV, dtype=torch.float16)
    with pytest.raises(ValueError, match="0"):
        helper.patch_model(bad, DEV, helper.A16W4_RTN_INT(), group_size=64)
