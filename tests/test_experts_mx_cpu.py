"""MXFP4 experts without a GPU: what gemlite_hip_experts_query / _fused_query answer for the MX branch of the experts
planner, one refusal per rule, and GemLiteExperts on CPU-built A16W4_MXFP layers.  The INT branch answers as before."""
import ctypes as C

import pytest
import torch

from gemlite_amd import DType, GemLiteExperts, _hip, experts as X, helper
from .test_experts_cpu import query, request as int_request, set_

OK, BAD_ARG, UNSUPPORTED, BAD_SHAPE = _hip.OK, _hip.ERR_BAD_ARGUMENT, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_SHAPE


def request(N=768, K=2048, dt=DType.MXFP16.value, bias=True):
    """A valid MXFP4 request on stand-in addresses, filled as core._call_args fills an A16W4_MXFP layer: 8 experts, 6 slots, 2 per x row."""
    e = int_request(N, K, bias=bias)
    a = e.layer
    a.zeros = None
    a.W_nbits, a.group_size, a.elements_per_sample, a.w_pack_bits, a.w_dtype = 4, 32, 2, 8, DType.UINT8.value
    a.input_dtype = dt
    a.output_dtype = DType.FP16.value if dt == DType.MXFP16.value else DType.BF16.value
    a.meta_dtype = DType.UINT8.value
    a.W_group_mode, a.channel_scale_mode = 2, 0
    a.stride_wk, a.stride_wn, a.stride_meta_g, a.stride_meta_n = 1, K // 2, N, 1
    e.stride_expert_w, e.stride_expert_meta = N * K // 2, (K // 32) * N
    return e


def fused(e, epilogue):
    f = X._fused_args(e, epilogue, 0x80000, DType.FP32.value, 2)
    return _hip.load().gemlite_hip_experts_fused_query(C.byref(f))


@pytest.mark.parametrize("dt", [DType.MXFP16.value, DType.MXBF16.value])
@pytest.mark.parametrize("N,K", [(32, 256), (32, 768), (48, 2048), (32, 14336), (768, 2048), (4096, 4096)])
def test_the_accepted_domain(N, K, dt):
    for bias in (True, False):
        e = request(N, K, dt, bias)
        assert query(e) == OK
        assert fused(e, _hip.EXPERTS_GLU) == (OK if N % 32 == 0 else BAD_SHAPE)
    e.ids_dtype, e.n_slots, e.stride_expert_w = DType.INT32.value, 65535, 1 << 33
    e.layer.meta_dtype = DType.E8M0.value
    for waves in (0, 4, 8, 16):
        e.layer.tuning[2] = waves
        assert query(e) == OK


REFUSALS = [
    ("K 128", set_("layer.K", 128), BAD_SHAPE), ("N 24", set_("layer.N", 24), BAD_SHAPE), ("too many slots", set_("n_slots", 65536), BAD_SHAPE),
    ("the stage past the LDS budget", lambda e: (set_("layer.K", 32768)(e), set_("layer.stride_wn", 16384)(e)), BAD_SHAPE),
    ("weight offsets past 2^32", set_("layer.stride_wn", 1 << 23), BAD_SHAPE), ("M 2", set_("layer.M", 2), BAD_SHAPE),
    ("fp8 weights", lambda e: (set_("layer.W_nbits", 8)(e), set_("layer.elements_per_sample", 1)(e), set_("layer.w_dtype", DType.FP8e4.value)(e)), UNSUPPORTED), ("nvfp4", set_("layer.input_dtype", DType.NVFP4.value), UNSUPPORTED),
    ("fp16 scales", set_("layer.meta_dtype", DType.FP16.value), UNSUPPORTED), ("output dtype", set_("layer.output_dtype", DType.BF16.value), UNSUPPORTED),
    ("codes not K-contiguous", set_("layer.stride_wk", 2), UNSUPPORTED), ("scale column stride", set_("layer.stride_meta_n", 2), UNSUPPORTED),
    ("misaligned scales base", set_("layer.scales", 0x30008), BAD_ARG), ("misaligned scale rows", set_("layer.stride_meta_g", 776), BAD_ARG),
    ("misaligned expert stride", set_("stride_expert_w", 768 * 1024 + 8), BAD_ARG), ("misaligned expert scales", set_("stride_expert_meta", 64 * 768 + 8), BAD_ARG),
    ("misaligned codes", set_("layer.w_q", 0x20008), BAD_ARG), ("misaligned x", set_("layer.x", 0x10008), BAD_ARG),
    ("x row stride", set_("stride_x_row", 2052), BAD_ARG), ("null scales", set_("layer.scales", None), BAD_ARG), ("waves 12", lambda e: e.layer.tuning.__setitem__(2, 12), BAD_ARG),
]


@pytest.mark.parametrize("what,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_refusal_per_rule_of_the_mx_branch(what, change, status):
    e = request()
    assert query(e) == OK
    change(e)
    assert query(e) == status, what


@pytest.mark.parametrize("xdt", [DType.MXFP8.value, DType.MXFP4.value])
def test_fp8_and_fp4_activations_glu_on_n_48_and_combine_are_refused(xdt):
    e = request()
    e.layer.input_dtype, e.layer.channel_scale_mode, e.layer.scales_x = xdt, 4, 0x90000
    assert query(e) == UNSUPPORTED
    assert fused(request(N=48), _hip.EXPERTS_GLU) == BAD_SHAPE and query(request(N=48)) == OK
    assert fused(request(), _hip.EXPERTS_COMBINE) == UNSUPPORTED
    r = X._rows_args(request(), 16, None)  # the batched path has no MX form
    assert _hip.load().gemlite_hip_experts_rows_per_block(C.byref(r)) == UNSUPPORTED


def test_int_experts_answer_as_before():
    e = int_request()
    assert query(e) == OK and fused(e, _hip.EXPERTS_GLU) == OK and fused(e, _hip.EXPERTS_COMBINE) == OK
    e.layer.tuning[2] = 12  # (not read by the INT branch)
    assert query(e) == OK
    e.layer.w_pack_bits, e.layer.elements_per_sample = 8, 2
    assert query(e) == UNSUPPORTED


def make_layers(E=4, N=48, K=768, dtype=torch.float16, bias=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    proc = helper.A16W4_MXFP(device="cpu", dtype=dtype)
    return [proc.from_weights(torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g), torch.randint(118, 127, (N, K // 32), dtype=torch.uint8, generator=g),
                              (torch.rand(N, generator=g) - 0.5).to(dtype) if bias else None) for _ in range(E)]


def test_from_layers_keeps_the_k_contiguous_storage_and_expert_views_share_it():
    layers = make_layers()
    ex = GemLiteExperts.from_layers(layers)
    assert tuple(ex.W_q.shape) == (4, 384, 48) and ex.W_q.stride() == (48 * 384, 1, 384) and ex.W_q.dtype == torch.uint8
    assert tuple(ex.scales.shape) == (4, 48, 24) and ex.scales.stride() == (24 * 48, 1, 48) and ex.zeros.numel() == 0
    for i, lin in enumerate(layers):
        v = ex.expert(i)
        assert torch.equal(v.W_q, lin.W_q) and torch.equal(v.scales, lin.scales) and torch.equal(v.bias, lin.bias)
        assert v.W_q.stride() == lin.W_q.stride() and v.W_q.data_ptr() == ex.W_q[i].data_ptr() and v.get_meta_args() == lin.get_meta_args()
    a = X._static_args(ex.W_q, ex.scales, ex.zeros, ex.bias, ex.get_meta_args())
    assert (a.n_experts, a.stride_expert_w, a.stride_expert_meta, a.layer.stride_wk, a.layer.stride_wn, a.layer.stride_meta_g) == (4, 48 * 384, 24 * 48, 1, 384, 48)
    ex2 = GemLiteExperts()
    ex2.load_state_dict({k: v.clone() for k, v in ex.state_dict().items()})
    assert ex2.W_q.stride() == ex.W_q.stride() and torch.equal(ex2.W_q, ex.W_q) and torch.equal(ex2.expert(3).scales, layers[3].scales)
    with pytest.raises(NotImplementedError, match="MXFP4 N=40"):
        GemLiteExperts.from_layers(make_layers(E=2, N=40))
