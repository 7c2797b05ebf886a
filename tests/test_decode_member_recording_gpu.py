"""The M = 1 decode kernels that share dec3::run_member (gemv_decode.hip) against a recording of their raw output bits (run on a real
MI355X via `pytest -m gpu`): gemv_w4_decode3_kernel, gemv_w4_decode3_experts_kernel and gemv_w4_decode3_experts_fused_kernel with the GLU
and COMBINE epilogues.  The other suites compare these kernels with each other, which says nothing about the code they share; here
every launch is compared with numpy.array_equal against tests/golden/decode_member_recording.npz.

The recording was made on an MI355X from a build of commit c5a745c, the last one in which the three kernels each had a body of their
own, by running launches() below on that build.  It is never made from the code under test.

Shapes: N = 256 with K = 1024 (4 chunks: 12 virtual waves write zeros), 4096 (one chunk per wave), 4352 (17 chunks: wave 0 alone has two)
and 8192 (two per wave, the single-layer planner's limit); for the experts kernels also N = 32 with K = 8448 (33 chunks: the third request
happens inside the loop, in wave 0 only).  Every shape runs the four rows of tests/test_experts_fused_gpu.py::ROWS (fp16 / bf16, groups of
32 / 128, zeros as tensor / scalar, with / without bias, ids int32 / int64), every launch of experts has one invalid id.  Inputs come from
fixed seeds on the CPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from gemlite_amd import _hip, core
from tests.test_experts_fused_gpu import COMBINE, GLU, ROWS, launch_fused
from tests.test_experts_gpu import DEV, TUNING, guards_intact, launch_guarded, make_experts, rand_x

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_member_recording.npz")
SHAPES = [(256, 1024), (256, 4096), (256, 4352), (256, 8192), (32, 8448)]  # the last: experts kernels only
N_EXPERTS = 4
# tuning[3]: GEMLITE_TF_GEMV_X_DIRECT (the planner then names gemv_w4_decode3_kernel up to two chunks per wave, K = 8192 included), and
# with GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS gemv_w4_decode3_kernel<Tag, NT = false, ...>
TUNING_DIRECT, TUNING_DEFAULT_POLICY = TUNING[:3] + (2,), TUNING[:3] + (2 | 32,)
TOP_KS = (1, 3, 16)  # 16: one wave per member; 3: an uneven split with idle waves


def bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy()


def invalid_id(ids_dtype):
    return (1 << 32) + 1 if ids_dtype == torch.int64 else -1


def single_layer(lin, x_row, tuning):
    """the expert's own gemv_w4_decode3_kernel launch, the bias added by the launch itself (both asserted)"""
    lib, x2 = _hip.load(), x_row.reshape(1, -1)
    a = core._call_args(x2, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, tuning, False, 0x1000, (lin.W_q.shape[1], 1))
    name = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
    assert name.startswith("gemv_w4_decode3_kernel"), name
    if lin.bias is not None:
        ext = _hip.forward_ext(lin.bias.data_ptr(), core.TORCH_TO_DTYPE[lin.bias.dtype].value)
        assert lib.gemlite_hip_bias_fused(C.byref(a), C.byref(ext)) == 1
    return core._hip_matmul(x2, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, tuning, bias=lin.bias)[0]


def combine_ids(T, top_k, ids_dtype):
    """ids cycling through the experts, slot 1 of the first token invalid where the token has one"""
    ids = ((torch.arange(T * top_k) * 3 + 1) % N_EXPERTS).view(T, top_k).to(ids_dtype)
    if top_k > 1:
        ids[0, 1] = invalid_id(ids_dtype)
    return ids.to(DEV)


def launches(N, K, row):
    """-> {name: the raw 16-bit output of one launch}, in a fixed order"""
    dtype, gs, zeros, bias, ids_dtype = ROWS[row]
    ex = make_experts(N, K, gs, dtype, zeros, bias, n=N_EXPERTS, seed=7)
    out = {}
    x = rand_x((3, K), dtype, 11 + row)
    if N == 256:
        for name, tuning in (("single", TUNING_DIRECT), ("single_default_policy", TUNING_DEFAULT_POLICY)):
            out[name] = bits(single_layer(ex.expert(1), x[1], tuning))  # (slot 2 of the experts launch below)
    ids = torch.tensor([[3, 1], [1, invalid_id(ids_dtype)], [0, 2]], dtype=ids_dtype, device=DEV)
    y, buf = launch_guarded(ex, x, ids)
    assert guards_intact(buf)
    out["experts"] = bits(y)
    y, buf = launch_fused(ex, GLU, x, ids)
    assert guards_intact(buf)
    out["glu"] = bits(y)
    for top_k in TOP_KS:
        T = {1: 3, 3: 2, 16: 1}[top_k]
        cids = combine_ids(T, top_k, ids_dtype)
        g = torch.Generator().manual_seed(100 + top_k)
        w = (torch.rand(T, top_k, generator=g) + 0.05).to(torch.float32 if row % 2 == 0 else dtype).to(DEV)
        y, buf = launch_fused(ex, COMBINE, rand_x((T, top_k, K), dtype, 20 + top_k), cids, w)
        assert guards_intact(buf)
        out[f"combine{top_k}"] = bits(y)
    return out


def key(N, K, row, name):
    return f"{N}x{K}_row{row}_{name}"


@pytest.mark.parametrize("row", range(len(ROWS)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_launch_is_bit_identical_to_the_recording(shape, row):
    N, K = shape
    rec = np.load(GOLDEN)
    got = launches(N, K, row)
    assert set(got) == {"experts", "glu", "combine1", "combine3", "combine16"} | ({"single", "single_default_policy"} if N == 256 else set())
    for name, arr in got.items():
        want = rec[key(N, K, row, name)]
        assert arr.shape == want.shape and arr.any(), (shape, row, name)
        assert np.array_equal(arr, want), (shape, row, name, int((arr != want).sum()))
    if N == 256:
        assert np.array_equal(got["experts"][2], got["single"])
    # the invalid slot of the experts launch and of GLU: exactly zero
    assert not got["experts"][3].any() and not got["glu"][3].any()
