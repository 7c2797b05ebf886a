"""Planner for 8- and 16-bit packed words (the reference's packing_bitwidth=8 / 16): W_q [K / e8, N] uint8 or [K / e16, N] int16.

Byte rows 4R .. 4R+3 (short rows 2R, 2R+1) of a column, concatenated little-endian, are that column's int32 word of packed row R, so the MFMA tile
kernel and the dot-product GEMV take these layouts with a different word source and nothing else.  No GPU: everything here goes through
gemlite_hip_kernel_name / gemlite_hip_workspace_bytes, which plan and never launch."""
import ctypes as C
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from tests.test_host_cpu import _args  # noqa: E402
from tests.test_planner_tile_families_cpu import SHAPES  # noqa: E402

MS = (1, 2, 4, 16, 33, 64, 128, 256, 2048)
W_DTYPE = {8: 5, 16: 9}  # UINT8 / INT16 (include/gemlite_hip.h)
SUFFIX = {8: ",b8>", 16: ",b16>"}


def _lib():
    lib = _hip.load()
    lib.gemlite_hip_workspace_bytes.restype = C.c_uint64
    return lib


def _pw(pb, **kw):
    """The request of _args() with its words packed into pb-bit samples (same shape, strides in elements of the word type)."""
    a = _args(**kw)
    a.w_pack_bits, a.w_dtype = pb, W_DTYPE[pb]
    a.elements_per_sample = pb // a.W_nbits
    a.stride_wk, a.stride_wn = a.N, 1
    return a


def _plan(lib, a):
    return lib.gemlite_hip_kernel_name(C.byref(a)).decode(), int(lib.gemlite_hip_workspace_bytes(C.byref(a)))


def _is_tile(name):
    return name.startswith(("gemm_w4_mma_kernel<", "gemm_w2_mma_kernel<", "gemm_w1_mma_kernel<", "gemm_w8_mma_kernel<"))


@pytest.mark.parametrize("nbits", [4, 2])
@pytest.mark.parametrize("in_dt", [1, 2])
def test_pack_widths_plan_specialised_kernels(nbits, in_dt):
    lib = _lib()
    same_plan = 0
    for (N, K) in SHAPES:
        for gs in (64, 128, K):
            for M in MS:
                kw = dict(M=M, N=N, K=K, nbits=nbits, gs=gs, in_dt=in_dt)
                n32, ws32 = _plan(lib, _args(**kw))
                for pb in (8, 16):
                    name, ws = _plan(lib, _pw(pb, **kw))
                    key = (pb, nbits, in_dt, N, K, gs, M, n32, name)
                    assert name != "unsupported", key
                    if "generic" not in n32:
                        assert "generic" not in name, key
                    if "generic" not in name:
                        assert name.endswith(SUFFIX[pb]), key
                    # where the 32-bit request plans a tile form, the packed-width request plans the same form (tile, K slices, combine)
                    if _is_tile(n32) and ",g32" not in n32:
                        assert name == n32[:-1] + SUFFIX[pb], key
                        assert ws == ws32, key
                        same_plan += 1
    assert same_plan >= 500


@pytest.mark.parametrize("pb", [8, 16])
def test_pack_widths_labels_at_one_and_many_rows(pb):
    lib = _lib()
    n1 = _plan(lib, _pw(pb, M=1, N=4096, K=4096))[0]
    assert n1.startswith("gemv_wn_kernel<tile32") and n1.endswith(SUFFIX[pb]), n1
    n1 = _plan(lib, _pw(pb, M=1, N=11008, K=4096))[0]
    assert n1.startswith("gemv_wn_kernel<tile64") and n1.endswith(SUFFIX[pb]), n1
    assert _plan(lib, _pw(pb, M=16, N=4096, K=4096))[0].startswith("gemm_w4_mma_kernel<32x128")
    assert _plan(lib, _pw(pb, M=256, N=4096, K=4096, nbits=2))[0].startswith("gemm_w2_mma_kernel<")
    # 1-bit words take the tile kernel and (16-bit words) the GEMV as well; 8-bit values in 16-bit words the tile kernel
    assert _plan(lib, _pw(pb, M=64, N=4096, K=4096, nbits=1))[0] == f"gemm_w1_mma_kernel<64x128{SUFFIX[pb]}"
    assert _plan(lib, _pw(pb, M=1, N=4096, K=4096, nbits=1))[0].endswith(SUFFIX[pb])
    if pb == 16:
        assert _plan(lib, _pw(pb, M=64, N=4096, K=4096, nbits=8))[0] == "gemm_w8_mma_kernel<64x128,b16>"
        assert _plan(lib, _pw(pb, M=1, N=4096, K=4096, nbits=8))[0] == "gemm_w8_mma_kernel<32x128,b16>"


@pytest.mark.parametrize("pb", [8, 16])
def test_pack_widths_misaligned_or_unsupported_take_the_coverage_kernel(pb):
    lib = _lib()
    for M in (1, 16, 256):
        a = _pw(pb, M=M, N=4096, K=4096)
        a.w_q = 0x1001  # not 4-byte aligned: no dword loads of words
        assert _plan(lib, a)[0] == "generic_matmul_kernel", (pb, M)
        a = _pw(pb, M=M, N=4096 + 16, K=4096)  # N not a multiple of the 32- / 64-column tiles
        assert _plan(lib, a)[0] == "generic_matmul_kernel", (pb, M)
        a = _pw(pb, M=M, N=4096, K=4096, gs=32)  # groups of 32: no packed-width form of the NGS = 2 tiles (one row: the GEMV takes them)
        assert _plan(lib, a)[0] == ("gemv_wn_kernel<tile32" + SUFFIX[pb] if M == 1 else "generic_matmul_kernel"), (pb, M)
        if pb == 8:
            a = _pw(pb, M=M, N=4096, K=4096)
            a.stride_wk = 4096 + 2  # byte-row stride not a multiple of 4 bytes
            assert _plan(lib, a)[0] == "generic_matmul_kernel", (pb, M)
    # 8-bit activations over 8- / 16-bit words: the coverage kernel (no packed-width form of the A8Wn kernels)
    a = _pw(pb, M=64, N=4096, K=4096, in_dt=3, c_mode=3, w_mode=0, gs=4096)
    a.scales_x = 0x1000
    assert _plan(lib, a)[0] == "generic_matmul_kernel"


@pytest.mark.parametrize("pb", [8, 16])
def test_pack_widths_forced_forms_without_a_packed_counterpart_decline(pb):
    """Forced tile variants and kernels that have no 8- / 16-bit word source fall to the coverage kernel instead of reading words as int32."""
    lib = _lib()
    cases = [dict(tuning=(0, 0, 33)), dict(tuning=(0, 0, 34)), dict(tuning=(0, 0, 35)),  # narrow variants 1 .. 3
             dict(tuning=(9,)),  # rows kernel
             dict(tuning=(2,)), dict(tuning=(1,)), dict(tuning=(4, 2))]  # round-1 tiled, streaming, gemv_mfma / direct
    for kw in cases:
        for M in (1, 4, 64, 256):
            name = _plan(lib, _pw(pb, M=M, N=4096, K=4096, **kw))[0]
            assert name == "generic_matmul_kernel" or name.endswith(SUFFIX[pb]), (kw, M, name)


@pytest.mark.parametrize("pb", [8, 16])
def test_pack_widths_fuzz(pb):
    lib = _lib()
    rng = random.Random(pb)
    for _ in range(3000):
        nbits = rng.choice([4, 2, 1] + ([8] if pb == 16 else []))
        N = rng.choice([64, 128, 192, 256, 1024, 4096, 4160, 11008])
        K = rng.choice([128, 256, 384, 640, 1024, 4096, 8960, 11008])
        gs = rng.choice([32, 64, 128, 96, K])
        if K % gs:
            gs = K
        M = rng.choice([1, 2, 3, 5, 16, 17, 31, 33, 64, 65, 128, 255, 256, 1024])
        tuning = tuple(rng.choice([0, 0, 0, 1, 2, 3, 4, 8, 9, 16, 20, 24, 32, 33, 48]) for _ in range(3))
        a = _pw(pb, M=M, N=N, K=K, nbits=nbits, gs=gs, in_dt=rng.choice([1, 2]), mt=rng.choice([-1, -1, 0, 1, 2, 3, 4]), tuning=tuning)
        name, _ = _plan(lib, a)
        assert name in ("generic_matmul_kernel", "unsupported") or name.endswith(SUFFIX[pb]), (pb, nbits, N, K, gs, M, tuning, name)
