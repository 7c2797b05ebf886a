"""CPU-only checks of the host side: pack() mode selection / layout against the reference's golden
outputs, the C-ABI library (loads, exports every symbol of include/gemlite_hip.h, struct ABI), kernel
selection, and loud failure without a GPU.  No compute is launched here."""
import ctypes as C
import json
import os
import sys
import re

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, GemLiteLinear, _hip, bitpack
from gemlite_amd.core import get_closest_m, get_matmul_type
from tests.golden_util import GOLDEN, as_torch, load_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = load_cases()


# ------------------------------------------------------------------------------------------- C ABI
def test_library_exports_every_header_symbol():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    declared = set(re.findall(r"\b(gemlite_hip_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_hip.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(lib, name), f"libgemlite_hip.so does not export {name}"
    assert lib.gemlite_hip_abi_version() == 1
    assert b"gfx950" in lib.gemlite_hip_build_info()


def _args(M=1, N=4096, K=4096, nbits=4, gs=128, in_dt=1, w_mode=4, c_mode=0, e=None, mt=-1, **kw):
    a = _hip.ForwardArgs()
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = mt
    a.x = a.w_q = a.scales = a.zeros = a.out = 0x1000  # never dereferenced by query / planning
    a.M, a.N, a.K = M, N, K
    e = 32 // nbits if e is None else e
    a.W_nbits, a.group_size, a.unpack_mask, a.elements_per_sample = nbits, gs, 2 ** nbits - 1, e
    a.w_pack_bits, a.w_dtype = (32, 6) if e > 1 else (0, kw.get("w_dtype", in_dt))
    a.input_dtype = a.output_dtype = a.meta_dtype = a.zeros_dtype = in_dt
    a.output_dtype = kw.get("out_dt", in_dt if in_dt in (0, 1, 2) else 1)
    if in_dt in (3, 4, 8):  # 8-bit activations: the per-channel weight scales are fp32 (helper.py:474-475)
        a.meta_dtype = kw.get("meta_dt", 0)
    elif "meta_dt" in kw:
        a.meta_dtype = kw["meta_dt"]
    if "zeros_dt" in kw:
        a.zeros_dtype = kw["zeros_dt"]
    a.zero_is_scalar = int(kw.get("zero_scalar", 0))
    a.channel_scale_mode, a.W_group_mode = c_mode, w_mode
    a.stride_xm, a.stride_xk = K, 1
    a.stride_wk, a.stride_wn = (N, 1) if e > 1 else (1, K)
    a.stride_om, a.stride_on = N, 1
    a.stride_meta_g, a.stride_meta_n = N, 1
    for i, t in enumerate(kw.get("tuning", ())):
        a.tuning[i] = t
    return a


def test_struct_abi_and_validation():
    lib = _hip.load()
    a = _args()
    assert lib.gemlite_hip_query(C.byref(a)) == 0
    a.struct_size += 4
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_BAD_ARGUMENT
    a = _args()
    a.x = None
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_BAD_ARGUMENT
    a = _args(in_dt=12)  # e4m3fnuz: not a gfx950 format
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_UNSUPPORTED
    a = _args(c_mode=4)  # MX block scales
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_UNSUPPORTED
    a = _args(K=4100)
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_BAD_SHAPE
    assert "unsupported" in _hip.status_string(_hip.ERR_UNSUPPORTED)
    with pytest.raises(NotImplementedError):
        _hip.raise_for_status(_hip.ERR_UNSUPPORTED, "x")
    with pytest.raises(_hip.GemliteHipError):
        _hip.raise_for_status(_hip.ERR_WORKSPACE, "x")


@pytest.mark.parametrize("kw,kernel", [
    (dict(M=1), "gemv_w4_decode3_kernel<tile16,16w>"),  # cfgA: 256 tiles of 16 columns, K not split; round-4 decode kernel (gemv_decode.hip:
    (dict(M=1, in_dt=2), "gemv_w4_decode3_kernel<tile16,16w>"),  # SGPR-preloaded scalar arguments, weights requested first)
    (dict(M=1, tuning=(0, 0, 0, 16)), "gemv_wn_kernel<tile16,xdirect,16w>"),  # tuning[3] & 16: the round-2 kernel (A/B runs)
    (dict(M=1, tuning=(0, 0, 4, 0)), "gemv_wn_kernel<tile16,xdirect>"),
    (dict(M=1, N=8192, K=8192), "gemv_wn_kernel<tile32>"),   # round 6: the dot-product family on counted asm loads (9.14 us) is ahead of the matrix-core GEMV (9.86) at one row
    (dict(M=1, N=8192, K=8192, tuning=(0, 0, 0, 512)), "gemv_wn_kernel<tile32>"),   # tuning[3] & 512: the dot-product family
    (dict(M=1, tuning=(0, 0, 0, 1024)), "gemv_mfma_kernel<tile16>"),   # tuning[3] & 1024: the matrix-core kernel wherever it applies
    (dict(M=1, N=16384, K=16384), "gemv_wn_kernel<tile64,8w>"),   # round 6: 8 waves from 128 chunks per block (24.5 vs 25.0 us on counted asm loads)
    (dict(M=2), "gemv_mfma_kernel<tile16,rows4>"),    # 2..4 rows: the decode MFMA kernel (x staged once per wave in LDS)
    (dict(M=4), "gemv_mfma_kernel<tile16,rows4>"),
    (dict(M=4, tuning=(0, 0, 0, 512)), "gemm_wn_direct_kernel<tile16>"),   # 2 <= M <= 32: registers-only MFMA kernel, K not split
    (dict(M=5), "gemm_wn_direct_kernel<tile32,8w>"),   # round 3: from 5 rows 32-column tiles x 2 K slices x 8 waves
    (dict(M=8, tuning=(0, 0, 0, 65536)), "gemm_wn_direct_kernel<tile32,8w>"),     # >= 8 rows: 32-column tiles x split-K 2 (less x traffic), round 3: 8 waves per block (tuning[3] & 65536: the round-4 choice)
    # round 5: the decode-shaped rows kernel (gemm_wn_rows.hip) from 8 rows where ONE round of its 16-column blocks covers N (N / 16 <= 256 CUs)
    (dict(M=8), "gemm_w4_rows_kernel<16x16>"),
    (dict(M=16), "gemm_w4_rows_kernel<16x16>"),
    (dict(M=17), "gemm_w4_rows_kernel<32x16>"),
    (dict(M=33), "gemm_w4_rows_kernel<48x16>"),
    (dict(M=64), "gemm_w4_rows_kernel<64x16>"),
    (dict(M=65), "gemm_w4_mma_kernel<64x64>"),
    (dict(M=7), "gemm_wn_direct_kernel<tile32,8w>"),     # ... 2 .. 7 rows at K <= 4096 keep the round-3 kernels (a draw)
    (dict(M=2, N=4096, K=11008), "gemm_w4_rows_kernel<16x16>"),   # ... a longer K: from 2 rows (M = 8: 17.1 -> 12.7 us)
    (dict(M=32, N=4096, K=11008), "gemm_w4_rows_kernel<32x16>"),
    (dict(M=48, N=4096, K=11008), "gemm_w4_mma_kernel<64x128>"),  # past the x re-read budget (176 MB): tile kernel
    (dict(M=16, N=4096, K=14336), "gemm_wn_direct_kernel<tile32>"),   # K > 12288: weights only two chunks ahead: the round-3 kernels
    (dict(M=16, N=6144, K=4096), "gemm_wn_direct_kernel<tile32>"),    # more blocks than CUs (one 146-KB block per CU): two rounds lose
    (dict(M=9, tuning=(9, 0, 0, 0), N=8192, K=8192), "gemm_w4_rows_kernel<16x32>"),   # tuning[0] = 9 forces it (4096 < N <= 8192: two column tiles per block)
    (dict(M=9, tuning=(9, 1, 0, 0), N=8192, K=8192), "gemm_w4_rows_kernel<16x16>"),   # ... tuning[1] = 1: one
    (dict(M=200, tuning=(9, 0, 0, 0)), "gemm_w4_rows_kernel<64x16>"),                   # ... at any M: 64-row blocks along grid.y
    (dict(M=4, gs=32, N=8192, K=8192), "gemm_w4_rows_kernel<16x16>"),   # groups of 32 at M >= 2: nothing but the coverage kernel behind it on shapes the streaming kernel refuses
    (dict(M=300, gs=32), "gemm_w4_mma_kernel<32x128,g32>"),             # ... above 32 rows (round 6): the 32-row tiles of the 8-wave kernel with two metadata pairs per sub-block (61.6 -> 25.4 us at M = 256) ...
    (dict(M=24, gs=32), "gemm_w4_rows_kernel<32x16>"),                  # ... the rows kernel up to its 32 rows per block
    (dict(M=300, gs=32, N=4112), "gemm_w4_rows_kernel<32x16>"),         # ... N % 64 != 0 too
    (dict(M=40, N=4112, K=4096), "gemm_w4_rows_kernel<48x16>"),         # N % 64 != 0 (N % 16 == 0)
    (dict(M=8, N=8192, K=8192), "gemm_wn_direct_kernel<tile64,8w>"),   # ... 64-column tiles x 2 where they still fill the chip
    (dict(M=8, N=6144, K=4096), "gemm_wn_direct_kernel<tile32>"),      # 192 blocks of 32 columns, unsplit: 4 waves
    (dict(M=6, tuning=(0, 0, 4, 0)), "gemm_wn_direct_kernel<tile32>"),   # tuning[2] = 4 / 8: waves per block
    (dict(M=7), "gemm_wn_direct_kernel<tile32,8w>"),   # ... from 5 rows (M = 6: 7.7 -> 6.5 us)
    (dict(M=5, N=8192, K=8192), "gemm_wn_direct_kernel<tile64,8w>"),
    (dict(M=16, N=16384, K=16384), "gemm_wn_direct_kernel<tile64>"),
    (dict(M=24, N=16384, K=16384), "gemm_w4_mma_kernel<32x128>"),   # 17..32 rows over K >= 8192: LDS-staged x wins
    (dict(M=6, tuning=(0, 0, 1, 0)), "gemm_wn_stream_kernel"),  # tuning[2] = 1: LDS-staged streaming kernel
    (dict(M=4, gs=64), "gemv_mfma_kernel<tile16,rows4>"),
    (dict(M=6, gs=64), "gemm_wn_direct_kernel<tile32>"),   # group size 64: registers-only kernel up to 16 rows (round 5: 2 .. 7 at 4096^2)
    (dict(M=8, gs=64), "gemm_w4_rows_kernel<16x16>"),
    (dict(M=24, gs=64, tuning=(0, 0, 0, 65536)), "gemm_wn_stream_kernel"),          # ... LDS-staged streaming kernel for 17..32 (the round-4 choice)
    (dict(M=24, gs=64, N=11008, K=4096), "gemm_w4_mma_kernel<32x128>"),             # round 5: ... where the rows kernel does not pay, the 32-row MFMA tiles (31.6 -> 16.6 us), not the streaming kernel
    (dict(M=24, gs=64, nbits=2), "gemm_w2_rows_kernel<32x16>"),                     # ... 2-bit: 16.4 -> 12.0 us on the MFMA tiles, then 7.8 on the rows kernel (late round 5)
    (dict(M=24, gs=64, nbits=2, N=11008, K=4096), "gemm_w2_mma_kernel<32x128>"),    # ... where the rows kernel does not pay: the 32-row MFMA tiles (31.4 -> 22.6 us)
    (dict(M=24, gs=64, N=1024, K=4096), "gemm_w4_rows_kernel<32x16>"),              # ... small N: the rows kernel (18.8 -> 8.1 us)
    (dict(M=24, gs=64, N=8960, K=1536), "gemm_wn_stream_kernel"),                   # ... a short K keeps the streaming kernel (10.6 vs 11.1 us)
    (dict(M=24, gs=64), "gemm_w4_rows_kernel<32x16>"),
    (dict(M=4, gs=32, tuning=(0, 0, 0, 65536)), "gemm_wn_stream_kernel"),
    (dict(M=4, gs=32), "gemm_w4_rows_kernel<16x16>"),
    (dict(M=48, tuning=(0, 0, 0, 65536)), "gemm_w4_mma_kernel<64x64>"),       # (the round-4 choice) from 33 rows: the 8-wave MFMA kernel; 4096^2: 32-row tiles x 4 slices (15.8 us vs 16.4)  [round 4, late: narrow 64 x 64 tiles]
    (dict(M=48, N=11008, K=4096), "gemm_w4_mma_kernel<64x64>"),   # round 4: one row tile, 172 column tiles: unsplit 64 x 64 tiles (18.0 -> 16.5 us)
    (dict(M=48, N=11008, K=4096, tuning=(0, 0, 0, 16384)), "gemm_w4_mma_kernel<64x128>"),
    (dict(M=8, N=11008, K=4096), "gemm_wn_direct_kernel<tile64>"),   # wide N: 64-column tiles, K not split
    (dict(M=48, mt=3, tuning=(0, 0, 0, 65536)), "gemm_wn_stream_kernel"),      # manual GEMM_SPLITK at 33..64 rows: LDS-staged streaming kernel (the round-4 choice)
    (dict(M=48, mt=3), "gemm_w4_rows_kernel<48x16>"),      # round 5: the rows kernel IS the GEMM_SPLITK family's kernel at 4096^2
    (dict(M=48, nbits=2), "gemm_w2_rows_kernel<48x16>"),   # late round 5: the rows kernel on 2-bit words (12.2 -> 8.8 us)
    (dict(M=48, nbits=2, tuning=(0, 0, 0, 65536)), "gemm_w2_mma_kernel<64x64>"),   # (the round-4 choice)
    (dict(M=48, nbits=1), "gemm_w1_mma_kernel<64x128>"),
    (dict(M=200, nbits=8), "gemm_w8_mma_kernel<64x128>"),   # tallest tile with >= 128 tiles: at most two K slices
    (dict(M=48, tuning=(1, 0, 0, 0)), "gemm_wn_stream_kernel"),          # tuning[0] = 1: LDS-staged streaming kernel
    (dict(M=48, tuning=(2, 0, 0, 0)), "gemm_w4_tiled_kernel<128x128>"),  # tuning[0] = 2: the 4-wave kernel of round 1
    (dict(M=48, gs=32, tuning=(0, 0, 0, 65536)), "gemm_w4_mma_kernel<32x128,g32>"),     # group size 32 above 32 rows: the tile kernel's g32 form (round 6) whether or not the rows kernel is switched off
    (dict(M=8, nbits=1, gs=32), "gemm_w1_mma_kernel<32x128,g32>"),             # round 6: 1- and 8-bit packed words with groups of 32 at M >= 2 leave the coverage kernel
    (dict(M=200, nbits=8, gs=32), "gemm_w8_mma_kernel<32x128,g32>"),
    (dict(M=8, nbits=2, gs=32, K=4352), "gemm_w2_mma_kernel<32x128,g32>"),     # ... and 2-bit words whose K is not a multiple of 512 (the rows kernel's chunk)
    (dict(M=256, nbits=2, gs=32, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2), "gemm_a8w2_mma_kernel<32x128,g32>"),   # ... fp8 activations x packed words
    (dict(M=48, gs=32), "gemm_w4_mma_kernel<32x128,g32>"),   # round 6: groups of 32 above 32 rows on the tile kernel
    # K = 11008 / 8960 (Llama-2-7B down_proj, Qwen2.5-1.5B): specialised kernels at every M, never the coverage kernel
    (dict(M=1, N=4096, K=11008), "gemv_w4_decode3_kernel<tile16,16w>"),
    (dict(M=1, N=4096, K=11008, gs=64), "gemv_w4_decode3_kernel<tile16,16w>"),
    (dict(M=1, N=1536, K=8960), "gemv_w4_decode3_kernel<tile16,16w>"),   # round 3: narrow N -> 16-column tiles unsplit (7.5 vs 9.4 us)
    (dict(M=1, N=1024, K=4096), "gemv_w4_decode3_kernel<tile16,16w>"),
    (dict(M=1, N=5120, K=5120), "gemv_wn_kernel<tile32>"),              # 160 blocks are enough (7.6 vs 8.9 us for 320 blocks of 16 columns)
    (dict(M=1, N=14336, K=4096), "gemv_wn_kernel<tile64,8w>"),   # (late round 6: 64-column tiles take 8 waves from 32 chunks per slice: 8.05 -> 7.72 us)
    (dict(M=1, N=6144, K=4096), "gemv_wn_kernel<tile32>"),              # round 6: no MFMA GEMV at one row of 4-bit words any more (20 of 22 shapes)
    (dict(M=1, N=8960, K=1536), "gemv_wn_kernel<tile64>"),
    (dict(M=1, N=8192, K=28672), "gemv_wn_kernel<tile64,8w>"),             # long K over a narrow N: 64-column tiles x 2 K slices (23.1 vs 25.8 us)
    (dict(M=1, N=4096, K=14336), "gemv_wn_kernel<tile64>"),
    (dict(M=4, N=4096, K=11008), "gemm_w4_rows_kernel<16x16>"),   # round 5 (13.0 -> 12.3 us)
    (dict(M=8, N=4096, K=11008, tuning=(0, 0, 0, 65536)), "gemm_w4_mma_kernel<32x128>"),
    (dict(M=32, N=4096, K=11008, gs=64, tuning=(0, 0, 0, 65536)), "gemm_w4_mma_kernel<32x128>"),
    (dict(M=16, N=1536, K=8960), "gemm_w4_mma_kernel<32x128>"),
    (dict(M=64, N=4096, K=11008), "gemm_w4_mma_kernel<64x128>"),
    (dict(M=8, N=4864, K=896), "gemm_w4_mma_kernel<128x128>"),   # K = 128 * 7 (Qwen2.5-0.5B): only the 128-k-step tiles divide it
    (dict(M=1, N=1024, K=896), "gemv_wn_kernel<tile64,xdirect>"),
    (dict(M=256, N=4096, K=11008), "gemm_w4_mma_kernel<128x128>"),   # block-time model: 128 rows x 4 slices (40.5 vs 42.3 us for 64 x 2)
    (dict(M=1, nbits=2), "gemv_wn_kernel<tile16>"),   # round 6: 2-bit decode back on the dot-product family (4.47 vs 4.76 us) ...
    (dict(M=1, nbits=2, N=4096, K=11008), "gemv_w2_mfma_kernel<tile16>"),   # ... except over a K that is not a multiple of 1024 (8.29 vs 9.16 us)
    (dict(M=1, nbits=2, tuning=(0, 0, 0, 512)), "gemv_wn_kernel<tile16>"),
    (dict(M=1, N=11008, K=4096), "gemv_wn_kernel<tile64,8w>"),   # round 6: 64-column tiles (172 blocks) of the dot-product family: 7.70 vs 7.98 us
    (dict(M=1, N=11008, K=4096, tuning=(0, 0, 0, 512)), "gemv_wn_kernel<tile64,8w>"),
    (dict(M=1, nbits=8), "gemv_wn_kernel<tile64>"),
    (dict(M=1, N=16384, K=16384, nbits=2), "gemv_wn_kernel<tile64,8w>"),   # 2-bit, long K: two waves per SIMD
    (dict(M=16, tuning=(0, 0, 0, 65536)), "gemm_wn_direct_kernel<tile32,8w>"),
    (dict(M=1, mt=4), "gemm_w4_mma_kernel<32x128>"),   # manual GEMM family at M=1 -> the tiled MFMA kernel
    (dict(M=128), "gemm_w4_mma_kernel<64x64>"),        # round 4: 128 narrow tiles x 2 K slices (15.4 -> 13.7 us)
    (dict(M=256), "gemm_w4_mma_kernel<64x64>"),        # cfgA: 256 narrow tiles, K UNSPLIT: no slab + ticket combine (19.8 -> 16.8 us)
    (dict(M=256, tuning=(0, 0, 0, 16384)), "gemm_w4_mma_kernel<64x128>"),   # tuning[3] & 16384: the round-3 choice, 128 tiles x 2 K slices
    (dict(M=256, N=4096, K=11008), "gemm_w4_mma_kernel<128x128>"),   # 344 MB of x re-reads through L2: the narrow tiles lose (33.3 vs 36.5 us)
    (dict(M=256, N=8192, K=8192, in_dt=2), "gemm_w4_mma_kernel<128x128>"),   # cfgB
    (dict(M=256, tuning=(0, 0, 8, 0)), "gemm_w4_mma_kernel<256x128>"),   # tuning[2]: tile rows / 32
    (dict(M=256, tuning=(2, 0, 8, 0)), "gemm_w4_tiled_kernel<256x128>|ab"),   # built with `make AB=1` only
    (dict(M=256, tuning=(2, 0, 4, 0)), "gemm_w4_tiled_kernel<legacy>|ab"),
    (dict(M=2048, N=8192, K=8192, in_dt=2), "gemm_w4_mma_kernel<256x256>"),   # prefill: 256 x 256 tiles alone fill the chip
    (dict(M=1024, N=8192, K=8192, in_dt=2), "gemm_w4_mma_kernel<256x128>"),   # 128 wide tiles do not
    (dict(M=256, N=8192, K=8192, in_dt=2, tuning=(0, 4, 20, 0)), "gemm_w4_mma_kernel<128x256>"),   # tuning[2] = 16 + rows / 32
    (dict(M=4096, N=16384, K=16384, nbits=2), "gemm_w2_mma_kernel<256x256>"),
    (dict(M=256, nbits=2), "gemm_w2_mma_kernel<64x64>"),
    (dict(M=256, N=16384, K=16384, nbits=2), "gemm_w2_mma_kernel<256x128>"),   # BASELINE config 5
    (dict(M=4, mt=3), "gemm_wn_direct_kernel<tile16>"),  # manual GEMM_SPLITK
    (dict(M=1, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_decode_kernel<tile16,16w>"),  # round 4: one wave per column, the row in flight at once
    (dict(M=1, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(7, 0, 0, 0)), "kmajor_matmul_kernel"),
    (dict(M=1, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, K=4096 + 512), "kmajor_matmul_kernel"),  # K % 1024 != 0
    # A8W8 int8 / fp8, 2 .. 64 rows: 16-column blocks.  Round 6: x through LDS in whole cache lines (gemm_w8_rows.hip); tuning[3] & 524288 = the round-3 kernel
    (dict(M=16, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<16x16>"),
    (dict(M=16, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 0, 524288)), "a8w8_rows_kernel<16x16>"),
    (dict(M=2, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<16x16>"),
    (dict(M=2, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1, K=4096 + 64), "a8w8_rows_kernel<16x16>"),   # K % 256 != 0
    (dict(M=17, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<32x16>"),
    (dict(M=17, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 0, 524288)), "a8w8_rows_kernel<32x16>"),  # round 3: 2 / 4 row tiles while the x re-reads stay < 88 MB
    (dict(M=32, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<32x16>"),
    (dict(M=8, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<16x16,2/cu>"),   # more blocks than CUs: 64 KB of LDS, two blocks per CU
    (dict(M=3, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_kernel<16x16>"),            # ... from 4 rows
    (dict(M=16, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<16x16,2/cu>"),  # ... up to 16 (23.8 (tiles) -> 22.0 us)
    (dict(M=4, N=14336, K=4096, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_kernel<16x16>"),           # >= 192 column tiles of 64: round-3 kernel, then the tiles
    (dict(M=17, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),  # round 4: M N K > 800 M with >= 128 column tiles: the unsplit 64 x 64 tiles
    (dict(M=32, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),
    (dict(M=32, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(6, 0, 0, 0)), "gemm_a8w8_mma_kernel<32x128>"),  # (round 3: the 8-wave MFMA kernel)
    (dict(M=40, N=4096, K=14336, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<48x16>"),  # one round of blocks, 147 MB of x re-reads (budget 256 MB; 4096 x 14336 M = 32: 31.3 -> 25.7 us)
    (dict(M=40, N=4096, K=14336, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 0, 524288)), "gemm_a8w8_mma_kernel<32x128>"),  # (round 3: past the 88-MB budget the 8-wave kernel)
    (dict(M=64, N=4096, K=28672, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_mma_kernel<32x128>"),  # 470 MB: tiles
    (dict(M=16, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 1, 0)), "gemm_a8w8_mma_kernel<32x128>"),
    (dict(M=48, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<48x16>"),
    (dict(M=64, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "a8w8_rows_lds_kernel<64x16>"),   # (4096^2 M = 64: 17.2 -> 13.7 us with the quantiser launch)
    (dict(M=64, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 0, 524288)), "a8w8_rows_kernel<64x16>"),
    (dict(M=64, N=8192, K=8192, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),   # round 4 (39.5 -> 30.0 us)
    (dict(M=65, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),   # round 4: unsplit 64 x 64 tiles while they fit
    (dict(M=256, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),  # one round of CUs (config 4: 21.7 -> 13.6 us) ...
    (dict(M=256, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1, tuning=(6, 0, 0, 0)), "gemm_a8w8_lds_kernel<128x128>"),   # (tuning[0] = 6: the round-3 tile, both operands through LDS)
    (dict(M=256, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),   # ... two rounds up to K = 8192 (late round 6: 35.4 -> 32.7 us)
    (dict(M=512, N=4096, K=11008, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_lds_kernel<128x128>"),   # ... of a longer K: the 128-row tile with K slices (58.8 vs 43.7)
    (dict(M=384, N=8192, K=2048, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<128x128>"),   # late round 6: short K, 192 tiles of 128 x 128 (30.0 -> 17.9)
    (dict(M=128, N=4096, K=14336, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_lds_kernel<128x128>"),   # late round 6: very long K under 128 tiles (30.6 -> 27.5)
    (dict(M=256, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1, tuning=(0, 0, 0, 64)), "gemm_a8w8_mma_kernel<128x128>"),   # A/B switch
    (dict(M=512, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<64x64>"),   # two rounds at K = 4096: 2 stages, two blocks per CU
    (dict(M=1024, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<128x128>"),   # round 5: 256 unsplit 128 x 128 tiles (27.5 vs 32.2 us)
    (dict(M=1024, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(6, 0, 0, 0)), "gemm_a8w8_lds_kernel<128x128>"),   # (round 3; 256-row tiles would leave half the chip idle)
    (dict(M=512, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<128x128>"),   # 256 tiles again (47.0 vs 52.7 us)
    (dict(M=256, N=8192, K=8192, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(6, 0, 0, 0)), "gemm_a8w8_lds_kernel<128x128>"),  # (round 3: 128 tiles with K slices; 128 x 128 unsplit: 44 us)
    (dict(M=4096, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_lds_kernel<256x128>"),
    (dict(M=256, N=16384, K=16384, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1), "gemm_a8w8_sq_kernel<128x128>"),  # config 5, round 5: 256 unsplit 128 x 128 tiles (95.8 vs 98.5 us)
    (dict(M=256, N=16384, K=16384, nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=1, tuning=(6, 0, 0, 0)), "gemm_a8w8_lds_kernel<256x128>"),  # (round 3: 128 tiles x 2 slices of a long K)
    (dict(M=256, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(2, 0, 0, 0)), "gemm_a8w8_kernel<64x64>"),  # round-1 kernel
    (dict(M=256, nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, tuning=(1, 0, 0, 0)), "kmajor_matmul_kernel"),
    (dict(M=1, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096), "a16w8_decode_kernel<tile16,16w>"),   # A16W8 int8, pre-scale, one row (round 4)
    (dict(M=1, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(4, 0, 0, 0)), "a16w8_rows_kernel<16x16>"),
    (dict(M=2, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096), "a16w8_rows_kernel<16x16>"),   # from 2 rows: MFMA, weights converted in registers
    (dict(M=8, nbits=8, e=1, in_dt=2, w_dtype=3, w_mode=0, c_mode=1, gs=4096), "a16w8_rows_lds_kernel<16x16>"),  # fp8 W, bf16 x; round 6: from 4 rows x through LDS (gemm_w8_rows.hip)
    (dict(M=8, nbits=8, e=1, in_dt=2, w_dtype=3, w_mode=0, c_mode=1, gs=4096, tuning=(0, 0, 0, 524288)), "a16w8_rows_kernel<16x16>"),
    (dict(M=40, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096), "a16w8_rows_lds_kernel<48x16>"),
    (dict(M=64, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096), "a16w8_rows_lds_kernel<64x16>"),   # ahead of the tile kernel while the x re-reads stay < 256 MB (17.0 -> 12.7 us)
    (dict(M=64, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(0, 0, 0, 524288)), "gemm_a16w8_kernel<64x64>"),
    (dict(M=64, N=4096, K=14336, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=14336), "gemm_a16w8_kernel<64x128>"),   # 470 MB: the tile kernel (29.6 vs 34.3 us)
    (dict(M=16, N=8192, K=8192, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=8192), "a16w8_rows_lds_kernel<16x16,2/cu>"),  # more blocks than CUs: up to 16 rows ahead of the tiles (24.4 -> 21.7 us)
    (dict(M=24, N=8192, K=8192, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=8192), "gemm_a16w8_kernel<32x128>"),
    (dict(M=300, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096), "gemm_a16w8_kernel<128x128>"),  # above 64 rows: the MFMA tile kernel (late round 6: never the 64-row tiles there)
    (dict(M=65, nbits=8, e=1, in_dt=2, w_dtype=3, w_mode=0, c_mode=1, gs=4096), "gemm_a16w8_kernel<64x64>"),  # round 4, late: narrow 64 x 64 tiles where narrow_auto() fires
    (dict(M=300, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(4, 0, 0, 0)), "a16w8_rows_lds_kernel<64x16>"),  # 64-row tiles along grid.y
    (dict(M=300, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(4, 0, 0, 524288)), "a16w8_rows_kernel<64x16>"),
    (dict(M=1, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(7, 0, 0, 0)), "kmajor_w8a16_kernel"),  # A/B switch: rounds 1-3
    (dict(M=1, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096 + 16, K=4096 + 16), "kmajor_w8a16_kernel"),    # K % 64 != 0
    (dict(M=1, N=1000), "generic_matmul_kernel"),    # N not a multiple of 64
    (dict(M=1, in_dt=4, w_mode=1, c_mode=1, out_dt=0), "generic_matmul_kernel"),  # int8 x W4 with tensor zeros, fp32 out
    # 8-bit activations x packed weights (A8Wn fp8 dynamic, BitNet int8: helper.py:502-615, 1006-1062): fp8 / int8 MFMA
    (dict(M=1, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2), "gemv_a8w4_kernel<tile16,16w>"),   # decode: per-weight cast, no K split
    (dict(M=4, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=3, c_mode=2), "a8w4_rows_kernel<16x16>"),   # round 4: from 2 rows (the GEMV re-reads the weights per row pair)
    (dict(M=4, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=3, c_mode=2, tuning=(7, 0, 0, 0)), "gemv_a8w4_kernel<tile16,16w>"),  # A/B switch
    (dict(M=1, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2, tuning=(0, 0, 1, 0)), "gemm_a8w4_mma_kernel<32x128>"),
    (dict(M=1, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2, mt=4), "gemm_a8w4_mma_kernel<32x128>"),  # manual GEMM
    (dict(M=8, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2), "a8w4_rows_kernel<16x16>"),   # round 4: 5 .. 64 rows, 16-column blocks on the 16-row fp8 MFMA
    (dict(M=3, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2, tuning=(4, 0, 0, 0)), "a8w4_rows_kernel<16x16>"),
    (dict(M=100, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2), "gemm_a8w4_mma_kernel<64x64>"),  # round 4, late: narrow 64 x 64 tiles where narrow_auto() fires
    (dict(M=100, in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2, tuning=(0, 0, 32, 0)), "gemm_a8w4_mma_kernel<64x64>"),   # round 4, late: narrow tiles for 8-bit activations (forced)
    (dict(M=300, nbits=2, in_dt=4, out_dt=2, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3, gs=4096, tuning=(0, 2, 32, 0)), "gemm_a8w2_mma_kernel<64x64>"),
    (dict(M=300, nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096, tuning=(0, 0, 32, 0)), "gemm_a16w8_kernel<64x64>"),
    (dict(M=512, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2, N=8192, K=8192), "gemm_a8w4_mma_kernel<128x128>"),
    (dict(M=16, nbits=2, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2), "a8w2_rows_kernel<16x16>"),
    (dict(M=1, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=1, c_mode=3, gs=4096), "gemv_a8w4_kernel<tile16,16w>"),  # channel-wise, post-scale
    (dict(M=1, nbits=2, in_dt=4, out_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3, gs=4096), "gemv_a8w2_kernel<tile16,16w>"),  # BitNet int8, fp32 scale
    (dict(M=8, nbits=2, in_dt=4, out_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3, gs=4096), "a8w2_rows_kernel<16x16>"),   # BitNet int8: v_mfma_i32_16x16x64_i8
    (dict(M=300, nbits=2, in_dt=4, out_dt=2, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3, gs=4096), "gemm_a8w2_mma_kernel<64x128>"),
    (dict(M=1, in_dt=8, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2), "generic_matmul_kernel"),   # e5m2 activations: coverage kernel
    # 16-bit activations whose output / channel-scale type differs (BitNet A16W158 with its fp32 scale; fp32 output)
    (dict(M=1, nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gs=4096), "gemv_wn_kernel<tile16>"),   # round 4: fp32 post-scale in the GEMV epilogue
    (dict(M=8, nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gs=4096), "gemm_w2_rows_kernel<16x16>"),  # ... late round 5: the rows kernel reads fp32 channel scales in its epilogue
    (dict(M=8, nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gs=4096, tuning=(0, 0, 0, 65536)), "gemm_wn_direct_kernel<tile32,8w>"),  # (round 4: the few-row kernels)
    (dict(M=64, nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gs=4096), "gemm_w2_rows_kernel<64x16>"),
    (dict(M=64, nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gs=4096, tuning=(0, 0, 0, 65536)), "gemm_w2_mma_kernel<64x64>"),  # round 4, late: narrow 64 x 64 tiles where narrow_auto() fires
    (dict(M=64, in_dt=1, out_dt=0), "gemm_w4_mma_kernel<64x64>"),  # round 4, late: narrow 64 x 64 tiles where narrow_auto() fires
])
def test_kernel_selection(kw, kernel):
    lib = _hip.load()
    a = _args(**kw)
    if kw.get("c_mode", 0) in (2, 3):
        a.scales_x = 0x1000
    assert lib.gemlite_hip_query(C.byref(a)) == 0
    if kernel.endswith("|ab"):  # A/B-only variants: present when the library was built with GL_AB_KERNELS, else never chosen
        got = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
        if "+ab_kernels" in lib.gemlite_hip_build_info().decode():
            assert got == kernel[:-3]
        else:
            assert got != kernel[:-3] and "tiled_kernel<" not in got.replace("gemm_w4_tiled_kernel<128x128>", ""), got
        return
    assert lib.gemlite_hip_kernel_name(C.byref(a)).decode() == kernel


def test_planner_choices_on_llm_shapes():
    """The kernel the C ABI picks on 23 LLM layer shapes x M in {1, 2, 4, 6, 8, 16, 32, 64, 256} (4-bit) / {1, 16, 256} (2-bit) is
    frozen in tests/golden/planner_llm_shapes.json: the planner rules of round 3 come from GPU sweeps over exactly these shapes
    (profiles/r03/probe_*_llm_shapes_*.log), and a rule edited for one shape should not silently move the others.  To regenerate
    after an intended change: rows = [[nb, M, N, K, kernel_name(_args(M=M, N=N, K=K, nbits=nb, gs=128, in_dt=1, mt=-1))] ...]."""
    lib = _hip.load()
    fx = json.load(open(os.path.join(GOLDEN, "planner_llm_shapes.json")))["rows"]
    assert len(fx) >= 270
    moved = []
    for nb, M, N, K, want in fx:
        a = _args(M=M, N=N, K=K, nbits=nb, gs=128, in_dt=1, mt=-1)
        got = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
        if got != want:
            moved.append((nb, M, N, K, want, got))
        assert "generic" not in got, (nb, M, N, K, got)   # none of these shapes may reach the coverage kernel
    assert not moved, moved[:10]


FEW_ROW_KERNELS = ("_rows_kernel", "gemv_", "gemm_wn_direct", "gemm_wn_stream", "_decode", "kmajor")


@pytest.mark.parametrize("fam", ["a16w8", "a8w8", "a8w4", "bitnet_int8", "a16w4"])
def test_few_row_to_tile_hand_over_is_monotone(fam):
    """Round 4, late: every few-row kernel has an M N K budget against its tile kernel.  Walking M upwards on the four layer sizes
    of the sweep, the plan must hand over ONCE — after a tile kernel was chosen no larger M may fall back to a few-row kernel — nothing
    may reach the coverage kernel, and from 65 rows no few-row kernel may be left."""
    lib = _hip.load()
    kw = {"a16w8": dict(nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2),
          "a8w8": dict(nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1),
          "a8w4": dict(in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2),
          "bitnet_int8": dict(nbits=2, in_dt=4, out_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3),
          "a16w4": dict()}[fam]
    for N, K in ((4096, 4096), (8192, 8192), (4096, 14336), (14336, 4096)):
        kk = dict(kw)
        if fam in ("a16w8", "a8w8", "bitnet_int8"):
            kk["gs"] = K
        tiled_at = None
        for M in list(range(1, 66)) + [96, 128, 256, 512]:
            a = _args(M=M, N=N, K=K, **kk)
            if kk.get("c_mode", 0) in (2, 3):
                a.scales_x = 0x1000
            assert lib.gemlite_hip_query(C.byref(a)) == 0
            name = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
            assert "generic" not in name, (fam, N, K, M, name)
            few = any(t in name for t in FEW_ROW_KERNELS)
            if not few and tiled_at is None:
                tiled_at = M
            if tiled_at is not None:
                assert not few, (fam, N, K, M, name, "tile kernel since M = %d" % tiled_at)
        assert tiled_at is not None and tiled_at <= 65, (fam, N, K, tiled_at)


def test_planner_fuzz_never_crashes_and_realistic_shapes_stay_off_the_coverage_kernel():
    """scripts/fuzz_planner.py (CPU only: query / kernel_name / workspace_bytes): random families x M x (N, K) x tuning.  Every accepted
    request names a kernel and a sane workspace; with default tuning on realistic shapes (N % 128 == 0, K % 256 == 0, >= 1024) only
    group size 32 of the packed integer formats (M >= 2) may still land on a coverage kernel."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("fuzz_planner", os.path.join(os.path.dirname(GOLDEN), "..", "scripts", "fuzz_planner.py"))
    fz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fz)
    cnt, cov = fz.run(seed=7, iters=12000)
    assert cnt["status 0"] > 8000
    assert all(f.endswith("/g32") for f in cov), sorted(cov)


def _mx_args(M, N, K, in_dt, nbits, c_mode):
    """A block-scaled layer (e8m0 scale per 32 k, K-contiguous weights) as GemLiteLinear.pack() lays it out; never dereferenced."""
    a = _args(M=M, N=N, K=K, nbits=nbits, gs=32, in_dt=in_dt, w_mode=0, c_mode=c_mode, e=1 if nbits == 8 else 2)
    a.w_pack_bits, a.w_dtype = (0, 3) if nbits == 8 else (8, 5)
    a.output_dtype, a.meta_dtype = 2, 5
    a.stride_xm = K // 2 if in_dt == 17 else K
    a.stride_wk, a.stride_wn = 1, K if nbits == 8 else K // 2
    a.stride_sx_m = K // 32
    a.scales_x = 0x1000
    return a


@pytest.mark.parametrize("fam", ["a16w4", "a16w2", "a8w8i", "a8w8f", "a16w8", "mxfp8", "mxfp4"])
def test_flag_bits_outside_the_public_mask_are_ignored(fam):
    """tuning[3] bits outside GEMLITE_TF_PUBLIC_MASK (0x0FFFDFFF; 28 .. 31 are the planner's own, e.g. its K-order bit 30) change nothing
    the C ABI answers: status, kernel name and workspace size stay those of the same request without them."""
    lib = _hip.load()
    kw = {"a16w4": dict(), "a16w2": dict(nbits=2),
          "a8w8i": dict(nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, gs=4096),
          "a8w8f": dict(nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=2, gs=4096),
          "a16w8": dict(nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gs=4096)}.get(fam)
    for M in (1, 16, 256, 1024):
        for t3 in (0, 1 << 16, 1 << 22):
            answers = []
            for extra in (0, 1 << 28, 1 << 30, -(1 << 31)):
                tun = (0, 0, 0, t3 | extra)
                if kw is None:
                    a = _mx_args(M, 4096, 4096, 16 if fam == "mxfp8" else 17, 8 if fam == "mxfp8" else 4, 4)
                    a.tuning[3] = tun[3]
                else:
                    a = _args(M=M, tuning=tun, **kw)
                    if kw.get("c_mode", 0) in (2, 3):
                        a.scales_x = 0x1000
                st = lib.gemlite_hip_query(C.byref(a))
                answers.append((st, lib.gemlite_hip_kernel_name(C.byref(a)), lib.gemlite_hip_workspace_bytes(C.byref(a))))
            assert answers[0][0] == 0, (fam, M, t3, answers[0])
            assert answers[1:] == answers[:1] * 3, (fam, M, t3, answers)


def test_workspace_sizing_cfgA():
    lib = _hip.load()
    a = _args(M=1)
    a.tuning[0], a.tuning[1] = 4, 8  # 64-column tiles x split-K 8: slabs of 64 fp32 behind the fixed counter block
    assert lib.gemlite_hip_workspace_bytes(C.byref(a)) == 65536 * 4 + 64 * 8 * 64 * 4
    a.tuning[0], a.tuning[1] = 2, 0  # 16-column tiles never split K at this shape: no workspace at all
    assert lib.gemlite_hip_workspace_bytes(C.byref(a)) == 0
    a.tuning[0], a.tuning[1] = 4, 3  # 3 does not divide the K steps -> falls through to another kernel family
    assert lib.gemlite_hip_kernel_name(C.byref(a)).decode() != "gemv_wn_kernel<tile64>"


# ------------------------------------------------------------------------------ bit packing (host)
def test_bitpack_cpu_matches_reference_bits():
    z = np.load(os.path.join(GOLDEN, "bitpack.npz"))
    for nb in (1, 2, 4, 8):
        for pb in (8, 16, 32):
            if f"in_{nb}_{pb}" not in z.files:
                continue
            W = torch.from_numpy(z[f"in_{nb}_{pb}"])
            packed, e = bitpack.pack_weights_over_cols(W, nb, pb, True)
            assert e == pb // nb
            ref = torch.from_numpy(z[f"out_{nb}_{pb}"])
            assert packed.dtype == ref.dtype and torch.equal(packed.contiguous(), ref)
            back = bitpack.unpack_over_cols(packed.t().contiguous(), nb, W.shape[1])
            assert torch.equal(back, W)
    W = torch.randint(0, 4, (8, 64), dtype=torch.uint8)
    p64, e = bitpack.pack_weights_over_cols(W, 2, 64, False)
    assert e == 32 and p64.dtype == torch.int64 and torch.equal(bitpack.unpack_over_cols(p64, 2, 64), W)
    rows, e = bitpack.pack_weights_over_rows(W.t().contiguous(), 2, 32, False)
    assert torch.equal(bitpack.unpack_over_rows(rows, 2, 64), W.t())


# ---------------------------------------------------------------- pack(): modes, layout, meta_args
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_pack_matches_reference(case):
    cfg = case["cfg"]
    tdt = cfg["tdt"]
    nb = cfg["nb"]
    unpacked = case["meta_args"][4] == 1
    if unpacked:
        w_code = 1 if nb == 16 else (4 if cfg["in_dt"] == 4 else 3)
        W_in = as_torch(case["W_in"], w_code)
    else:
        W_in = torch.from_numpy(case["W_in"])
    sdt = 0 if case["scales_in"].dtype == np.float32 else tdt
    scales = as_torch(case["scales_in"], sdt) if cfg["scales_kind"] else None
    zeros = {0: None, 1: (int(case["zeros_in"][0]) if cfg["zeros_kind"] == 1 else None),
             2: as_torch(case["zeros_in"], tdt)}[cfg["zeros_kind"]]
    lin = GemLiteLinear(nb, None if cfg["gs"] < 0 else cfg["gs"], cfg["K"], cfg["N"], DType(cfg["in_dt"]),
                        DType(cfg["out_dt"]), scaled_activations=bool(cfg["scaled_act"]))
    lin.pack(W_in, scales, zeros, None, fma_mode=bool(cfg["fma"]), packing_bitwidth=None if cfg["pb"] < 0 else cfg["pb"])
    if case["name"] == "a8w4_int8_dyn_intzero":
        lin.meta_dtype = DType.FP32  # the golden generator applied the reference test's override
    assert lin.get_meta_args() == case["meta_args"]
    assert tuple(lin.W_q.shape) == case["W_q"].shape and list(lin.W_q.stride()) == list(case["W_q_stride"])
    w_ref = as_torch(case["W_q"], TORCH_DT_CODE(lin.W_q.dtype))
    assert torch.equal(lin.W_q.data.contiguous().view(torch.uint8), w_ref.contiguous().view(torch.uint8))
    for name in ("scales", "zeros"):
        mine, ref = getattr(lin, name).data, case[name]
        assert tuple(mine.shape) == ref.shape, name
        if ref.size:
            ref_t = as_torch(ref, TORCH_DT_CODE(mine.dtype))
            assert mine.dtype == ref_t.dtype, name
            assert torch.equal(mine.reshape(-1).view(torch.uint8), ref_t.reshape(-1).view(torch.uint8)), name
    sd = lin.state_dict()
    assert set(sd) >= {"W_q", "scales", "zeros", "metadata", "orig_shape"}
    lin2 = GemLiteLinear()
    lin2.load_state_dict(dict(sd))
    if case["name"] != "a8w4_int8_dyn_intzero":  # attribute overridden after pack(): saved metadata is older
        assert lin2.get_meta_args() == lin.get_meta_args()
    assert all(torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
               for a, b in zip(lin2.get_tensor_args(), lin.get_tensor_args()) if a.numel())


def TORCH_DT_CODE(dt):
    return gemlite_amd.dtypes.TORCH_TO_DTYPE[dt].value


def test_constructor_and_pack_errors():
    with pytest.raises(NotImplementedError):
        GemLiteLinear(3, 64, 128, 128)
    with pytest.raises(NotImplementedError):
        GemLiteLinear(4, 64, 100, 128)
    with pytest.raises(NotImplementedError):
        GemLiteLinear(4, 8, 128, 128)
    lin = GemLiteLinear(4, 64, 128, 64, DType.INT8, DType.FP32)
    with pytest.raises(Exception, match="INT8"):
        lin.pack(torch.zeros(64, 128, dtype=torch.uint8), torch.ones(64, 1), torch.full((64, 1), 0.5))
    lin = GemLiteLinear(4, 64, 128, 64)
    with pytest.raises(Exception, match="not packed"):
        lin.pack(torch.zeros(64, 128, dtype=torch.int32), None, None)


def test_forward_on_cpu_fails_loudly():
    """No silent fallback: CPU tensors are refused by the product path."""
    lin = GemLiteLinear(4, 64, 128, 64)
    lin.pack(torch.randint(0, 16, (64, 128), dtype=torch.uint8), torch.rand(128, 1).half(), torch.rand(128, 1).half())
    with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
        lin(torch.randn(1, 128).half())


def test_dispatch_thresholds_and_m_buckets():
    assert [get_matmul_type(m, 4) for m in (1, 2, 64, 65)] == ["GEMV_REVSPLITK", "GEMM_SPLITK", "GEMM_SPLITK", "GEMM"]
    assert get_matmul_type(1, 8) == "GEMV_SPLITK"
    buckets = [1, 2, 4, 8, 16, 24, 32, 48, 64, 96, 128, 192, 256, 384, 512, 768, 1024, 1536, 2048, 3072, 4096]
    assert sorted({get_closest_m(m) for m in range(1, 5000)}) == buckets
    assert get_closest_m(17) == 24 and get_closest_m(5000) == 4096


def test_config_shims(tmp_path):
    gemlite_amd.reset_config()
    gemlite_amd.set_autotune(False)
    assert gemlite_amd.core.AUTOTUNE.GEMM == "default"
    gemlite_amd.set_autotune("max", use_cuda_graph=True)
    assert gemlite_amd.core.AUTOTUNE.GEMV == "max" and gemlite_amd.core.AUTOTUNE.USE_CUDA_GRAPH
    f = tmp_path / "cfg.json"
    gemlite_amd.core.GEMLITE_HIP_CONFIG_CACHE["GEMM"] = {"(256, 4096, 4096, 128, 8, 104)": {"splitk": 2}}
    gemlite_amd.cache_config(str(f))
    gemlite_amd.reset_config()
    assert gemlite_amd.load_config(str(f)) and "GEMM" in gemlite_amd.core.GEMLITE_HIP_CONFIG_CACHE
    assert gemlite_amd.load_config(str(tmp_path / "missing.json"), print_error=False) is False
    gemlite_amd.set_autotune("fast", use_cuda_graph=False)


def test_tuning_table_lookup_and_json_round_trip(tmp_path):
    """GEMLITE_HIP_CONFIG_CACHE: reference-style keys, consulted per launch, persisted by cache_config / load_config."""
    from gemlite_amd import core
    core.GemLiteLinear.reset_config()
    a = _args(M=1)  # cfgA: N = K = 4096, 4-bit, group 128, e = 8, type_id 104
    a.type_id = 104
    assert core.lookup_tuning(-1, 1, a) is None
    key = core.config_key(1, 4096, 4096, 128, 8, 104)
    assert key == "(1, 4096, 4096, 128, 8, 104)" and core.config_key(100, 1, 2, 3, 4, 5).startswith("(128,")  # M bucket
    fam = core.config_family(-1, 1, 4)
    assert fam == "GEMV_REVSPLITK" and core.config_family(3, 1, 4) == "GEMM_SPLITK" and core.config_family(-1, 256, 4) == "GEMM"
    core.GEMLITE_HIP_CONFIG_CACHE.setdefault(fam, {})[key] = {"tuning": [2, 1, 8], "us": 4.7}
    assert core.lookup_tuning(-1, 1, a) == (2, 1, 8, 0)
    assert core.lookup_tuning(-1, 2, a) is None and core.lookup_tuning(4, 1, a) is None  # other bucket / other family
    path = str(tmp_path / "hints.json")
    core.GemLiteLinear.cache_config(path)
    core.GemLiteLinear.reset_config()
    assert core.lookup_tuning(-1, 1, a) is None
    assert core.GemLiteLinear.load_config(path) is not False
    assert core.lookup_tuning(-1, 1, a) == (2, 1, 8, 0)
    core.GemLiteLinear.reset_config()


def test_shipped_mi355x_table_is_well_formed_and_every_entry_selects_a_specialised_kernel():
    """gemlite_amd/configs/mi355x.json (measured on the MI355X by scripts/make_tuning_table.py, autoloaded by device name
    like the reference's configs/*.json, core.py:634-654): reference-style keys, 4 small ints per entry, and the planner
    accepts every entry at both ends of its M bucket (an entry it rejected would drop the shape to a slower family)."""
    import ast, json, os
    from gemlite_amd import core
    path = os.path.join(os.path.dirname(core.__file__), "configs", "mi355x.json")
    table = json.load(open(path))
    assert table and set(table) <= set(core.GEMLITE_MATMUL_TYPES)
    lib = _hip.load()
    n = 0
    for fam, entries in table.items():
        for key, e in entries.items():
            Mb, N, K, gs, eps, tid = ast.literal_eval(key)
            assert core.get_closest_m(Mb) == Mb and eps == 8 and tid == 104 and gs == 128
            t = e["tuning"]
            assert len(t) == 4 and all(isinstance(v, int) and 0 <= v < 256 for v in t) and t[3] & ~0x3 == 0 and e["us"] > 0
            lo = 1 if Mb == 1 else Mb // 2 + 1
            for M in (lo, Mb):
                assert core.config_family(-1, M, 4) == fam
                a = _args(M=M, N=N, K=K, tuning=tuple(t))
                assert lib.gemlite_hip_query(C.byref(a)) == 0
                name = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
                assert name.startswith(("gemv_wn", "gemv_w4_decode", "gemv_mfma", "gemm_wn_direct", "gemm_wn_stream", "gemm_w4_mma", "gemm_w4_tiled")), (key, t, M, name)
            n += 1
    assert n >= 5   # (round 3: five of the eleven cells fell to planner rules derived from the 22-shape sweep)


def test_helper_processors_select_the_reference_modes():
    """(W_group_mode, channel_scale_mode) per processor as in the reference's helper.py; host only."""
    from gemlite_amd import helper as H
    from gemlite_amd.dtypes import DType
    torch.manual_seed(0)
    W = (torch.randn(64, 128) / 30).half()
    lin = H.A16W8(device="cpu").from_weights(W)
    assert (lin.W_group_mode, lin.channel_scale_mode, lin.elements_per_sample, lin.W_q.dtype) == (2, 0, 1, torch.int8)
    assert tuple(lin.W_q.shape) == (128, 64) and lin.W_q.stride() == (1, 128)  # [K, N] view of the [N, K] tensor
    lin = H.A16W8(device="cpu", post_scale=True).from_weights(W)
    assert (lin.W_group_mode, lin.channel_scale_mode) == (0, 1)
    assert H.A16W8_FP8(device="cpu").from_weights(W).W_q.dtype == torch.float8_e4m3fn
    Wq = torch.randint(0, 16, (64, 128), dtype=torch.uint8)
    s, z = (torch.rand(128, 1) * 0.01 + 0.001).half(), (torch.rand(128, 1) * 15).half()
    lin = H.A8W4_HQQ_INT_dynamic(device="cpu").from_weights(Wq, s, z)
    assert (lin.W_group_mode, lin.channel_scale_mode, lin.group_size, lin.input_dtype, lin.scaled_activations) == (3, 2, 64, DType.FP8, True)
    lin = H.A8W4_HQQ_INT_dynamic(device="cpu").from_weights(Wq, s[:64], z[:64])  # one group per row: channel-wise
    assert (lin.W_group_mode, lin.channel_scale_mode) == (1, 3)
    Wt = torch.randint(-1, 2, (64, 128)).half()
    lin = H.A16W158_INT(device="cpu").from_weights(Wt, torch.tensor(0.02))
    assert (lin.W_nbits, lin.W_group_mode, lin.channel_scale_mode, int(lin.zeros.item()), lin.zeros.dtype) == (2, 1, 1, 1, torch.int32)
    lin = H.A8W158_INT_dynamic(device="cpu").from_weights(Wt, torch.tensor(0.02))
    assert (lin.W_group_mode, lin.channel_scale_mode, lin.input_dtype) == (1, 3, DType.INT8)

    class FakeHQQ:  # the attributes the reference reads from an HQQLinear
        def __init__(self):
            self.W_q, self.bias, self.in_features = torch.zeros(1), None, 128
            self.meta = dict(axis=1, nbits=4, group_size=64, shape=(64, 128), scale=s.clone(), zero=z.clone())

        def unpack(self, dtype):
            return Wq.reshape(128, 64).to(dtype)

    lin = H.A16W4_HQQ_INT(device="cpu").from_hqqlinear(FakeHQQ())
    assert (lin.W_group_mode, lin.channel_scale_mode, tuple(lin.W_q.shape)) == (4, 0, (16, 64))
    model = torch.nn.Sequential(torch.nn.Linear(128, 64), torch.nn.ReLU(), torch.nn.Linear(64, 32)).half()
    model.add_module("lm_head", torch.nn.Linear(32, 8).half())
    H.patch_model(model, "cpu", H.A16W8_INT8(device="cpu"))  # the reference's argument order
    assert type(model[0]).__name__ == "GemLiteLinearHIP" and isinstance(model.lm_head, torch.nn.Linear)
    with pytest.raises(NotImplementedError):
        H.patch_model(torch.nn.Sequential(torch.nn.Linear(8, 8)), "cpu", H.A16W4_HQQ_INT(device="cpu"))


def _bits(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).numpy()
    if t.dtype in (torch.float8_e4m3fn, torch.float8_e5m2):
        return t.view(torch.uint8).numpy()
    return t.numpy()


def test_helper_processors_match_the_reference_bit_for_bit():
    """tests/golden/helpers.npz holds what the reference's own processors produced on CPU for seeded inputs
    (oracle/gen_golden_helpers.py): packed / transposed W_q, scales, zeros, bias, meta_args, modes must be identical."""
    from gemlite_amd import helper as H
    z = np.load(os.path.join(GOLDEN, "helpers.npz"))
    W, bias = torch.from_numpy(z["in_W"]), torch.from_numpy(z["in_bias"])
    W_q4, s64, z64 = torch.from_numpy(z["in_W_q4"]), torch.from_numpy(z["in_s64"]), torch.from_numpy(z["in_z64"])
    sch, zch, Wt = torch.from_numpy(z["in_sch"]), torch.from_numpy(z["in_zch"]), torch.from_numpy(z["in_Wt"])
    wscale, fp8, K = torch.tensor(float(z["in_wscale"])), torch.float8_e4m3fn, W.shape[1]
    cases = {
        "a16w8_int8_pre": lambda: H.A16W8(device="cpu").from_weights(W.clone(), bias.clone()),
        "a16w8_int8_post": lambda: H.A16W8(device="cpu", post_scale=True).from_weights(W.clone()),
        "a16w8_fp8_pre": lambda: H.A16W8(device="cpu", fp8=fp8).from_weights(W.clone()),
        "a16wn_g64": lambda: H.A16Wn(device="cpu").from_weights(W_q4.clone(), s64.clone(), z64.clone(), 4, 64, bias.clone()),
        "a16wn_channel": lambda: H.A16Wn(device="cpu", post_scale=True).from_weights(W_q4.clone(), sch.clone(), zch.clone(), 4, K),
        "a8w8_int8_dyn": lambda: H.A8W8_dynamic(device="cpu", fp8=False).from_weights(W.clone(), bias.clone()),
        "a8w8_fp8_dyn": lambda: H.A8W8_dynamic(device="cpu", fp8=fp8).from_weights(W.clone()),
        "a8w4_dyn_g64": lambda: H.A8Wn_HQQ_INT_dynamic(device="cpu", fp8=fp8, W_nbits=4).from_weights(W_q4.clone(), s64.clone(), z64.clone()),
        "a8w4_dyn_channel": lambda: H.A8Wn_HQQ_INT_dynamic(device="cpu", fp8=fp8, W_nbits=4, post_scale=True).from_weights(W_q4.clone(), sch.clone(), zch.clone()),
        "a16w158": lambda: H.A16W158_INT(device="cpu").from_weights(Wt.clone(), wscale, bias.clone()),
        "a8w158_dyn": lambda: H.A8W158_INT_dynamic(device="cpu").from_weights(Wt.clone(), wscale),
    }
    assert sorted(cases) == sorted(str(n) for n in z["names"])
    for name, make in cases.items():
        lin = make()
        assert lin.get_meta_args() == [int(v) for v in z[f"{name}__meta"]], (name, lin.get_meta_args(), z[f"{name}__meta"])
        assert [lin.W_group_mode, lin.channel_scale_mode] == [int(v) for v in z[f"{name}__modes"]], name
        assert str(lin.W_q.dtype) == str(z[f"{name}__W_q_dtype"]) and list(lin.W_q.stride()) == [int(v) for v in z[f"{name}__W_q_strides"]], name
        assert np.array_equal(_bits(lin.W_q.data), z[f"{name}__W_q"]), name
        assert str(lin.scales.dtype) == str(z[f"{name}__scales_dtype"]), (name, lin.scales.dtype, z[f"{name}__scales_dtype"])
        assert np.array_equal(lin.scales.data.float().numpy(), z[f"{name}__scales"]), name
        assert str(lin.zeros.dtype) == str(z[f"{name}__zeros_dtype"]), (name, lin.zeros.dtype)
        assert np.array_equal(lin.zeros.data.float().numpy(), z[f"{name}__zeros"]), name
        ref_bias = z[f"{name}__bias"]
        assert (lin.bias is None and ref_bias.size == 0) or np.array_equal(lin.bias.data.float().numpy(), ref_bias), name


def test_host_lookup_tables_match_the_reference():
    """get_closest_m (autotune M buckets) and get_matmul_type for every M the reference was asked
    (tests/golden/host_tables.npz from oracle/gen_golden_helpers.py)."""
    from gemlite_amd import core
    z = np.load(os.path.join(GOLDEN, "host_tables.npz"))
    mine = np.array([core.get_closest_m(int(m)) for m in z["Ms"]], np.int64)
    bad = np.nonzero(mine != z["closest_m"])[0]
    assert bad.size == 0, (bad[:10], mine[bad[:10]], z["closest_m"][bad[:10]])
    kinds = [str(k) for k in z["kinds"]]
    for nb in (1, 2, 4, 8):
        got = [kinds.index(core.get_matmul_type(int(m), nb)) for m in z["Ms"][1:200]]
        assert got == [int(v) for v in z[f"matmul_type_w{nb}"]], nb


def test_constructor_validation_matches_the_reference_on_a_grid():
    """GemLiteLinear.__init__ accepts / rejects (and derives group_size, unpack_mask, scaled_activations, acc / meta
    dtype) exactly like the reference over 1176 argument combinations (tests/golden/ctor_grid.npz)."""
    import itertools
    grid = dict(W_nbits=(1, 2, 3, 4, 8, 16), group_size=(None, 8, 16, 32, 64, 100, 128), in_features=(64, 96, 100, 4096),
                dtype=("FP32", "FP16", "BF16", "FP8", "INT8", "FP8e5", "UINT8"))
    rows = [str(r) for r in np.load(os.path.join(GOLDEN, "ctor_grid.npz"))["rows"]]
    combos = list(itertools.product(*grid.values()))
    assert len(rows) == len(combos)
    for (nb, gs, k, dt), want in zip(combos, rows):
        try:
            lin = GemLiteLinear(nb, gs, k, 64, getattr(DType, dt), DType.FP16, scaled_activations=True)
            got = f"ok|{lin.group_size}|{lin.unpack_mask}|{int(lin.scaled_activations)}|{lin.acc_dtype.value}|{lin.meta_dtype.value}"
        except Exception as e:  # noqa: BLE001
            got = type(e).__name__
        assert got == want, ((nb, gs, k, dt), got, want)


def test_pack_decisions_match_the_reference_on_a_grid():
    """pack() over 432 combinations of scale / zero kinds, fma mode, input dtype and activation scaling: the modes,
    meta_args, dtypes / shapes / sums of the stored metadata — or the exception class — equal the reference's
    (tests/golden/pack_grid.npz, inputs re-created by oracle/gen_golden_helpers.py::pack_inputs)."""
    import importlib.util
    import itertools
    spec = importlib.util.spec_from_file_location("_ggh", os.path.join(ROOT, "oracle", "gen_golden_helpers.py"))
    src = open(spec.origin).read()
    ns = {}
    # only the grid definition and the seeded input builder are needed (the module itself imports the reference)
    start, end = src.index("PACK_GRID = dict("), src.index("def pack_grid(")
    exec("import torch\n" + src[start:end], ns)
    rows = [str(r) for r in np.load(os.path.join(GOLDEN, "pack_grid.npz"))["rows"]]
    combos = list(itertools.product(*ns["PACK_GRID"].values()))
    assert len(rows) == len(combos)
    bad = []
    for (nb, sk, zk, fma, dt, sa), want in zip(combos, rows):
        if sk == "none" and zk == "tensor":
            # tensor zeros without scales is not a working configuration in the reference (fma mode dereferences
            # `scales`: AttributeError; otherwise it records mode 3 without scales); here it is "shift only", mode 1
            assert want == "AttributeError" or want.startswith("ok|3|")
            continue
        W_q, scales, zeros = ns["pack_inputs"](nb, sk, zk)
        gs = 128 if sk == "channel" else 64
        try:
            lin = GemLiteLinear(nb, gs, 128, 16, getattr(DType, dt), DType.FP16, scaled_activations=sa)
            lin.pack(W_q, scales, zeros, None, fma_mode=fma)
            got = "|".join(str(v) for v in (
                "ok", lin.W_group_mode, lin.channel_scale_mode, lin.get_meta_args(), str(lin.scales.dtype), tuple(lin.scales.shape),
                str(lin.zeros.dtype), tuple(lin.zeros.shape), float(lin.zeros.float().sum()), float(lin.scales.float().sum())))
        except Exception as e:  # noqa: BLE001
            got = type(e).__name__
        if got != want:
            bad.append(((nb, sk, zk, fma, dt, sa), got, want))
    assert not bad, (len(bad), bad[:4])


def test_c_consumer_links_and_queries(tmp_path):
    """include/gemlite_hip.h is valid C99 and a plain-C program can link the library and use the host-only entry points."""
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("gcc not available")
    _hip.load()
    exe = str(tmp_path / "abi_smoke")
    libdir = os.path.dirname(_hip.LIB_PATH)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c_abi", "abi_smoke.c"), "-o", exe, "-L", libdir, "-lgemlite_hip",
                    f"-Wl,-rpath,{libdir}"], check=True, capture_output=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "gemv_w4_decode3_kernel<tile16,16w>" in out and "libgemlite_hip gfx950" in out


def _from_bits(arr, dtype_str):
    t = torch.from_numpy(np.array(arr))
    if dtype_str == "torch.bfloat16":
        return t.view(torch.bfloat16)
    if dtype_str == "torch.float8_e4m3fn":
        return t.view(torch.float8_e4m3fn)
    return t


def test_dtype_codes_and_state_dict_format_match_the_reference():
    """DType members / codes, and the reference's own state_dict() of three packed layers: loading it here gives the same
    meta_args and tensors, and this package's state_dict() of the same layer has the same keys, dtypes and bits."""
    from gemlite_amd import helper as H
    z = np.load(os.path.join(GOLDEN, "state_dicts.npz"))
    ref_codes = {str(n): int(v) for n, v in zip(z["dtype_names"], z["dtype_values"])}
    mine = {d.name: d.value for d in DType}
    assert mine == ref_codes
    W_q, sc = torch.from_numpy(z["sd_in_W_q"]), torch.from_numpy(z["sd_in_scales"])
    zr, bias = torch.from_numpy(z["sd_in_zeros"]), torch.from_numpy(z["sd_in_bias"])
    built = GemLiteLinear(4, 128, 256, 32, DType.FP16, DType.FP16)
    built.pack(W_q, sc, zr, bias)
    for name in ("a16w4", "a8w8", "bitnet"):
        keys = [str(k) for k in z[f"sd_{name}__keys"]]
        sd = {k: _from_bits(z[f"sd_{name}__{k}"], str(z[f"sd_{name}__{k}__dtype"])) for k in keys}
        lin = GemLiteLinear()
        lin.load_state_dict(dict(sd))
        assert lin.get_meta_args() == [int(v) for v in z[f"sd_{name}__meta_args"]], name
        assert torch.equal(lin.W_q, sd["W_q"]) and torch.equal(lin.scales, sd["scales"]) and torch.equal(lin.zeros, sd["zeros"])
        if name == "a16w4":  # the same layer packed here serialises to the same dictionary
            mine_sd = built.state_dict()
            assert list(mine_sd.keys()) == keys
            for k in keys:
                assert str(mine_sd[k].dtype) == str(z[f"sd_{name}__{k}__dtype"]), k
                assert np.array_equal(_bits(mine_sd[k]), z[f"sd_{name}__{k}"]), k


def test_forward_functional_is_registered_under_the_reference_namespace_with_a_fake_impl():
    """Reference: @torch.library.custom_op("gemlite::forward_functional") + register_fake (core.py:128-135,197-206).
    hqq / vLLM resolve torch.ops.gemlite.forward_functional; the fake impl must give shape/dtype without touching data."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    import gemlite_amd.core  # noqa: F401 (registers the op)
    op = torch.ops.gemlite.forward_functional
    assert "gemlite::forward_functional" in str(op.default._schema)
    meta = [0, 4, 64, 15, 8, 1, 1, 0, 1, 0, 4, 1]
    with FakeTensorMode():
        x = torch.empty(3, 5, 64, dtype=torch.float16)
        W = torch.empty(8, 32, dtype=torch.int32)
        s = torch.empty(1, 32, dtype=torch.float16)
        z = torch.empty(1, 32, dtype=torch.float16)
        y = op(x, None, [W, s, z], meta, -1)
        assert tuple(y.shape) == (3, 5, 32) and y.dtype == torch.float16
    # schema: (Tensor x, Tensor? bias, Tensor[] tensor_args, int[] meta_args, int matmul_type=-1) -> Tensor
    sch = op.default._schema
    assert [a.name for a in sch.arguments] == ["x", "bias", "tensor_args", "meta_args", "matmul_type"]


def test_launch_templates_are_immutable_and_keyed_by_everything_they_hold():
    """a shared mutable per-layer struct raced between threads and could go stale.  Now: an immutable byte
    template per layer, copied per call; the key carries addresses, shapes, strides, dtypes and the meta ints."""
    from gemlite_amd import core
    W = torch.zeros(8, 32, dtype=torch.int32)
    s = torch.ones(1, 32, dtype=torch.float16)
    z = torch.ones(1, 32, dtype=torch.float16)
    meta = [0, 4, 64, 15, 8, 1, 1, 0, 1, 0, 4, 1]
    a, b = core._static_args(W, s, z, meta), core._static_args(W, s, z, meta)
    assert a is not b and bytes(a) == bytes(b)
    a.M, a.x = 7, 0x1234  # per-call fields of one struct never leak into the next
    c = core._static_args(W, s, z, meta)
    assert c.M == 0 and not c.x
    k1 = core._template_key(W, s, z, meta)
    assert core._template_key(W, s.float(), z, meta) != k1            # dtype is part of the key
    assert core._template_key(W.t().contiguous().t(), s, z, meta) != k1  # so are the strides (and the address)
    assert core._template_key(W, s, z, meta[:-1] + [0]) != k1
    assert core.lookup_tuning(-1, 1, a) is None
    core.GEMLITE_HIP_CONFIG_CACHE.setdefault("GEMV_REVSPLITK", {})[core.config_key(1, a.N, a.K, 64, 8, a.type_id)] = {"tuning": [2, 1, 16, 7]}
    try:
        assert core.lookup_tuning(-1, 1, a) == (2, 1, 16, 3)  # development bits of tuning[3] are not loadable from a table
    finally:
        core.GemLiteLinear.reset_config()


def test_built_library_is_up_to_date_with_its_sources():
    """`make -q`: the in-tree libgemlite_hip.so (what travels to the GPU box) is newer than every source — a source edit that
    does not compile leaves the previous library behind, and every other test would pass on it."""
    import subprocess
    import gemlite_amd
    csrc = os.path.join(os.path.dirname(gemlite_amd.__file__), "csrc")
    rc = subprocess.run(["make", "-q", "-C", csrc], capture_output=True).returncode
    assert rc == 0, "gemlite_amd/csrc is newer than libgemlite_hip.so: run `python -c 'import __graft_entry__ as g; g.build()'`"


def test_isa_guard_no_scratch_or_spills_in_the_built_kernels():
    """scripts/isa_guard.py over the resource remarks of the build (gemlite_amd/csrc/build/*.remarks): only the known fallback
    kernels may touch scratch memory."""
    import subprocess
    if not os.path.isdir(os.path.join(ROOT, "gemlite_amd", "csrc", "build")):
        pytest.skip("no build directory (prebuilt library only)")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "isa_guard.py")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 new" in out.stdout


@pytest.mark.parametrize("script", ["isa_loops.py", "isa_asmloads.py"])
def test_isa_loop_guards_on_the_built_library(script):
    """scripts/isa_loops.py: no full `s_waitcnt vmcnt(0)` inside an arithmetic loop of a hot kernel outside the known list (real loop
    detection: dominators + back edges); scripts/isa_asmloads.py: no register of an inline-asm load is touched before the counted
    wait that covers it (the MFMA tile kernel retires its weight loads by hand).  Exit code 2 = the tools are not there: skip."""
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)], capture_output=True, text=True)
    if out.returncode == 2:
        pytest.skip(out.stdout.strip())
    assert out.returncode == 0, out.stdout + out.stderr


def test_in_launch_activation_quantisation_is_planned_from_two_rows_and_says_when_it_is_not():
    """include/gemlite_hip.h: scales_x == NULL with 16-bit x and unpacked 8-bit weights (channel_scale_mode 2 / 3) asks for the
    quantisation inside the matmul launch.  M = 1: the fused GEMV; 2 <= M: a launch whose first blocks quantise the rows
    for it (2 <= M <= 64: producer blocks in front of the rows kernel; workspace = flags + M K bytes + M floats); where neither applies the answer is GEMLITE_ERR_NO_FUSED_QUANT (-7),
    which core._forward_impl turns into quantiser + matmul — never an exception."""
    lib = _hip.load()

    def ask(M, N=4096, K=4096, w=4, **kw):
        a = _args(M=M, N=N, K=K, nbits=8, gs=K, in_dt=1, w_mode=0, c_mode=3, e=1, w_dtype=w, meta_dt=0, **kw)
        a.scales_x = None
        return lib.gemlite_hip_query(C.byref(a)), lib.gemlite_hip_kernel_name(C.byref(a)).decode(), int(lib.gemlite_hip_workspace_bytes(C.byref(a)))

    assert ask(1)[:2] == (0, "a8w8_decode_fused_quant_kernel<tile16,16w>")
    assert ask(1, tuning=(7, 0, 0, 0))[:2] == (0, "kmajor_fused_quant_kernel")  # the round-2 kernel (quantises before it asks for weights)
    assert ask(1, K=4096 + 512)[:2] == (0, "kmajor_fused_quant_kernel")         # K % 1024 != 0
    for w in (4, 3):  # int8, fp8 e4m3
        assert ask(2, w=w)[:2] == (0, "a8w8_rows_fq_kernel<16x16>")
        assert ask(17, w=w)[:2] == (0, "a8w8_rows_fq_kernel<32x16>")
        assert ask(64, w=w)[:2] == (0, "a8w8_rows_fq_kernel<64x16>")
        assert ask(65, w=w)[0] == _hip.ERR_NO_FUSED_QUANT   # the tile kernels: every block would be a producer, the chain in front of
        assert ask(256, w=w)[0] == _hip.ERR_NO_FUSED_QUANT  # its own pipeline — measured slower than two launches (profiles/r04)
    rc, _, ws = ask(64)
    assert ws == 65536 * 4 + 64 * 4096 + 256  # ticket words | quantised rows | scales (padded to 256)
    assert ask(32, N=16384, K=16384)[0] == _hip.ERR_NO_FUSED_QUANT       # past the rows kernel's x re-read budget: the 8-wave kernel
    assert ask(16, tuning=(0, 2, 0, 0))[0] == _hip.ERR_NO_FUSED_QUANT    # a forced plan keeps the two-launch form
    a = _args(M=16, nbits=4, gs=128, in_dt=1, w_mode=3, c_mode=2)        # packed weights (A8Wn): scales_x stays mandatory
    a.scales_x = None
    assert lib.gemlite_hip_query(C.byref(a)) == _hip.ERR_BAD_ARGUMENT
    assert b"scales_x" in lib.gemlite_hip_status_string(_hip.ERR_NO_FUSED_QUANT)


def test_warmup_takes_the_reference_arguments():
    """helper.warmup(processor, shapes, batch_sizes, group_size, dtype) (reference: helper.py:1067-1118).  Without a GPU it loads the
    library and returns; with one it runs every (shape, batch size) once (tests/test_gpu_parity.py)."""
    import inspect
    from gemlite_amd import helper
    assert list(inspect.signature(helper.warmup).parameters)[:5] == ["processor", "shapes", "batch_sizes", "group_size", "dtype"]
    assert helper.warmup() is None
    assert helper.warmup(helper.A16W8(device="cpu"), shapes=[(64, 64)], batch_sizes=[1]) is None


def test_tuning_table_mutations_bump_the_epoch_of_the_cpp_fast_path():
    """core.GEMLITE_HIP_CONFIG_CACHE counts its mutations (also those of the family dicts inside it): the C++ eager path caches tuning[]
    per (layer, M) for one epoch only."""
    from gemlite_amd import core
    e0 = core._CACHE_EPOCH[0]
    try:
        fam = core.GEMLITE_HIP_CONFIG_CACHE.setdefault("GEMM", {})
        e1 = core._CACHE_EPOCH[0]
        fam["(1, 2, 3, 4, 5, 6)"] = {"tuning": [0, 0, 0, 0]}
        e2 = core._CACHE_EPOCH[0]
        core.GEMLITE_HIP_CONFIG_CACHE.update({"GEMV": {"k": {"tuning": [1, 0, 0, 0]}}})
        core.GEMLITE_HIP_CONFIG_CACHE["GEMV"]["k2"] = {"tuning": [2, 0, 0, 0]}
        e3 = core._CACHE_EPOCH[0]
        assert e0 < e1 < e2 < e3
        assert json.loads(json.dumps(core.GEMLITE_HIP_CONFIG_CACHE))["GEMV"]["k2"]["tuning"][0] == 2   # still a plain JSON object
    finally:
        core.GemLiteLinear.reset_config()
    assert core._CACHE_EPOCH[0] > e3 and not core.GEMLITE_HIP_CONFIG_CACHE


def test_rows_kernel_bit_tricks_restate_natural_k_order():
    """The integer identities gemm_wn_rows.hip builds its MFMA B fragments with, restated in numpy: (i) a 16-bit half of a 2-bit word spread to
    eight nibbles by three shift-or + and steps holds q0 .. q7 in order; (ii) t_lo / t_hi + the byte selectors 0x0C040C00 + p * 0x00010001 of
    v_perm_b32, OR-ed with the magic halves, give the fp16 / bf16 codes OFF + q_2p, OFF + q_2p+1 of pair p — k in natural order, which is
    why the A fragment is x as it lies in memory."""
    rng = np.random.default_rng(3)
    halves = rng.integers(0, 1 << 16, size=4096, dtype=np.uint64)
    w = halves.copy()
    w = (w | (w << 8)) & 0x00FF00FF
    w = (w | (w << 4)) & 0x0F0F0F0F
    w = (w | (w << 2)) & 0x33333333
    for i in range(8):
        assert np.array_equal((w >> (4 * i)) & 0xF, (halves >> (2 * i)) & 0x3), i

    def v_perm(s0, s1, sel):  # byte k of the result = byte sel_k of the 8-byte value {s0 (bytes 4..7), s1 (bytes 0..3)}; selector 0x0C = 0x00
        src = [(s1 >> (8 * b)) & 0xFF for b in range(4)] + [(s0 >> (8 * b)) & 0xFF for b in range(4)]
        out = np.zeros_like(s0)
        for k in range(4):
            sk = (sel >> (8 * k)) & 0xFF
            out |= (np.zeros_like(s0) if sk == 0x0C else src[sk]) << (8 * k)
        return out

    words = rng.integers(0, 1 << 32, size=4096, dtype=np.uint64)
    t_lo, t_hi = words & 0x0F0F0F0F, (words >> 4) & 0x0F0F0F0F
    for magic, off in ((0x64006400, 1024), (0x43004300, 128)):
        for p_ in range(4):
            frag = v_perm(t_hi, t_lo, 0x0C040C00 + p_ * 0x00010001) | magic
            lo, hi = frag & 0xFFFF, frag >> 16
            q0, q1 = (words >> (8 * p_)) & 0xF, (words >> (8 * p_ + 4)) & 0xF
            if off == 1024:   # fp16: 0x6400 | q = 1024 + q exactly
                assert np.array_equal(lo.astype(np.uint16).view(np.float16).astype(np.float64), 1024.0 + q0)
                assert np.array_equal(hi.astype(np.uint16).view(np.float16).astype(np.float64), 1024.0 + q1)
            else:             # bf16: 0x4300 | q = 128 + q exactly (the upper half of the fp32 pattern)
                assert np.array_equal((lo.astype(np.uint32) << 16).view(np.float32).astype(np.float64), 128.0 + q0)
                assert np.array_equal((hi.astype(np.uint32) << 16).view(np.float32).astype(np.float64), 128.0 + q1)


def test_w8_rows_lds_layout():
    """The LDS image of an x piece in w8_rows_lds_kernel (gemm_w8_rows.hip), restated in numpy for every geometry the planner can pick
    (x bytes 2 / 1, row tiles 1 .. 4, 8-KB and 4-KB buffers): (i) an A fragment read back through the XOR swizzle holds exactly the k-values
    the weight register of the same lane faces — 16-bit x: the lane's sixteen k as the two 16-byte slots 2 kb + e; 8-bit x: slot kb — and (ii)
    every ds_read_b128 is conflict-free: its four lane groups (MI355X_MICROARCH.md, section LDS) touch sixteen distinct 16-byte slots of the
    256-byte bank row."""
    GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
              list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]

    def fswz(ppr, a16, j):
        if ppr >= 16:
            return j & 15
        return (((j >> 1) & 7) ^ ((((j + 4) >> 3) & 1) << 1)) if a16 else ((j >> 1) & 7)

    seen = set()
    for xb in (2, 1):
        a16 = xb == 2
        for mt, bufcap in ((1, 8192), (2, 8192), (3, 8192), (4, 8192), (1, 4096), (2, 4096)):
            per = bufcap // (16 * mt)
            cap = 512 if per >= 512 else (256 if per >= 256 else 128)
            rowb = min(256 * xb, cap)
            bpp, ppr, rpi = rowb // (64 * xb), rowb // 16, 1024 // rowb
            dpi = 16 * mt // rpi
            assert bpp >= 1 and 4 % bpp == 0 and dpi * rpi == 16 * mt and dpi * 1024 <= bufcap
            seen.add((xb, rowb, dpi))
            rows = 16 * mt
            # x piece: element value = row * 4096 + k (k counted in ELEMENTS inside the piece); 16-byte slot s of a row = elements [s * 16 / xb, ...)
            eps = 16 // xb  # elements per slot
            lds = np.full(dpi * 1024 // 16, -1, dtype=np.int64)  # per 16-byte slot: (row, logical slot) encoded
            for q in range(dpi):
                for lane in range(64):
                    r, pp = q * rpi + lane // ppr, lane % ppr
                    logical = pp ^ fswz(ppr, a16, r & 15)
                    assert 0 <= logical < ppr
                    lds[(q * 1024 + lane * 16) // 16] = r * 1024 + logical
            assert (lds >= 0).all() and len(set(lds.tolist())) == rows * ppr  # every (row, slot) exactly once
            for t in range(mt):
                for bq in range(bpp):
                    for e in range(2 if a16 else 1):
                        addrs = []
                        for lane in range(64):
                            j, kb = lane & 15, lane >> 4
                            xbase = (t * 16 + j) * rowb + ((((2 if a16 else 1) * kb) ^ fswz(ppr, a16, j)) << 4)
                            addr = xbase ^ (((8 * bq + e) if a16 else (4 * bq)) << 4)
                            assert addr % 16 == 0 and addr < dpi * 1024
                            got = lds[addr // 16]
                            want_slot = (8 * bq + 2 * kb + e) if a16 else (4 * bq + kb)
                            # the weight register of this lane: k = 64 bq + 16 kb .. + 15 -> x elements 64 bq + 16 kb + 8 e .. (16-bit) / 64 bq + 16 kb .. (8-bit)
                            first_k = 64 * bq + 16 * kb + (8 * e if a16 else 0)
                            assert want_slot * eps == first_k
                            assert got == (t * 16 + j) * 1024 + want_slot, (xb, mt, bufcap, t, bq, e, lane)
                            addrs.append(addr)
                        for grp in GROUPS:
                            banks = [(addrs[l] // 16) % 16 for l in grp]
                            assert len(set(banks)) == 16, (xb, mt, bufcap, t, bq, e, sorted(banks))
    assert len(seen) >= 7, seen


def test_group_index_by_multiply_high():
    """gs_magic (plan_forward.hip, round 6): the tile kernel finds the metadata row of a 32-k slice of a group size that is a multiple of 32 and not a power
    of two as mulhi(k / 32, ceil(2^32 / (group / 32))).  Exact for every slice of every (K, group) pair the planner admits (K * group < 2^40)."""
    rng = np.random.default_rng(9)
    for gs in [96, 160, 192, 224, 288, 320, 384, 480, 768, 1056, 3 * 4096, 5 * 8192, 96 * 341]:
        d = gs // 32
        magic = ((1 << 32) + d - 1) // d
        assert magic < (1 << 32)
        kmax = min((1 << 40) // gs, 1 << 31)
        q = np.concatenate([np.arange(0, min(kmax // 32, 1 << 16), dtype=np.uint64), rng.integers(0, kmax // 32, size=1 << 16, dtype=np.uint64),
                            np.array([kmax // 32 - 1], dtype=np.uint64)])
        assert np.array_equal((q * np.uint64(magic)) >> np.uint64(32), q // np.uint64(d)), gs


def test_k_order_is_a_permutation_of_the_k_steps():
    """k_order() (gl_async.h, round 6): the order in which row tile mt of a weight column tile walks its K steps — whole-K rotation or groups of 2^gsh steps
    rotated inside every run of mtiles groups, plain order in a tail of fewer than mtiles groups.  Restated here: for every (nsteps, mtiles, mode) it must
    visit every step exactly once, and in the grouped mode each row tile must LEAD (be the first to reach) a different group of every full run."""
    def k_order(step, mt, mtiles, nsteps, gm):
        if mtiles < 2:
            return step
        if gm == 0:
            k = step + (mt * nsteps) // mtiles
            return k - nsteps if k >= nsteps else k
        gsh = gm - 1
        g, i = step >> gsh, step & ((1 << gsh) - 1)
        magic = ((1 << 32) + mtiles - 1) // mtiles          # the kernel's quotient: one scalar multiply-high
        base = ((g * magic) >> 32) * mtiles
        assert base == (g // mtiles) * mtiles
        if base + mtiles <= (nsteps >> gsh):
            r = g - base + mt
            g = base + (r - mtiles if r >= mtiles else r)
        return (g << gsh) + i

    for nsteps in list(range(1, 40)) + [56, 64, 112, 128]:
        for mtiles in (1, 2, 3, 4, 5, 8):
            for gm in (0, 1, 2, 3, 4):
                orders = [[k_order(s, mt, mtiles, nsteps, gm) for s in range(nsteps)] for mt in range(mtiles)]
                for o in orders:
                    assert sorted(o) == list(range(nsteps)), (nsteps, mtiles, gm)
                if gm >= 1 and mtiles >= 2:
                    G = 1 << (gm - 1)
                    for run in range((nsteps // G) // mtiles):
                        first = [orders[mt][run * mtiles * G] // G for mt in range(mtiles)]   # the group each tile starts the run with
                        assert sorted(first) == list(range(run * mtiles, run * mtiles + mtiles)), (nsteps, mtiles, gm, run)
