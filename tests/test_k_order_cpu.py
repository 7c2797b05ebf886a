"""K order of the unsplit 8-bit tiles, host side (no GPU): the rule the kernels compile and the planner's choice of it.

`gemlite_hip_k_order_step` evaluates `KOrder` of csrc/gl_async.h — the very struct gemm_a8w8_sq_kernel<64x64> / <128x128> and
gemm_mx_*_sq_kernel call per request — compiled for the host; `gemlite_hip_k_order_mode` plans a request and reports the order the planned
kernel is launched with (-1 plain, 0 whole-K rotation, 1 .. 15 the group field).  tests/test_host_cpu.py keeps a Python restatement of the
arithmetic; here the library's answer is checked against it and against the properties the kernels rely on.  tests/test_k_order_gpu.py
launches every order."""
import ctypes as C
import os
import re

import pytest

from gemlite_amd import _hip
from tests.test_host_cpu import _args, _mx_args

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gemlite_amd", "csrc")
NO_K_ROTATION, REQUESTS_FIRST, ROUND5_EPILOGUE = 4194304, 2097152, 262144
INT8, E4M3, E5M2, MXFP8, MXFP4 = 4, 3, 8, 16, 17


def restated(step, mt, mtiles, nsteps, mode):
    """the restatement of tests/test_host_cpu.py::test_k_order_is_a_permutation_of_the_k_steps, with the plain mode in front"""
    if mode < 0 or mtiles < 2:
        return step
    if mode == 0:
        k = step + (mt * nsteps) // mtiles
        return k - nsteps if k >= nsteps else k
    gsh = mode - 1
    g, i = step >> gsh, step & ((1 << gsh) - 1)
    base = (g // mtiles) * mtiles
    if base + mtiles <= (nsteps >> gsh):
        r = g - base + mt
        g = base + (r - mtiles if r >= mtiles else r)
    return (g << gsh) + i


NSTEPS = list(range(1, 41)) + [56, 64, 112, 128]
MTILES = list(range(1, 9)) + [16]


def _orders(lib, mtiles, nsteps, mode):
    return [[lib.gemlite_hip_k_order_step(s, mt, mtiles, nsteps, mode) for s in range(nsteps)] for mt in range(mtiles)]


@pytest.mark.parametrize("mode", list(range(-1, 16)))
def test_library_k_order_step_visits_every_step_once_and_leads_as_documented(mode):
    lib = _hip.load()
    for nsteps in NSTEPS:
        for mtiles in MTILES:
            orders = _orders(lib, mtiles, nsteps, mode)
            tag = (mode, nsteps, mtiles)
            plain = list(range(nsteps))
            for mt, o in enumerate(orders):
                assert sorted(o) == plain, (tag, mt, o)                                        # every step exactly once
                assert o == [restated(s, mt, mtiles, nsteps, mode) for s in plain], (tag, mt)  # ... and what the restatement says
            assert orders[0] == plain, tag                                                     # row tile 0 is never moved
            if mode < 0 or mtiles < 2:
                assert all(o == plain for o in orders), tag
            elif mode == 0:
                for mt, o in enumerate(orders):  # a rotation: consecutive steps, starting at mt nsteps / mtiles
                    assert o[0] == (mt * nsteps) // mtiles and all((o[s + 1] - o[s]) % nsteps == 1 for s in range(nsteps - 1)), (tag, mt)
            else:
                G = 1 << (mode - 1)
                ngroups = nsteps // G
                runs = ngroups // mtiles
                for run in range(runs):  # each tile LEADS a different group of every full run, and walks whole groups
                    first = [orders[mt][run * mtiles * G] // G for mt in range(mtiles)]
                    assert first == [run * mtiles + mt for mt in range(mtiles)], (tag, run, first)
                    for mt, o in enumerate(orders):
                        for j in range(mtiles):
                            seg = o[(run * mtiles + j) * G:(run * mtiles + j + 1) * G]
                            g = run * mtiles + (mt + j) % mtiles
                            assert seg == list(range(g * G, g * G + G)), (tag, run, mt, j, seg)
                # a tail of fewer than mtiles groups, and a partial last group, are plain; so is everything when G > nsteps
                for o in orders:
                    assert o[runs * mtiles * G:] == plain[runs * mtiles * G:], tag
                if G > nsteps:
                    assert all(o == plain for o in orders), tag


def test_library_k_order_step_refuses_arguments_out_of_range():
    lib = _hip.load()
    assert lib.gemlite_hip_k_order_step(0, 0, 1, 1, -1) == 0
    for bad in ((-1, 0, 2, 4, 0), (4, 0, 2, 4, 0), (0, 2, 2, 4, 0), (0, -1, 2, 4, 0), (0, 0, 0, 4, 0), (0, 0, 2, 0, 0), (0, 0, 2, 4, -2), (0, 0, 2, 4, 16)):
        assert lib.gemlite_hip_k_order_step(*bad) == -1, bad


# ---------------------------------------------------------------------------------------------------- the planner's choice
def _a8(M, N, K, dt, tuning=(0, 0, 0, 0)):
    a = _args(M=M, N=N, K=K, nbits=8, e=1, in_dt=dt, w_mode=0, c_mode=3, out_dt=1, tuning=tuning)
    a.scales_x = 0x1000
    return a


def _mx(M, N, K, dt, nbits, tuning=(0, 0, 0, 0)):
    a = _mx_args(M, N, K, dt, nbits, 4)
    for i, t in enumerate(tuning):
        a.tuning[i] = t
    return a


def _a16w8(M, N, K, tuning=(0, 0, 0, 0), w_dtype=INT8):
    return _args(M=M, N=N, K=K, nbits=8, e=1, in_dt=1, w_dtype=w_dtype, w_mode=2, gs=K, tuning=tuning)


SQ64, SQ128 = "gemm_a8w8_sq_kernel<64x64>", "gemm_a8w8_sq_kernel<128x128>"
MX88, MX44 = "gemm_mx_a8w8_sq_kernel<64x64>", "gemm_mx_a4w4_sq_kernel<64x64>"
NARROW = "gemm_a16w8_kernel<64x64>"

PLANNED = [
    # the planner's own choice
    ("int8 4096^2 M=256: whole rotation", lambda: _a8(256, 4096, 4096, INT8), SQ64, 0),
    ("int8 4096 x 14336 M=256: 7 MB of weight tiles per XCD, groups of one step", lambda: _a8(256, 4096, 14336, INT8), SQ64, 1),
    ("int8 4096 x 8192 M=256: 4 MB, groups of one step", lambda: _a8(256, 4096, 8192, INT8, (5, 0, 0, 0)), SQ64, 1),
    ("e4m3 4096^2 M=192", lambda: _a8(192, 4096, 4096, E4M3), SQ64, 0),
    ("fp8 16384^2 M=256 on the 128 x 128 tiles", lambda: _a8(256, 16384, 16384, E4M3), SQ128, 1),
    ("e5m2 16384^2 M=256 on the 128 x 128 tiles", lambda: _a8(256, 16384, 16384, E5M2, (10, 0, 0, 0)), SQ128, 1),
    ("int8 on the 128 x 128 tiles: plain", lambda: _a8(1024, 4096, 4096, INT8), SQ128, -1),
    ("fp8 128 x 128, one row tile", lambda: _a8(128, 16384, 16384, E4M3, (10, 0, 0, 0)), SQ128, -1),
    ("fp8 128 x 128, N / 128 % 8 != 0", lambda: _a8(256, 128 * 12, 4096, E4M3, (10, 0, 0, 0)), SQ128, -1),
    ("N / 64 % 8 != 0", lambda: _a8(256, 768, 4096, INT8, (5, 0, 0, 0)), SQ64, -1),
    ("M <= 64", lambda: _a8(64, 4096, 4096, INT8, (5, 0, 0, 0)), SQ64, -1),
    ("M = 65: two row tiles", lambda: _a8(65, 4096, 4096, INT8), SQ64, 0),
    ("mxfp8 4096^2 M=256", lambda: _mx(256, 4096, 4096, MXFP8, 8), MX88, 0),
    ("mxfp4 4096^2 M=65", lambda: _mx(65, 4096, 4096, MXFP4, 4), MX44, 0),
    ("mxfp4 M=64: one row tile", lambda: _mx(64, 4096, 4096, MXFP4, 4), MX44, -1),
    ("mxfp8 N / 64 % 8 != 0", lambda: _mx(256, 768, 4096, MXFP8, 8, (6, 0, 0, 0)), MX88, -1),
    # GEMLITE_TF_NO_K_ROTATION: plain for every kernel
    ("no rotation, sq64", lambda: _a8(256, 4096, 4096, INT8, (0, 0, 0, NO_K_ROTATION)), SQ64, -1),
    ("no rotation, sq64 grouped shape", lambda: _a8(256, 4096, 14336, INT8, (0, 0, 0, NO_K_ROTATION)), SQ64, -1),
    ("no rotation, sq128", lambda: _a8(256, 16384, 16384, E4M3, (0, 0, 0, NO_K_ROTATION)), SQ128, -1),
    ("no rotation, mx", lambda: _mx(256, 4096, 4096, MXFP8, 8, (0, 0, 0, NO_K_ROTATION)), MX88, -1),
    ("no rotation, narrow", lambda: _a16w8(256, 4096, 4096, (0, 0, 32, NO_K_ROTATION)), NARROW, -1),
    ("no rotation wins over a forced group, sq64", lambda: _a8(256, 4096, 4096, INT8, (5, 0, 0, NO_K_ROTATION | (2 << 24))), SQ64, -1),
    ("no rotation wins over a forced group, mx", lambda: _mx(256, 4096, 4096, MXFP8, 8, (6, 0, 0, NO_K_ROTATION | (2 << 24))), MX88, -1),
    # the two other public switches change the code path, not the order
    ("requests first", lambda: _a8(256, 4096, 4096, INT8, (0, 0, 0, REQUESTS_FIRST)), SQ64, 0),
    ("round-5 epilogue, narrow", lambda: _a16w8(256, 4096, 4096, (0, 0, 32, ROUND5_EPILOGUE)), NARROW, 0),
    # the narrow tiles of the weight-only 8-bit layers: whole rotation by k_rotation_pays(), the group field is ignored
    ("a16w8 4096^2 M=256", lambda: _a16w8(256, 4096, 4096), NARROW, 0),
    ("a16w8 fp8 4096^2 M=256 forced narrow", lambda: _a16w8(256, 4096, 4096, (0, 0, 32, 0), E4M3), NARROW, 0),
    ("a16w8 4096 x 14336: past the L2 rule", lambda: _a16w8(256, 4096, 14336, (0, 0, 32, 0)), NARROW, -1),
    ("a16w8 N / 64 % 8 != 0", lambda: _a16w8(256, 768, 4096, (0, 0, 32, 0)), NARROW, -1),
    ("a16w8 group field ignored", lambda: _a16w8(192, 4096, 4096, (0, 0, 32, 2 << 24)), NARROW, 0),
    ("a16w8 group field ignored where the rotation does not pay", lambda: _a16w8(256, 4096, 14336, (0, 0, 32, 2 << 24)), NARROW, -1),
    # a split K has no order
    ("a16w8 narrow tiles, two K slices", lambda: _a16w8(256, 4096, 4096, (0, 2, 32, 0)), NARROW, -1),
    ("a8w8 K-sliced 128-row tiles", lambda: _a8(512, 4096, 11008, INT8), "gemm_a8w8_lds_kernel<128x128>", -1),
    ("a8w8 forced slices", lambda: _a8(256, 4096, 4096, INT8, (0, 2, 4, 0)), "gemm_a8w8_lds_kernel<128x128>", -1),
    # kernels without an order
    ("packed 4-bit narrow tiles", lambda: _args(M=256), "gemm_w4_mma_kernel<64x64>", -1),
    ("decode", lambda: _args(M=1), "gemv_w4_decode3_kernel<tile16,16w>", -1),
]
# forced groups 1 .. 4 (and the largest field): that group on sq64, sq128 and mx_sq, also under the plain block map (column tiles not a multiple of 8)
for _g in (1, 2, 3, 4, 15):
    _t3 = _g << 24
    PLANNED += [
        (f"forced {_g} sq64", lambda t=_t3: _a8(256, 4096, 4096, INT8, (5, 0, 0, t)), SQ64, _g),
        (f"forced {_g} sq64 plain map", lambda t=_t3: _a8(256, 768, 4096, E4M3, (5, 0, 0, t)), SQ64, _g),
        (f"forced {_g} sq64 one row tile", lambda t=_t3: _a8(64, 4096, 4096, INT8, (5, 0, 0, t)), SQ64, -1),
        (f"forced {_g} sq128 int8", lambda t=_t3: _a8(256, 4096, 4096, INT8, (10, 0, 0, t)), SQ128, _g),
        (f"forced {_g} sq128 plain map", lambda t=_t3: _a8(300, 384, 4096, E5M2, (10, 0, 5, t)), SQ128, _g),
        (f"forced {_g} sq128 one row tile", lambda t=_t3: _a8(128, 4096, 4096, E4M3, (10, 0, 0, t)), SQ128, -1),
        (f"forced {_g} mx88", lambda t=_t3: _mx(256, 4096, 4096, MXFP8, 8, (6, 0, 0, t)), MX88, _g),
        (f"forced {_g} mx44 plain map", lambda t=_t3: _mx(129, 768, 4096, MXFP4, 4, (6, 0, 0, t)), MX44, _g),
    ]


@pytest.mark.parametrize("label,make,kernel,mode", PLANNED, ids=[p[0] for p in PLANNED])
def test_planner_k_order_mode(label, make, kernel, mode):
    lib = _hip.load()
    a = make()
    assert lib.gemlite_hip_query(C.byref(a)) == 0
    assert lib.gemlite_hip_kernel_name(C.byref(a)).decode() == kernel
    assert lib.gemlite_hip_k_order_mode(C.byref(a)) == mode


def test_k_order_mode_of_a_request_without_a_kernel_is_plain():
    lib = _hip.load()
    a = _args(in_dt=12)  # e4m3fnuz: not a gfx950 format
    assert lib.gemlite_hip_k_order_mode(C.byref(a)) == -1
    a = _args()
    a.struct_size += 4
    assert lib.gemlite_hip_k_order_mode(C.byref(a)) == -1


# ---------------------------------------------------------------------------------------------------- the K step of each kernel, read from its source
def kernel_k_steps():
    """k per K step of the four kernels with a K order, parsed from their sources (tests/test_k_order_gpu.py sizes K in these steps)"""
    a8 = open(os.path.join(CSRC, "gemm_a8w8.hip")).read()
    mx = open(os.path.join(CSRC, "gemm_mx.hip")).read()
    wn = open(os.path.join(CSRC, "gemm_wn_mma.hip")).read()
    body64 = a8[a8.index("void gemm_a8w8_sq_kernel("):]
    sq64 = int(re.search(r"constexpr int BM = 64, BN = 64, KSTEP = (\d+)", body64).group(1))
    sq128 = {int(m) for m in re.findall(r"fn = GL_SQ128\((\d+), \d\)", a8)}
    bodymx = mx[mx.index("void gemm_mx_sq_kernel("):]
    mxs = int(re.search(r"constexpr int BM = 64, BN = 64, KSTEP = (\d+)", bodymx).group(1))
    narrow = int(re.search(r"const int units = \(int\)\(a\.K / (\d+)\), splitk = a\.tuning\[2\] == 32", wn).group(1))  # (mma_lookup(6, ...): the narrow form)
    assert len(sq128) == 1
    return {"sq64": sq64, "sq128": sq128.pop(), "mx_sq": mxs, "narrow": narrow}


def test_k_steps_read_from_the_kernels():
    assert kernel_k_steps() == {"sq64": 256, "sq128": 128, "mx_sq": 256, "narrow": 256}
