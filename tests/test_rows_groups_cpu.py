"""Capture-time grouping of the few-row rows kernel (gemm_w4_rows_kernel, 2 .. 64 rows), host side (no GPU):
gemlite_hip_capture_group_compatible[_ex] applies the join rule of gemlite_amd/csrc/capture_group.hip to two hand-built argument structs —
the same kernel function, tiles, strides, modes and M, one row block, and no output overlapping the other launch's inputs or output.
Nothing is dereferenced, so the addresses are made up."""
import ctypes as C

import pytest

from gemlite_amd import _hip

# launch A's buffers, far apart; launch B's default buffers sit 64 GiB above them
X_A, W_A, S_A, Z_A, OUT_A, BIAS_A = 0x1000000000, 0x1100000000, 0x1200000000, 0x1300000000, 0x1400000000, 0x1500000000
SHIFT_B = 0x1000000000
ROWS = b"gemm_w4_rows_kernel<"


def _args(M, n=4096, k=4096, gs=128, dt=1, w_mode=4, t0=0, x=X_A, w=W_A, s=S_A, z=Z_A, out=OUT_A, stride_wk=None, stride_xm=None,
          stride_om=None):
    a = _hip.ForwardArgs()
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = -1
    a.x, a.w_q, a.scales, a.zeros, a.out = x, w, s, z, out
    a.M, a.N, a.K = M, n, k
    a.W_nbits, a.group_size, a.unpack_mask, a.elements_per_sample = 4, gs, 15, 8
    a.w_pack_bits, a.w_dtype = 32, 6
    a.input_dtype = a.output_dtype = a.meta_dtype = a.zeros_dtype = dt
    a.channel_scale_mode, a.W_group_mode = 0, w_mode
    a.stride_xm, a.stride_xk = (k if stride_xm is None else stride_xm), 1
    a.stride_wk, a.stride_wn = (n if stride_wk is None else stride_wk), 1
    a.stride_om, a.stride_on = (n if stride_om is None else stride_om), 1
    a.stride_meta_g, a.stride_meta_n = n, 1
    a.tuning[0] = t0
    return a


def _b(M, **kw):
    for name, base in (("x", X_A), ("w", W_A), ("s", S_A), ("z", Z_A), ("out", OUT_A)):
        kw.setdefault(name, base + SHIFT_B)
    return _args(M, **kw)


def _name(a):
    return _hip.load().gemlite_hip_kernel_name(C.byref(a))


def _ok(a, b):
    lib = _hip.load()
    ab = lib.gemlite_hip_capture_group_compatible(C.byref(a), C.byref(b))
    assert ab == lib.gemlite_hip_capture_group_compatible(C.byref(b), C.byref(a)), "the rule is symmetric"
    return ab == 1


def _rows_pair(M, **kw):
    """(a, b): the same launch on disjoint buffers, both planned onto the rows kernel"""
    a, b = _args(M, **kw), _b(M, **kw)
    assert _name(a).startswith(ROWS) and _name(b).startswith(ROWS), (_name(a), _name(b))
    return a, b


@pytest.mark.parametrize("M,kw", [(8, dict()), (16, dict(n=1024)), (2, dict(n=272, k=512, t0=9))], ids=["4096x4096_M8", "1024x4096_M16", "272x512_M2_forced"])
def test_independent_rows_launches_join(M, kw):
    """The test that fails without the feature: before it no rows launch joined anything."""
    a, b = _rows_pair(M, **kw)
    assert _ok(a, b)
    assert _ok(a, _b(M, x=X_A, **kw))                       # one x, distinct weights and outputs
    assert _ok(a, _b(M, x=X_A, w=W_A, s=S_A, z=Z_A, **kw))  # shared inputs are reads on both sides


def test_an_output_inside_the_other_launchs_buffers_does_not_join():
    """The overlap cases of the M = 1 file on an M = 16 pair: x and out are 16 rows now."""
    M, N, K = 16, 1024, 4096
    kw = dict(n=N)
    a, _ = _rows_pair(M, **kw)
    w_bytes, meta_bytes, x_bytes, out_bytes = (K // 8) * N * 4, (K // 128) * N * 2, M * K * 2, M * N * 2
    for base, size in ((X_A, x_bytes), (W_A, w_bytes), (S_A, meta_bytes), (Z_A, meta_bytes), (OUT_A, out_bytes)):
        assert not _ok(a, _b(M, out=base + size - 2, **kw)), hex(base)   # B's first output element is A's last element
        assert _ok(a, _b(M, out=base + size, **kw)), hex(base)           # just past it
        assert not _ok(a, _b(M, out=base - out_bytes + 2, **kw)), hex(base)  # B's last output element is A's first element
        assert _ok(a, _b(M, out=base - out_bytes, **kw)), hex(base)
    assert not _ok(a, _b(M, out=X_A + (M - 1) * K * 2, **kw))     # inside the LAST of the 16 rows of x
    assert not _ok(a, _b(M, x=OUT_A, **kw))                       # lin2(lin1(x))
    assert not _ok(a, _b(M, x=OUT_A + out_bytes - 2, **kw))       # x_B begins on the last element of out_A
    assert _ok(a, _b(M, x=OUT_A + out_bytes, **kw))


@pytest.mark.parametrize("ka,kb", [
    (dict(M=8), dict(M=16)),
    (dict(M=16), dict(M=17)),
    (dict(M=16, n=1024), dict(M=16, n=2048)),
    (dict(M=16, n=1024, k=4096), dict(M=16, n=1024, k=2048)),
    (dict(M=16, gs=128), dict(M=16, gs=64)),
    (dict(M=16, dt=1), dict(M=16, dt=2)),
    (dict(M=16, w_mode=4), dict(M=16, w_mode=3)),
    (dict(M=16, n=1024), dict(M=16, n=1024, stride_wk=2048)),
    (dict(M=16), dict(M=16, stride_xm=8192)),
    (dict(M=16), dict(M=16, stride_om=8192)),
], ids=["M_8_16_same_function", "M_16_17", "N", "K", "group_size", "dtype", "W_group_mode", "stride_wk", "stride_xm", "stride_om"])
def test_rows_launches_that_differ_in_one_property_do_not_join(ka, kb):
    a, a2 = _rows_pair(**ka)
    b2, b = _rows_pair(**kb)
    assert _ok(a, a2) and _ok(b2, b), "each side joins its own kind"
    assert not _ok(a, b)


def test_m_8_and_16_run_the_same_function():
    assert _name(_args(8)) == _name(_args(16)) == b"gemm_w4_rows_kernel<16x16>"


def test_biased_and_unbiased_rows_launches_do_not_join():
    lib = _hip.load()
    a, b = _rows_pair(16, n=1024)
    ea, eb = _hip.forward_ext(BIAS_A, 1), _hip.forward_ext(BIAS_A + SHIFT_B, 1)
    assert lib.gemlite_hip_bias_fused(C.byref(a), C.byref(ea)) == 1
    assert lib.gemlite_hip_kernel_name_ex(C.byref(a), C.byref(ea)).startswith(ROWS)

    def ok_ex(a, ea, b, eb):
        r = lib.gemlite_hip_capture_group_compatible_ex(C.byref(a), ea, C.byref(b), eb)
        assert r == lib.gemlite_hip_capture_group_compatible_ex(C.byref(b), eb, C.byref(a), ea)
        return r == 1

    assert ok_ex(a, C.byref(ea), b, C.byref(eb))      # biased with biased
    assert ok_ex(a, None, b, None)                    # unbiased with unbiased
    assert not ok_ex(a, C.byref(ea), b, None)         # the kernel functions differ
    # a bias is one more input: B's output on A's bias
    assert not ok_ex(a, C.byref(ea), _b(16, n=1024, out=BIAS_A + 2 * 1024 - 2), C.byref(eb))
    assert ok_ex(a, C.byref(ea), _b(16, n=1024, out=BIAS_A + 2 * 1024), C.byref(eb))


def test_a_rows_launch_and_a_decode_launch_of_one_layer_do_not_join():
    a, b = _args(8), _b(1)
    assert _name(a).startswith(ROWS) and _name(b).startswith(b"gemv_w4_decode3_kernel<")
    assert not _ok(a, b)
    assert _ok(_args(1), b) and _ok(a, _b(8)), "each family joins its own"


@pytest.mark.parametrize("M,kw", [(80, dict(n=1024, t0=9)), (33, dict(n=1024, gs=32, t0=9))], ids=["M80", "g32_M33"])
def test_launches_with_row_blocks_never_group(M, kw):
    """More than 16 MT rows: the single-layer kernel runs row blocks along grid.y, the grouped form has none."""
    a, b = _rows_pair(M, **kw)
    assert not _ok(a, b)
    fits = 64 if kw.get("gs", 128) != 32 else 32
    a1, b1 = _rows_pair(fits, **kw)
    assert _ok(a1, b1), "the same layer with one row block joins"


def test_the_host_only_rule_counts_nothing():
    lib = _hip.load()
    seen, joined = C.c_uint64(0), C.c_uint64(0)
    lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    before = (seen.value, joined.value)
    a, b = _rows_pair(16, n=1024)
    assert _ok(a, b)
    lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    assert (seen.value, joined.value) == before
