"""Capture-time grouping of the M = 1 decode kernel, host side (no GPU): gemlite_hip_capture_group_compatible applies the join rule of
gemlite_amd/csrc/capture_group.hip — same kernel / shape / strides / modes, and no output overlapping the other launch's inputs or
output — to two hand-built argument structs.  Nothing is dereferenced, so the addresses are made up."""
import ctypes as C

import pytest

from gemlite_amd import _hip

N = K = 4096
GS = 128
W_BYTES = (K // 8) * N * 4
META_BYTES = (K // GS) * N * 2
# launch A's buffers, far apart; launch B's default buffers sit 64 GiB above them
X_A, W_A, S_A, Z_A, OUT_A = 0x1000000000, 0x1100000000, 0x1200000000, 0x1300000000, 0x1400000000
SHIFT_B = 0x1000000000


def _args(x=X_A, w=W_A, s=S_A, z=Z_A, out=OUT_A, n=N, k=K, gs=GS, dt=1, w_mode=4, stride_wk=None):
    a = _hip.ForwardArgs()
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = -1
    a.x, a.w_q, a.scales, a.zeros, a.out = x, w, s, z, out
    a.M, a.N, a.K = 1, n, k
    a.W_nbits, a.group_size, a.unpack_mask, a.elements_per_sample = 4, gs, 15, 8
    a.w_pack_bits, a.w_dtype = 32, 6
    a.input_dtype = a.output_dtype = a.meta_dtype = a.zeros_dtype = dt
    a.channel_scale_mode, a.W_group_mode = 0, w_mode
    a.stride_xm, a.stride_xk = k, 1
    a.stride_wk, a.stride_wn = (n if stride_wk is None else stride_wk), 1
    a.stride_om, a.stride_on = n, 1
    a.stride_meta_g, a.stride_meta_n = n, 1
    return a


def _b(**kw):
    for name, base in (("x", X_A), ("w", W_A), ("s", S_A), ("z", Z_A), ("out", OUT_A)):
        kw.setdefault(name, base + SHIFT_B)
    return _args(**kw)


def _ok(a, b):
    lib = _hip.load()
    ab = lib.gemlite_hip_capture_group_compatible(C.byref(a), C.byref(b))
    assert ab == lib.gemlite_hip_capture_group_compatible(C.byref(b), C.byref(a)), "the rule is symmetric"
    return ab == 1


def test_both_launches_run_the_decode_kernel():
    lib = _hip.load()
    for a in (_args(), _b(), _args(dt=2)):
        assert lib.gemlite_hip_kernel_name(C.byref(a)) == b"gemv_w4_decode3_kernel<tile16,16w>"


def test_group_limit_and_counters_without_a_gpu():
    lib = _hip.load()
    assert 2 <= lib.gemlite_hip_capture_group_max() <= 16
    seen, joined = C.c_uint64(1), C.c_uint64(2)
    lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    assert joined.value <= seen.value  # (both 0 unless this process has captured decode launches)
    before = (seen.value, joined.value)
    _ok(_args(), _b())  # the host-only rule counts nothing
    lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    assert (seen.value, joined.value) == before
    lib.gemlite_hip_capture_group_stats(None, None)  # either pointer may be NULL


def test_disjoint_buffers_join():
    assert _ok(_args(), _b())
    assert _ok(_args(), _b(x=X_A))                       # the benchmark step: one x, distinct weights and outputs
    assert _ok(_args(), _b(x=X_A, w=W_A, s=S_A, z=Z_A))  # shared inputs are reads on both sides


def test_a_dependent_launch_does_not_join():
    assert not _ok(_args(), _b(x=OUT_A))                      # lin2(lin1(x))
    assert not _ok(_args(x=OUT_A + SHIFT_B), _b())            # ... in the other order
    assert not _ok(_args(), _b(x=OUT_A - 2 * K + 2))          # the LAST element of x_B is the first of out_A
    assert _ok(_args(), _b(x=OUT_A - 2 * K))                  # x_B ends where out_A begins
    assert not _ok(_args(), _b(x=OUT_A + 2 * N - 2))          # the first element of x_B is the last of out_A
    assert _ok(_args(), _b(x=OUT_A + 2 * N))


def test_overlapping_outputs_do_not_join():
    assert not _ok(_args(), _b(out=OUT_A))                    # a reused allocator block
    assert not _ok(_args(), _b(out=OUT_A + 2 * (N - 1)))      # one element in common
    assert not _ok(_args(), _b(out=OUT_A - 2 * (N - 1)))
    assert _ok(_args(), _b(out=OUT_A + 2 * N))                # back to back
    assert _ok(_args(), _b(out=OUT_A - 2 * N))


def test_an_output_inside_the_other_launchs_inputs_does_not_join():
    assert not _ok(_args(), _b(out=W_A + W_BYTES // 2))       # inside A's W_q
    assert not _ok(_args(), _b(out=W_A + W_BYTES - 2))        # its last two bytes
    assert _ok(_args(), _b(out=W_A + W_BYTES))
    assert not _ok(_args(), _b(out=W_A - 2 * N + 2))
    assert not _ok(_args(), _b(out=S_A + META_BYTES - 2))     # A's scales
    assert _ok(_args(), _b(out=S_A + META_BYTES))
    assert not _ok(_args(), _b(out=Z_A + META_BYTES - 2))     # A's zeros
    assert _ok(_args(), _b(out=Z_A + META_BYTES))
    assert not _ok(_args(), _b(out=X_A + 2 * K - 2))          # A's x


def test_strided_and_offset_views_are_ranged_to_their_last_element():
    # W_q as every other row of a [2 K/8, N] buffer: the last row starts at (K/8 - 1) * 2N words
    wide = _args(stride_wk=2 * N)
    end = ((K // 8 - 1) * 2 * N + N) * 4
    assert end > W_BYTES
    assert _ok(wide, _b(stride_wk=2 * N))
    assert not _ok(wide, _b(stride_wk=2 * N, out=W_A + end - 2))
    assert _ok(wide, _b(stride_wk=2 * N, out=W_A + end))
    # an offset view: A's x starts 1000 elements into its buffer; B writes just below / onto its first element
    off = _args(x=X_A + 2000)
    assert _ok(off, _b(out=X_A + 2000 - 2 * N))
    assert not _ok(off, _b(out=X_A + 2000 - 2 * N + 2))


@pytest.mark.parametrize("kw", [dict(w_mode=3), dict(k=11008), dict(gs=64), dict(dt=2), dict(stride_wk=2 * N)],
                         ids=["modes", "shape", "group_size", "dtype", "weight_stride"])
def test_differing_modes_shape_or_dtype_do_not_join(kw):
    assert _ok(_args(**kw), _b(**kw)), "the pair joins when both sides agree"
    assert not _ok(_args(), _b(**kw))


def test_launches_of_other_kernels_do_not_join():
    lib = _hip.load()
    a, b = _args(), _b()
    a.M = b.M = 2  # the rows kernel
    assert lib.gemlite_hip_query(C.byref(a)) == 0
    assert not _ok(a, b)
    a, b = _args(), _b()
    a.tuning[3] = b.tuning[3] = 4  # GEMLITE_TF_TIMELINE: a probed launch is always its own
    assert not _ok(a, b)
    assert lib.gemlite_hip_capture_group_compatible(None, C.byref(b)) == 0
