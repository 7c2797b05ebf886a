"""Child process of tests/test_decode_group_policy_gpu.py: GEMLITE_HIP_CAPTURE_GROUP_TILES, _LINES and _NT are read once per process, so
every forced (TB, H, policy) runs in a process of its own.  usage: python -m tests.decode_group_policy_child <scenario>; prints one
"RESULT <json>" line per group of the scenario.  Every group goes through the C ABI with its outputs as adjacent rows of ONE allocation
between 0xFF guard bytes, is captured, replayed twice and compared torch.equal with the eager layer on the same inputs.  After every call
of the captured step the child notes gemlite_hip_capture_group_last_form / _last_lines / _last_policy: what the node that call joined
(or opened) looks like at that moment."""
import ctypes as C
import json
import sys

import torch

import gemlite_amd
from gemlite_amd import _hip, core
from tests.decode_group_lines_child import layer_any
from tests.decode_group_tiles_child import B16, F16, GUARD, TDT
from tests.test_capture_groups_gpu import DEV, _capture, _replay

KERNEL = "gemv_w4_decode3_kernel<"
FLAG = 32  # GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS (tuning[3])
# (N, K, members, dtype, group size, zeros kind, biased, index of the member with an x of its own or None, byte offset of every member's
#  weights in their storage, per member: does its tuning carry FLAG)
# N = 64: four tiles, one TB = 4 tile group; N = 512: 32 tiles, several blocks.  K = 256: one chunk (most waves idle); 4352: 17 chunks
# (virtual wave 0 holds two).  2 members: the per-wave-x form; 5 and 16 with one x: the shared-x form
SHAPES = [
    (64, 256, 2, F16, 128, "tensor", False, None, 0, None),
    (64, 4352, 5, B16, 64, "tensor", True, None, 0, None),
    (512, 4096, 16, F16, 512, "tensor", False, None, 0, None),  # (a group of 512 over K = 512 would be channel-wise: another kernel)
    (512, 4096, 5, F16, 128, "tensor", False, 2, 0, None),
    (512, 4352, 16, B16, 128, "int", True, 3, 0, None),     # a scalar zero point, biased, member 3 on an x of its own
    (512, 512, 5, B16, 128, "tensor", False, None, 0, None),
]
POLICY = [
    (512, 512, 5, F16, 128, "tensor", False, None, 64, None),              # every member's weights start 64 bytes into a line
    (512, 512, 5, F16, 128, "tensor", False, None, 0, [1] * 5),            # the members' own launches are default-policy
    (512, 512, 9, F16, 128, "tensor", False, None, 0, [1, 1, 1, 0, 0, 0, 1, 1, 1]),  # flag / no flag / flag: three nodes
    (512, 512, 5, B16, 128, "tensor", True, 1, 128, None),                 # 128 bytes in: still whole lines
]
GROUPS = {"shapes": SHAPES, "policy": POLICY}


def offset_view(t, off_bytes):
    """The same values, starting off_bytes into a fresh storage"""
    if not off_bytes:
        return t
    assert off_bytes % t.element_size() == 0 and t.is_contiguous()
    pad = off_bytes // t.element_size()
    store = torch.empty(t.numel() + pad, dtype=t.dtype, device=t.device)
    v = store[pad:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 128 == off_bytes % 128
    return v


def run_group(idx, spec):
    N, K, members, dt, gs, zeros_kind, biased, own, w_off, flags = spec
    tdt = TDT[dt]
    lib = _hip.load()
    lins = [layer_any(N, K, tdt, gs, zeros_kind, biased, 8000 + 100 * idx + i, 3 + 2 * (i % 6)) for i in range(members)]
    x = torch.randn(1, K, generator=torch.Generator().manual_seed(55 + idx)).mul(0.5).to(tdt).to(DEV)
    x_own = torch.randn(1, K, generator=torch.Generator().manual_seed(155 + idx)).mul(0.5).to(tdt).to(DEV)
    xs = [x_own if i == own else x for i in range(members)]
    core.FUSE_BIAS = False  # the eager reference of a biased layer: the matmul launch, then torch's add
    want = [lin(xi).clone() for lin, xi in zip(lins, xs)]
    core.FUSE_BIAS = True
    torch.cuda.synchronize()
    buf = torch.empty(GUARD + members * N + GUARD, dtype=tdt, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    calls, names, keep = [], set(), []
    for i, (lin, xi) in enumerate(zip(lins, xs)):
        W_q, scales, zeros = lin.get_tensor_args()
        W_q = offset_view(W_q, w_off)
        keep.append(W_q)
        tuning = (0, 0, 0, FLAG) if flags and flags[i] else None
        a = core._call_args(xi, W_q, scales, zeros, None, lin.get_meta_args(), -1, tuning, False, buf[GUARD + i * N:].data_ptr(), (N, 1))
        ext = _hip.forward_ext(lin.bias.data_ptr(), gemlite_amd.dtypes.TORCH_TO_DTYPE[lin.bias.dtype].value) if biased else None
        names.add((lib.gemlite_hip_kernel_name_ex(C.byref(a), C.byref(ext)) if biased else lib.gemlite_hip_kernel_name(C.byref(a))).decode())
        calls.append((a, ext))
    trail = []

    def step():
        st = _hip.current_stream_handle(x.device)
        del trail[:]
        for a, ext in calls:
            rc = lib.gemlite_hip_forward_ex(C.byref(a), C.byref(ext), st) if ext is not None else lib.gemlite_hip_forward(C.byref(a), st)
            assert rc == 0, rc
            trail.append([lib.gemlite_hip_capture_group_last_form(), lib.gemlite_hip_capture_group_last_lines(),
                          lib.gemlite_hip_capture_group_last_policy()])

    g, _, seen, joined = _capture(step)
    under_capture = [list(t) for t in trail]
    geo = (C.c_int32 * 4)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    buf.view(torch.uint8).fill_(0xFF)
    _replay(g, 2)
    raw = buf.view(torch.int16)
    guards = bool((raw[:GUARD] == -1).all()) and bool((raw[GUARD + members * N:] == -1).all())
    equal = [bool(torch.equal(buf[GUARD + i * N: GUARD + (i + 1) * N].view(1, N), w)) for i, w in enumerate(want)]
    print("RESULT " + json.dumps({"group": idx, "spec": list(spec), "kernels": sorted(names), "seen": seen, "joined": joined, "trail": under_capture,
                                  "w_mod_128": sorted({int(w.data_ptr() % 128) for w in keep}), "cus": cus, "guards": guards, "equal": equal}),
          flush=True)


if __name__ == "__main__":
    for idx, spec in enumerate(GROUPS[sys.argv[1]]):
        run_group(idx, spec)
