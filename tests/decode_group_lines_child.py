"""Child process of tests/test_decode_group_lines_gpu.py: GEMLITE_HIP_CAPTURE_GROUP_TILES and GEMLITE_HIP_CAPTURE_GROUP_LINES are read once per
process, so every forced (TB, H) runs in a process of its own.  usage: python -m tests.decode_group_lines_child <scenario>; prints one
"RESULT <json>" line per group of the scenario.  The scenarios are those of tests/decode_group_tiles_child.py (of "n4096" only the 16-member
fp16 group) and "lines": the smallest shapes at which what depends on the PASS of a wave can go wrong.  Every group goes through the C ABI
with its outputs as adjacent rows of ONE allocation between 0xFF guard bytes, is captured, replayed twice and compared torch.equal with
the eager layer on the same inputs."""
import ctypes as C
import json
import sys

import numpy as np
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from oracle import gemlite_oracle as O
from tests.decode_group_tiles_child import B16, F16, GUARD, KERNEL, SCENARIOS, TDT, layer
from tests.test_capture_groups_gpu import DEV, _capture, _replay

# (N, K, members, dtype, group size, zeros kind, biased, index of the member with an x of its own or None), as in the tiles child;
# zeros kind "none": scales only (W_group_mode 2: the kernel requests no zeros)
LINES = [
    (64, 512, 4, F16, 128, "tensor", False, None),    # four tiles: ONE run of tiles under H = 4, one block per member
    (128, 768, 3, B16, 128, "tensor", True, None),    # eight tiles, three chunks (virtual waves 3 .. 15 write zeros in every pass), biased
    # groups of 32, 256 and 512: log2(group) below, at and above 8 — the metadata row changes inside a pass (32), between the passes of
    # a chunk (64 / 128 in the other scenarios), between chunks (256) and every second chunk (512).  (A single group over all of K is
    # channel-wise metadata, which the planner gives to gemv_w4_decode_kernel: 512 is the largest group that reaches this kernel here.)
    (1024, 1024, 5, F16, 32, "tensor", False, None),
    (1024, 1024, 5, F16, 256, "tensor", False, 2),    # (member 2 on an x of its own: the per-wave-x form, whose x offset moves with the pass)
    (1024, 1024, 5, F16, 512, "tensor", False, None),
    (1024, 1024, 5, F16, 128, "none", False, None),   # no zeros: their requests go to the weight buffer's first bytes
]
GROUPS = dict(SCENARIOS, n4096=SCENARIOS["n4096"][:1], lines=LINES)


def layer_any(N, K, tdt, gs, zeros_kind, biased, seed, zero_point):
    if zeros_kind != "none":
        return layer(N, K, tdt, gs, zeros_kind, biased, seed, zero_point)
    W_q, scales, _ = O.gen_data(N, K, 4, gs, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, gs, K, N, code, code)
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV), None, None, fma_mode=True)
    return lin


def run_group(idx, spec):
    N, K, members, dt, gs, zeros_kind, biased, own = spec
    tdt = TDT[dt]
    lib = _hip.load()
    lins = [layer_any(N, K, tdt, gs, zeros_kind, biased, 6000 + 100 * idx + i, 3 + 2 * (i % 6)) for i in range(members)]
    x = torch.from_numpy(O.gen_x(1, K, seed=91 + idx)).to(tdt).to(DEV)
    x_own = torch.from_numpy(O.gen_x(1, K, seed=191 + idx)).to(tdt).to(DEV)
    xs = [x_own if i == own else x for i in range(members)]
    core.FUSE_BIAS = False  # the eager reference of a biased layer: the matmul launch, then torch's add
    want = [lin(xi).clone() for lin, xi in zip(lins, xs)]
    core.FUSE_BIAS = True
    torch.cuda.synchronize()
    buf = torch.empty(GUARD + members * N + GUARD, dtype=tdt, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    calls, names = [], set()
    for i, (lin, xi) in enumerate(zip(lins, xs)):
        W_q, scales, zeros = lin.get_tensor_args()
        a = core._call_args(xi, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, buf[GUARD + i * N:].data_ptr(), (N, 1))
        ext = _hip.forward_ext(lin.bias.data_ptr(), gemlite_amd.dtypes.TORCH_TO_DTYPE[lin.bias.dtype].value) if biased else None
        names.add((lib.gemlite_hip_kernel_name_ex(C.byref(a), C.byref(ext)) if biased else lib.gemlite_hip_kernel_name(C.byref(a))).decode())
        calls.append((a, ext))

    def step():
        st = _hip.current_stream_handle(x.device)
        for a, ext in calls:
            rc = lib.gemlite_hip_forward_ex(C.byref(a), C.byref(ext), st) if ext is not None else lib.gemlite_hip_forward(C.byref(a), st)
            assert rc == 0, rc

    g, _, seen, joined = _capture(step)
    form, last_lines = lib.gemlite_hip_capture_group_last_form(), lib.gemlite_hip_capture_group_last_lines()
    geo = (C.c_int32 * 4)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.gemlite_hip_capture_group_geometry(N // 16, members, cus, 0, 0, C.byref(geo)) == 0
    lines = lib.gemlite_hip_capture_group_lines(N // 16, members, cus, geo[0], 0)
    buf.view(torch.uint8).fill_(0xFF)
    _replay(g, 2)
    raw = buf.view(torch.int16)
    guards = bool((raw[:GUARD] == -1).all()) and bool((raw[GUARD + members * N:] == -1).all())
    equal = [bool(torch.equal(buf[GUARD + i * N: GUARD + (i + 1) * N].view(1, N), w)) for i, w in enumerate(want)]
    print("RESULT " + json.dumps({"group": idx, "spec": list(spec), "kernels": sorted(names), "seen": seen, "joined": joined, "form": form,
                                  "geometry": list(geo), "lines": lines, "last_lines": last_lines, "cus": cus, "guards": guards,
                                  "equal": equal}), flush=True)


if __name__ == "__main__":
    for idx, spec in enumerate(GROUPS[sys.argv[1]]):
        run_group(idx, spec)
