"""Child process of tests/test_decode_group_tiles_gpu.py: GEMLITE_HIP_CAPTURE_GROUP_TILES is read once per process, so every forced
(TB, placement) runs in a process of its own.  usage: python -m tests.decode_group_tiles_child <scenario>; prints one "RESULT <json>" line per
group of the scenario.  Every group goes through the C ABI with its outputs as adjacent rows of ONE allocation between 0xFF guard bytes,
is captured, replayed twice and compared torch.equal with the eager layer on the same inputs."""
import ctypes as C
import json
import sys

import numpy as np
import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from oracle import gemlite_oracle as O
from tests.test_capture_groups_gpu import DEV, _capture, _replay

F16, B16 = "fp16", "bf16"
TDT = {F16: torch.float16, B16: torch.bfloat16}
KERNEL = "gemv_w4_decode3_kernel<"
GUARD = 512

# scenario -> groups: (N, K, members, dtype, group size, zeros kind, biased, index of the member with an x of its own or None)
SCENARIOS = {
    # 64 tiles on 256 CUs: grid.y > 1 under every TB, blocks that hold different numbers of layers
    "n1024": [(1024, 4096, 7, F16, 128, "tensor", False, None), (1024, 4096, 16, F16, 128, "tensor", False, None)],
    # 256 tiles: one round of blocks; 16 slots of one wave each under TB = 1, 2 and 4 (the benchmark's launch), and a bf16 group of five
    "n4096": [(4096, 4096, 16, F16, 128, "tensor", False, None), (4096, 4096, 5, B16, 128, "tensor", False, None)],
    # 70 tiles (2 divides, 4 does not: TB = 4 falls back to 2) and 67 tiles (odd: TB = 1 whatever is asked); 67 groups: span = identity
    "widths": [(1120, 4096, 3, F16, 128, "tensor", False, None), (1072, 4096, 5, F16, 128, "tensor", False, None),
               (1120, 512, 16, B16, 128, "tensor", True, None)],
    # K = 256: one chunk, most virtual waves empty; 4352: a remainder chunk; 16640 on a shared x: the second staging trip
    "ks": [(1024, 256, 3, F16, 128, "tensor", False, None), (4096, 256, 16, F16, 128, "tensor", False, None),
           (1024, 4352, 5, F16, 128, "tensor", False, None), (4096, 16640, 3, F16, 128, "tensor", False, None)],
    # the forms: two members (form 1), a member with its own x (form 1), biased on a shared x and on its own x, a scalar zero point, groups of 64
    "forms": [(1024, 512, 2, F16, 128, "tensor", False, None), (1024, 768, 7, F16, 128, "tensor", False, 3),
              (1024, 768, 7, B16, 128, "tensor", True, None), (4096, 512, 5, F16, 128, "tensor", True, 1),
              (1024, 768, 5, B16, 128, "int", False, None), (1024, 4096, 5, F16, 64, "tensor", False, None)],
}


def layer(N, K, tdt, gs, zeros_kind, biased, seed, zero_point):
    W_q, scales, zeros = O.gen_data(N, K, 4, gs, seed=seed, np_float=np.float16)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lin = GemLiteLinear(4, gs, K, N, code, code)
    z = zero_point if zeros_kind == "int" else torch.from_numpy(zeros.astype(np.float32)).to(tdt).to(DEV)
    b = (torch.randn(N, generator=torch.Generator().manual_seed(seed)) * 0.5).to(tdt).to(DEV) if biased else None
    lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(scales.astype(np.float32)).to(tdt).to(DEV), z, b, fma_mode=True)
    return lin


def run_group(idx, spec):
    N, K, members, dt, gs, zeros_kind, biased, own = spec
    tdt = TDT[dt]
    lib = _hip.load()
    lins = [layer(N, K, tdt, gs, zeros_kind, biased, 4000 + 100 * idx + i, 3 + 2 * (i % 6)) for i in range(members)]
    x = torch.from_numpy(O.gen_x(1, K, seed=77 + idx)).to(tdt).to(DEV)
    x_own = torch.from_numpy(O.gen_x(1, K, seed=177 + idx)).to(tdt).to(DEV)
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
    form = lib.gemlite_hip_capture_group_last_form()
    geo = (C.c_int32 * 4)()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert lib.gemlite_hip_capture_group_geometry(N // 16, members, cus, 0, 0, C.byref(geo)) == 0
    buf.view(torch.uint8).fill_(0xFF)
    _replay(g, 2)
    raw = buf.view(torch.int16)
    guards = bool((raw[:GUARD] == -1).all()) and bool((raw[GUARD + members * N:] == -1).all())
    equal = [bool(torch.equal(buf[GUARD + i * N: GUARD + (i + 1) * N].view(1, N), w)) for i, w in enumerate(want)]
    print("RESULT " + json.dumps({"group": idx, "spec": list(spec), "kernels": sorted(names), "seen": seen, "joined": joined, "form": form,
                                  "geometry": list(geo), "cus": cus, "guards": guards, "equal": equal}), flush=True)


if __name__ == "__main__":
    for idx, spec in enumerate(SCENARIOS[sys.argv[1]]):
        run_group(idx, spec)
