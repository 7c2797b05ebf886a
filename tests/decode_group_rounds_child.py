"""Child process of tests/test_decode_group_rounds_gpu.py: GEMLITE_HIP_CAPTURE_GROUP_MAX and GEMLITE_HIP_CAPTURE_GROUP_ROUNDS are read once per
process, so every case runs in a process of its own (the parent sets CASES[name]["env"]).  usage: python -m tests.decode_group_rounds_child
<case>; prints one "RESULT <json>" line.  The layers of a case go through the C ABI with their outputs as adjacent rows of ONE allocation
between guard elements, are captured as one step, replayed three times and compared torch.equal with the eager layer on the same inputs.
After every call of the captured step the child notes gemlite_hip_capture_group_last_form / _last_lines / _last_policy / _last_rounds: what
the node that call joined, opened or merged looks like at that moment.

With a member limit L of 2 or 3 a node fills after two or three launches, so merges happen with 4 to 13 small layers.  N = 256 (16 tiles) and
N = 272 (17: no tile group but TB = 1) at K = 4096 are the smallest shapes the planner gives gemv_w4_decode3_kernel; K = 4352 is 17
chunks, wave 0 holds two."""
import ctypes as C
import json
import sys

import torch

import gemlite_amd
from gemlite_amd import GemLiteLinear, _hip, core
from tests.decode_group_policy_child import offset_view
from tests.decode_group_tiles_child import B16, F16, GUARD, KERNEL, TDT, layer
from tests.test_capture_groups_gpu import DEV, _capture, _replay

SWITCH = "GEMLITE_HIP_CAPTURE_GROUP_ROUNDS"


def _case(L, n, N=256, K=4096, dt=F16, biased=False, kind="plain", env=None, gs=128):
    e = {"GEMLITE_HIP_CAPTURE_GROUP_MAX": str(L)} if L != 16 else {}
    e.update(env or {})
    return {"L": L, "n": n, "N": N, "K": K, "dt": dt, "biased": biased, "kind": kind, "env": e, "gs": gs}


# kind: what is special about the step (run() has the details).  n: layers of the step
CASES = {
    # 4 L + 1 independent layers on one x: four full groups become one node of four rounds, the last launch stays alone
    "basic-fp16": _case(2, 9),
    "basic-fp16-bias": _case(3, 13, N=272, biased=True),
    "basic-bf16": _case(3, 13, N=272, dt=B16),
    "basic-bf16-bias": _case(2, 9, K=4352, dt=B16, biased=True),
    # the last group is partial (one launch; two launches: a grouped node of its own behind the merged one)
    "partial-1": _case(2, 5),
    "partial-2": _case(3, 8, N=272),
    # five full groups: the node stops absorbing at four rounds, and the fifth group has no predecessor to merge with
    "limit": _case(2, 10),
    # the second group reads another x: the merged node takes the per-wave-x form (L = 3: both groups alone take the shared-x form)
    "different-x": _case(3, 6, kind="different-x"),
    # one member of the second group starts 64 bytes into a 128-byte line (whole lines forced: TB = 2, H = 2, so the first group is non-temporal)
    "unaligned": _case(2, 4, kind="unaligned", env={"GEMLITE_HIP_CAPTURE_GROUP_TILES": "2i", "GEMLITE_HIP_CAPTURE_GROUP_LINES": "2"}),
    # launch L + 1 reads an output of the first group as (part of) its x
    "dependent": _case(2, 4, kind="dependent"),
    # a torch elementwise kernel on the capturing stream between launch L and launch L + 1
    "foreign": _case(2, 4, kind="foreign"),
    # another stream forks from the capture behind launch L + 1 and joins back at the end of the step
    "fork": _case(2, 4, kind="fork"),
    # replays after x was overwritten in place
    "new-x": _case(2, 5, kind="new-x"),
    # merging switched off: the joins of the parent, no merge
    "off": _case(2, 9, env={SWITCH: "1"}),
    "two-rounds": _case(2, 9, env={SWITCH: "2"}),
    # the benchmark's layers at the real limit: 16 + 16 + 1
    "headline": _case(16, 33, N=4096, kind="headline"),
}


def big_layers(n, N, K):
    """(generated on the GPU: the host generator takes seconds at this size)"""
    g = torch.Generator(device=DEV).manual_seed(25)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[torch.float16]
    out = []
    for _ in range(n):
        lin = GemLiteLinear(4, 128, K, N, code, code)
        W_q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        s = (torch.rand(N * K // 128, 1, generator=g, device=DEV) * 0.01 + 0.001).half()
        z = (torch.rand(N * K // 128, 1, generator=g, device=DEV) * 15).half()
        out.append(lin.pack(W_q, s, z, None, fma_mode=True))
    return out


def run(name):
    c = CASES[name]
    L, n, N, K, kind, biased = c["L"], c["n"], c["N"], c["K"], c["kind"], c["biased"]
    tdt = TDT[c["dt"]]
    lib = _hip.load()
    assert lib.gemlite_hip_capture_group_max() == L, (lib.gemlite_hip_capture_group_max(), L)
    lins = big_layers(n, N, K) if kind == "headline" else [layer(N, K, tdt, c["gs"], "tensor", biased, 9000 + i, 0) for i in range(n)]
    gen = torch.Generator().manual_seed(251)
    x, x2, x_new = ((torch.randn(1, K, generator=gen) * 0.5).to(tdt).to(DEV) for _ in range(3))
    # [front: K finite elements the dependent case reads as x][n outputs of N][GUARD elements of 0xFF]
    front = (torch.randn(K, generator=gen) * 0.5).to(tdt).to(DEV)
    buf = torch.empty(K + n * N + GUARD, dtype=tdt, device=DEV)
    buf.view(torch.uint8).fill_(0xFF)
    buf[:K].copy_(front)
    outs = [buf[K + i * N: K + (i + 1) * N] for i in range(n)]
    xs = [x] * n
    if kind == "different-x":
        xs = [x if i < L else x2 for i in range(n)]
    if kind == "dependent":
        assert n * N <= K
        xs[L] = buf[N: N + K].view(1, K)  # the end of the front, then output 0 (and whatever of the next outputs fits): launch L + 1 reads it
        assert xs[L].data_ptr() + 2 * K > outs[0].data_ptr()

    def eager():
        """every layer on its own, in order, into the buffer (the dependent case reads what the launches before it wrote)"""
        core.FUSE_BIAS = False  # the eager reference of a biased layer: the matmul launch, then torch's add
        want = []
        for lin, xi, o in zip(lins, xs, outs):
            y = lin(xi).clone()
            o.copy_(y.view(-1))
            want.append(y)
        core.FUSE_BIAS = True
        torch.cuda.synchronize()
        return want

    want = eager()
    calls, names, keep = [], set(), []
    for i, (lin, xi, o) in enumerate(zip(lins, xs, outs)):
        W_q, scales, zeros = lin.get_tensor_args()
        if kind == "unaligned" and i == L + 1:
            W_q = offset_view(W_q, 64)
        keep.append(W_q)
        a = core._call_args(xi, W_q, scales, zeros, None, lin.get_meta_args(), -1, None, False, o.data_ptr(), (N, 1))
        ext = _hip.forward_ext(lin.bias.data_ptr(), gemlite_amd.dtypes.TORCH_TO_DTYPE[lin.bias.dtype].value) if biased else None
        names.add((lib.gemlite_hip_kernel_name_ex(C.byref(a), C.byref(ext)) if biased else lib.gemlite_hip_kernel_name(C.byref(a))).decode())
        calls.append((a, ext))
    assert all(k.startswith(KERNEL) for k in names), names  # first: the case is about this kernel
    side = torch.cuda.Stream()
    scratch = torch.zeros(64, device=DEV)
    trail = []

    def step():
        cur = torch.cuda.current_stream()
        st = _hip.current_stream_handle(x.device)
        del trail[:]
        forked = False
        for i, (a, ext) in enumerate(calls):
            if kind == "foreign" and i == L:
                scratch.add_(1.0)
            rc = lib.gemlite_hip_forward_ex(C.byref(a), C.byref(ext), st) if ext is not None else lib.gemlite_hip_forward(C.byref(a), st)
            assert rc == 0, rc
            trail.append([lib.gemlite_hip_capture_group_last_form(), lib.gemlite_hip_capture_group_last_lines(),
                          lib.gemlite_hip_capture_group_last_policy(), lib.gemlite_hip_capture_group_last_rounds()])
            if kind == "fork" and i == L:
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    scratch.add_(1.0)
                forked = True
        if forked:
            cur.wait_stream(side)

    merged0 = C.c_uint64(0)
    lib.gemlite_hip_capture_group_merge_stats(C.byref(merged0))
    g, _, seen, joined = _capture(step)
    merged1 = C.c_uint64(0)
    lib.gemlite_hip_capture_group_merge_stats(C.byref(merged1))
    under_capture = [list(t) for t in trail]
    for o in outs:
        o.view(torch.uint8).fill_(0xFF)
    scratch.zero_()
    _replay(g, 3)
    if kind == "new-x":
        x.copy_(x_new)
        for o in outs:
            o.view(torch.uint8).fill_(0xFF)
        want_new = eager()
        assert not torch.equal(want[0], want_new[0])
        want = want_new
        for o in outs:
            o.view(torch.uint8).fill_(0xFF)
        _replay(g, 3)
    guards = bool(torch.equal(buf[:K], front)) and bool((buf[K + n * N:].view(torch.int16) == -1).all())
    equal = [bool(torch.equal(o.view(1, N), w)) for o, w in zip(outs, want)]
    print("RESULT " + json.dumps({"case": name, "kernels": sorted(names), "seen": seen, "joined": joined, "merged": merged1.value - merged0.value,
                                  "trail": under_capture, "rounds_max": lib.gemlite_hip_capture_group_rounds_max(), "guards": guards,
                                  "equal": equal, "scratch": float(scratch[0]), "w_mod_128": sorted({int(w.data_ptr() % 128) for w in keep})}),
          flush=True)


if __name__ == "__main__":
    run(sys.argv[1])
