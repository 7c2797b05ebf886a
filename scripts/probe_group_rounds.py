"""Steps in which a merged grouped decode node leaves a tail.  (A16W4 g128 4096 x 4096, M = 1, fp16, every layer distinct, one x.)

    python scripts/probe_group_rounds.py [--layers 32,33,40,48,64] [--replays 200] [--runs 2]

One captured step of n independent layers per n; ms per step, the median over `--replays` replays timed in blocks of ten, `--runs` times.
The member limit and the round limit come from the environment (GEMLITE_HIP_CAPTURE_GROUP_MAX, GEMLITE_HIP_CAPTURE_GROUP_ROUNDS: read once
per process), and the other side of a comparison is this script run from a build of the parent commit, every run its own process,
alternating.  Prints one JSON line per n: {"layers", "ms": [...], "us_per_layer": [...], "joined", "merged" (null: a library without
rounds), "group_max", "rounds_max"}."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemlite_amd  # noqa: E402
from gemlite_amd import GemLiteLinear, _hip  # noqa: E402

DEV = "cuda:0"
N = K = 4096


def make_layers(n):
    g = torch.Generator(device=DEV).manual_seed(0)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[torch.float16]
    out = []
    for _ in range(n):
        lin = GemLiteLinear(4, 128, K, N, code, code)
        W_q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.int32, device=DEV).to(torch.uint8)
        s = (torch.rand(N * K // 128, 1, generator=g, device=DEV) * 0.01 + 0.001).half()
        z = (torch.rand(N * K // 128, 1, generator=g, device=DEV) * 15).half()
        lin.pack(W_q, s, z, None)
        out.append(lin)
    return out


def counters(lib):
    seen, joined, merged = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
    if not hasattr(lib, "gemlite_hip_capture_group_merge_stats"):
        return joined.value, None
    lib.gemlite_hip_capture_group_merge_stats.argtypes = [C.POINTER(C.c_uint64)]
    lib.gemlite_hip_capture_group_merge_stats(C.byref(merged))
    return joined.value, merged.value


def capture(lins, x):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    step = lambda: [lin(x) for lin in lins]  # noqa: E731
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        keep = step()
    return g, keep


def ms_per_step(g, replays):
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(1, replays // 10)):
        t0 = time.perf_counter()
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / 10 * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", default="32,33,40,48,64")
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--runs", type=int, default=2)
    args = ap.parse_args()
    sizes = [int(v) for v in args.layers.split(",")]
    lib = _hip.load()
    lins = make_layers(max(sizes))
    x = (torch.randn(1, K, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) / 10).half()
    want = [lin(x).clone() for lin in lins]
    rounds_max = lib.gemlite_hip_capture_group_rounds_max() if hasattr(lib, "gemlite_hip_capture_group_rounds_max") else None
    for n in sizes:
        j0, m0 = counters(lib)
        g, keep = capture(lins[:n], x)
        j1, m1 = counters(lib)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(keep, want)), "a captured layer differs from its eager output"
        ms = [ms_per_step(g, args.replays) for _ in range(args.runs)]
        print(json.dumps({"layers": n, "ms": [round(v, 5) for v in ms], "us_per_layer": [round(v * 1e3 / n, 4) for v in ms], "joined": j1 - j0,
                          "merged": None if m1 is None else m1 - m0, "group_max": lib.gemlite_hip_capture_group_max(),
                          "rounds_max": rounds_max}), flush=True)
        del g, keep
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
