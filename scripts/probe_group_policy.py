"""At which rotation size do non-temporal weight requests stop paying in a grouped decode launch?  (A16W4 g128 4096 x 4096, M = 1, fp16.)

    python scripts/probe_group_policy.py [--runs 3] [--replays 200] [--layers 64,32,16,8]

The headline step over 64, 32, 16 and 8 distinct layers (572, 286, 143 and 71 MB of rotating weights), captured as a graph that always holds
64 launches (the step repeated 64 / layers times), under both weight-load policies in ONE process: the policy of a group follows its
members' own launches (gl_common.h: decode3_group_nt), so the default-policy side is the same layers called with
GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS in tuning[3] (core.TUNING_OVERRIDE while that graph is captured).  The two graphs of a size alternate
`--runs` times; each figure is us per layer, the median over `--replays` replays timed in blocks of ten.  Prints one JSON line per size:
{"layers", "MB", "nt_us": [...], "default_us": [...], "policy": [nt, default] as gemlite_hip_capture_group_last_policy() reported them}."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemlite_amd  # noqa: E402
from gemlite_amd import GemLiteLinear, _hip, core  # noqa: E402

DEV = "cuda:0"
N = K = 4096
LAUNCHES = 64
FLAG = 32  # GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS


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


def capture(lins, x, reps, flagged):
    core.TUNING_OVERRIDE = (0, 0, 0, FLAG) if flagged else None
    try:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        step = lambda: [lin(x) for _ in range(reps) for lin in lins]  # noqa: E731
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            keep = step()
        return g, keep, _hip.load().gemlite_hip_capture_group_last_policy()
    finally:
        core.TUNING_OVERRIDE = None


def us_per_layer(g, replays):
    for _ in range(10):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(1, replays // 10)):
        t0 = time.perf_counter()
        for _ in range(10):
            g.replay()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / (10 * LAUNCHES) * 1e6)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--layers", default="64,32,16,8")
    args = ap.parse_args()
    sizes = [int(v) for v in args.layers.split(",")]
    lins = make_layers(max(sizes))
    x = (torch.randn(1, K, generator=torch.Generator(device=DEV).manual_seed(1), device=DEV) / 10).half()
    for n in sizes:
        reps = max(1, LAUNCHES // n)
        g_nt, keep_nt, p_nt = capture(lins[:n], x, reps, False)
        g_df, keep_df, p_df = capture(lins[:n], x, reps, True)
        g_nt.replay()
        g_df.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(keep_nt, keep_df)), "the two policies must give the same bits"
        nt, df = [], []
        for _ in range(args.runs):
            nt.append(round(us_per_layer(g_nt, args.replays) * LAUNCHES / (n * reps), 4))
            df.append(round(us_per_layer(g_df, args.replays) * LAUNCHES / (n * reps), 4))
        print(json.dumps({"layers": n, "MB": round(n * 8.93), "nt_us": nt, "default_us": df, "policy": [p_nt, p_df]}), flush=True)
        del g_nt, g_df, keep_nt, keep_df
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
