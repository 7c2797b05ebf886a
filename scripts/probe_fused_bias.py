"""What the bias inside the launch buys (A16W4 g128 4096 x 4096, graph-replayed over rotating HBM-cold layers like the benchmark headline).

    python scripts/probe_fused_bias.py [--runs 5] [--layers 64] [--replays 20]

A/B in ONE process through core.FUSE_BIAS, alternating (unfused, fused) `--runs` times; the unfused side is the two-launch path the
library had before (its kernels are unchanged).  Per dtype it prints, in us per layer:
  (a) a dependent chain of biased layers at M = 1           (b) `--layers` independent biased layers on one x at M = 1, and the same
  layers without a bias (the grouped launch the bias should cost nothing in)          (c) M = 16 and M = 64, biased, independent
Each figure is the median over `--replays` replays of one captured graph of `--layers` layers (576 MB of weights: HBM-cold per replay)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemlite_amd  # noqa: E402
from gemlite_amd import GemLiteLinear, core  # noqa: E402

DEV = "cuda:0"
N = K = 4096


def make_layers(n, tdt, bias):
    g = torch.Generator().manual_seed(0)
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    out = []
    for i in range(n):
        lin = GemLiteLinear(4, 128, K, N, code, code)
        W_q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8).to(DEV)
        s = (torch.rand(N * K // 128, 1, generator=g) * 0.002 + 0.0005).to(tdt).to(DEV)
        z = (torch.rand(N * K // 128, 1, generator=g) * 15).to(tdt).to(DEV)
        b = (torch.randn(N, generator=g) * 0.1).to(tdt).to(DEV) if bias else None
        lin.pack(W_q, s, z, b, fma_mode=True)
        out.append(lin)
    return out


def time_graph(step, replays):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        keep = step()
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    ts = []
    for _ in range(replays):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    del keep
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--layers", type=int, default=64)
    ap.add_argument("--replays", type=int, default=20)
    a = ap.parse_args()
    L = a.layers
    print(f"probe_fused_bias: {torch.cuda.get_device_properties(0).name} | gemlite_amd {gemlite_amd.__version__} | {L} layers {N}x{K} g128 | "
          f"{a.runs} alternating runs, median of {a.replays} replays each | us per layer")
    for tdt in (torch.float16, torch.bfloat16):
        biased, plain = make_layers(L, tdt, True), make_layers(L, tdt, False)
        xs = {M: (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) / 10).to(tdt).to(DEV) for M in (1, 16, 64)}

        def chain():
            y = xs[1]
            for lin in biased:
                y = lin(y)
            return y

        cases = [("(a) chain M=1 biased", chain, True),
                 ("(b) independent M=1 biased", lambda: [lin(xs[1]) for lin in biased], True),
                 ("(b) independent M=1 NO bias", lambda: [lin(xs[1]) for lin in plain], False),
                 ("(c) independent M=16 biased", lambda: [lin(xs[16]) for lin in biased], True),
                 ("(c) independent M=64 biased", lambda: [lin(xs[64]) for lin in biased], True)]
        for label, step, ab in cases:
            res = {False: [], True: []}
            for _ in range(a.runs):
                for fuse in ((False, True) if ab else (True,)):
                    core.FUSE_BIAS = fuse
                    res[fuse].append(time_graph(step, a.replays) / L)
            core.FUSE_BIAS = True
            line = f"{str(tdt).split('.')[-1]:9s} {label:30s}"
            for fuse in ((False, True) if ab else (True,)):
                v = sorted(res[fuse])
                line += f" | {'fused  ' if fuse else 'unfused'} median {statistics.median(v):6.3f} best {v[0]:6.3f} worst {v[-1]:6.3f}"
            print(line, flush=True)
        del biased, plain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
