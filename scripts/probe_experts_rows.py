"""Batches of tokens through the experts: route + forward_batched (slots sorted by expert on the GPU, one MFMA rows launch) against
experts.forward (one M = 1 GEMV per slot), A16W4 g128 fp16, uniformly random ids (top_k distinct experts per token).

    python scripts/probe_experts_rows.py [--runs 3] [--replays 100] [--rows-per-block R]     the driver: starts the workers, prints the table
    python scripts/probe_experts_rows.py --worker                                            one process: a JSON line per (cell, T)

Both paths are measured in the SAME process, each as a captured graph of ONE call (forward: one launch; batched: the route launch and the
rows launch, rows_per_block the library's default, or --rows-per-block for every cell and T).  Timing as scripts/probe_experts.py:
device events around `--replays` replays (fewer where a replay is long) after 20 warm-up replays, three windows per process (their
median is the process's figure); `--runs` processes; the table gives the median over runs and the spread (max - min).  Number 1 of a cell: the smallest T from which, at every measured T
upwards, the batched path is below forward by more than three spreads (the larger of the two paths' spreads); number 2: the ratio
forward / batched at T = 64."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOKENS = (1, 2, 4, 8, 16, 32, 64, 128)
# (label, N, K, top_k, E)
CELLS = [("qwen3-30b-a3b gate/up 768x2048", 768, 2048, 8, 128),
         ("qwen3-30b-a3b down 2048x768", 2048, 768, 8, 128),
         ("mixtral gate/up 14336x4096", 14336, 4096, 2, 8),
         ("mixtral down 4096x14336", 4096, 14336, 2, 8),
         ("4096x4096 top2", 4096, 4096, 2, 16),
         ("4096x4096 top8", 4096, 4096, 8, 16)]


def worker(replays, rows_per_block):
    sys.path.insert(0, ROOT)
    import torch
    from gemlite_amd import DType, GemLiteExperts, GemLiteLinear
    dev, tdt = "cuda:0", torch.float16

    def make_experts(N, K, E):
        g = torch.Generator(device=dev).manual_seed(0)
        one = GemLiteLinear(4, 128, K, N, DType.FP16, DType.FP16).pack(
            torch.randint(0, 16, (N, K), dtype=torch.uint8, device=dev, generator=g),
            (torch.rand(N * K // 128, 1, device=dev, generator=g) * 0.002 + 0.0005).to(tdt),
            (torch.rand(N * K // 128, 1, device=dev, generator=g) * 15).to(tdt))
        ex = GemLiteExperts()
        ex.load_state_dict({
            "W_q": torch.randint(-2 ** 31, 2 ** 31 - 1, (E, K // 8, N), dtype=torch.int32, device=dev, generator=g), "bias": None,
            "scales": (torch.rand(E, K // 128, N, device=dev, generator=g) * 0.002 + 0.0005).to(tdt),
            "zeros": (-(torch.rand(E, K // 128, N, device=dev, generator=g) * 0.02)).to(tdt),
            "metadata": torch.tensor(one.get_meta_args(), dtype=torch.int32), "orig_shape": torch.tensor([N, K], dtype=torch.int32),
            "n_experts": torch.tensor(E, dtype=torch.int32)})
        return ex

    def capture(step):
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
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        return g, keep

    def window(g, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / n  # us per replay

    def time_graph(g):
        n = max(10, min(replays, int(50000.0 / max(window(g, 5), 1.0))))  # a window of about 50 ms at the most
        return statistics.median(window(g, n) for _ in range(3))

    for label, N, K, top_k, E in CELLS:
        ex = make_experts(N, K, E)
        gen = torch.Generator().manual_seed(2)
        for T in TOKENS:
            ids = torch.stack([torch.randperm(E, generator=gen)[:top_k] for _ in range(T)]).to(dev)
            x = (torch.randn(T, K, generator=gen) * 0.5).to(tdt).to(dev)
            g_fwd, y_fwd = capture(lambda: ex(x, ids))
            g_bat, y_bat = capture(lambda: ex.forward_batched(x, ids, ex.route(ids, rows_per_block)))
            torch.cuda.synchronize()
            diff = float((y_fwd.float() - y_bat.float()).abs().max() / y_fwd.float().abs().mean())
            assert diff < 5e-2, (label, T, diff)  # (two roundings of the same sums: the kernels add K in different orders)
            R = ex.rows_per_block(ids.numel(), rows_per_block)
            blocks = int(ex.route(ids, rows_per_block).workspace[0])
            t_fwd, t_bat = time_graph(g_fwd), time_graph(g_bat)
            print(json.dumps({"cell": label, "T": T, "forward_us": t_fwd, "batched_us": t_bat, "rows_per_block": R, "blocks": blocks,
                              "experts_hit": int(ids.unique().numel()), "max_diff_over_mean": diff}), flush=True)
            del g_fwd, g_bat, y_fwd, y_bat
        del ex
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=100)
    ap.add_argument("--rows-per-block", type=int, default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays, a.rows_per_block)
    rows, info = {}, {}
    for run in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays)] +
                           (["--rows-per-block", str(a.rows_per_block)] if a.rows_per_block else []), stdout=subprocess.PIPE,
                           text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"worker failed with {p.returncode}")
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                rows.setdefault((r["cell"], r["T"]), []).append((r["forward_us"], r["batched_us"]))
                info[(r["cell"], r["T"])] = r
    print(f"probe_experts_rows: rows_per_block {a.rows_per_block or 'default'}; {a.runs} runs (processes), up to {a.replays} replays per window; us per call: median over runs (spread = max - min)")
    for label, N, K, top_k, E in CELLS:
        print(f"\n{label}   top_k {top_k}, {E} experts")
        print("    T  slots  experts hit   R  blocks    forward us (spread)    route + batched us (spread)   forward / batched   batched ahead by > 3 spreads")
        ahead = {}
        for T in TOKENS:
            vals, i = rows[(label, T)], info[(label, T)]
            f, b = [v[0] for v in vals], [v[1] for v in vals]
            fm, bm, fs, bs = statistics.median(f), statistics.median(b), max(f) - min(f), max(b) - min(b)
            ahead[T] = fm - bm > 3 * max(fs, bs)
            print(f"  {T:3d}  {T * top_k:5d}  {i['experts_hit']:11d}  {i['rows_per_block']:2d}  {i['blocks']:6d}   {fm:10.2f} ({fs:6.2f})      {bm:14.2f} ({bs:6.2f})"
                  f"            {fm / bm:8.3f}          {'yes' if ahead[T] else 'no'}")
        first = next((T for k, T in enumerate(TOKENS) if all(ahead[t] for t in TOKENS[k:])), None)
        vals = rows[(label, 64)]
        ratio = statistics.median(v[0] for v in vals) / statistics.median(v[1] for v in vals)
        print(f"  number 1: {'no T wins' if first is None else f'from T = {first}'}    number 2: forward / batched at T = 64 = {ratio:.2f}")


if __name__ == "__main__":
    main()
