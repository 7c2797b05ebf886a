"""The batched expert MLP in four launches — route, gate/up with SwiGLU inside, down, combine (GemLiteExpertsMLP.forward_batched_fused) —
against forward_batched (route, two rows launches and the torch ops between and behind them), A16W4 g128 fp16, uniformly random ids
(top_k distinct experts per token).

    python scripts/probe_experts_rows_fused.py [--runs 3] [--replays 100]     the driver: starts the workers, prints the table
    python scripts/probe_experts_rows_fused.py --worker                       one process: a JSON line per (cell, T)

Both paths are measured in the SAME process, each as a captured graph of ONE call, their windows ALTERNATING (unfused, fused, unfused,
...).  Timing as scripts/probe_experts_rows.py: device events around `--replays` replays (fewer where a replay is long) after 20 warm-up
replays, three windows per path and process (their median is the process's figure); `--runs` processes; the table gives the median over
runs and the spread (max - min).  A cell counts as a win or a loss only where the medians differ by more than three spreads (the larger
of the two paths' spreads); otherwise it is a tie.  The outputs at the timed sizes are compared in the same run with the checks of
tests/test_experts_rows_fused_gpu.py: on one routing the GLU launch lies within one ulp of silu(gate) * up of the unfused launch and the
combine launch equals the fp32 loop bit for bit, and the fused call lies within the DESIGN §4 gate of forward_batched."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TOKENS = (8, 32, 64, 256)
# (label, hidden, intermediate, top_k, E)
CELLS = [("qwen3-30b-a3b 2048 / 768", 2048, 768, 8, 128),
         ("mixtral 4096 / 14336", 4096, 14336, 2, 8),
         ("4096 / 4096 top2", 4096, 4096, 2, 16),
         ("4096 / 4096 top8", 4096, 4096, 8, 16)]


def worker(replays):
    sys.path.insert(0, ROOT)
    import torch
    from gemlite_amd import DType, GemLiteExperts, GemLiteExpertsMLP, GemLiteLinear
    dev, tdt = "cuda:0", torch.float16

    def make_experts(N, K, E, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
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

    def time_pair(ga, gb):
        """Three windows per graph, alternating a, b, a, b, a, b -> the two medians."""
        na = max(10, min(replays, int(50000.0 / max(window(ga, 5), 1.0))))  # a window of about 50 ms at the most
        nb = max(10, min(replays, int(50000.0 / max(window(gb, 5), 1.0))))
        a, b = [], []
        for _ in range(3):
            a.append(window(ga, na))
            b.append(window(gb, nb))
        return statistics.median(a), statistics.median(b)

    for label, hidden, inter, top_k, E in CELLS:
        mlp = GemLiteExpertsMLP(make_experts(2 * inter, hidden, E, 0), make_experts(hidden, inter, E, 1))
        gen = torch.Generator().manual_seed(2)
        for T in TOKENS:
            ids = torch.stack([torch.randperm(E, generator=gen)[:top_k] for _ in range(T)]).to(dev)
            w = torch.softmax(torch.randn(T, top_k, generator=gen), -1).to(dev)
            x = (torch.randn(T, hidden, generator=gen) * 0.5).to(tdt).to(dev)
            g_un, y_un = capture(lambda: mlp.forward_batched(x, ids, w))
            g_fu, y_fu = capture(lambda: mlp.forward_batched_fused(x, ids, w))
            torch.cuda.synchronize()
            # the checks of the tests, the three new calls on ONE routing (the bits of a slot depend on the row the route gives it, DESIGN
            # §3.2.2): GLU within one ulp of silu(gate) * up of the unfused launch, the combine bit for bit the fp32 loop, and the fused
            # call within the §4 gate of forward_batched
            R = mlp.rows_per_block_fused(ids.numel())
            routing = mlp.gate_up.route(ids, R)
            h = mlp.gate_up.forward_batched_glu(x, ids, routing)
            y = mlp.gate_up.forward_batched(x, ids, routing).double()
            g64, u64 = y[..., :inter], y[..., inter:]
            glu_ref = g64 / (1.0 + torch.exp(-g64)) * u64
            ulp = torch.exp2(torch.floor(torch.log2(glu_ref.abs().clamp_min(2.0 ** -14))) - 10)
            glu_ulp = float(((h.double() - glu_ref).abs() / ulp).max())
            assert glu_ulp <= 1.0, (label, T, glu_ulp)
            d = mlp.down.forward_batched(h, ids, routing)
            acc = torch.zeros(T, hidden, dtype=torch.float32, device=dev)
            for k in range(top_k):
                acc = acc + w[:, k, None] * d[:, k].float()
            assert torch.equal(mlp.down.combine_batched(d, ids, w), acc.to(tdt)), (label, T)
            ref = y_un.double()
            err, scale, tol = (y_fu.double() - ref).abs(), float(ref.abs().mean()), 1e-3
            rel = float(err.mean()) / scale
            assert rel < tol and bool((err <= 10 * tol * scale + 4 * tol * ref.abs()).all()), (label, T, rel, float(err.max()))
            t_un, t_fu = time_pair(g_un, g_fu)
            print(json.dumps({"cell": label, "T": T, "unfused_us": t_un, "fused_us": t_fu, "rows_per_block": R,
                              "rows_per_block_unfused": mlp.rows_per_block(ids.numel()), "blocks": int(routing.workspace[0]),
                              "experts_hit": int(ids.unique().numel()), "rel_err": rel, "glu_ulp": glu_ulp}), flush=True)
            del g_un, g_fu, y_un, y_fu
        del mlp
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=100)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays)
    rows, info = {}, {}
    for run in range(a.runs):
        p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays)], stdout=subprocess.PIPE, text=True)
        for line in p.stdout:  # (progress on stderr, line by line: a run takes minutes)
            if line.startswith("{"):
                r = json.loads(line)
                rows.setdefault((r["cell"], r["T"]), []).append((r["unfused_us"], r["fused_us"]))
                info[(r["cell"], r["T"])] = r
                print(f"run {run}: {r['cell']} T = {r['T']}: {r['unfused_us']:.1f} / {r['fused_us']:.1f} us", file=sys.stderr, flush=True)
        if p.wait(timeout=900) != 0:
            sys.exit(f"worker failed with {p.returncode}")
    print(f"probe_experts_rows_fused: {a.runs} runs (processes), up to {a.replays} replays per window, windows alternating; "
          "us per call: median over runs (spread = max - min); outputs compared in every run (GLU within 1 ulp, combine bit for bit, the gate of forward_batched)")
    for label, hidden, inter, top_k, E in CELLS:
        print(f"\n{label}   top_k {top_k}, {E} experts")
        print("    T  slots  experts hit   R  blocks   forward_batched us (spread)   forward_batched_fused us (spread)   unfused / fused   beyond 3 spreads")
        for T in TOKENS:
            vals, i = rows[(label, T)], info[(label, T)]
            u, f = [v[0] for v in vals], [v[1] for v in vals]
            um, fm, us, fs = statistics.median(u), statistics.median(f), max(u) - min(u), max(f) - min(f)
            verdict = "win" if um - fm > 3 * max(us, fs) else ("loss" if fm - um > 3 * max(us, fs) else "tie")
            print(f"  {T:3d}  {T * top_k:5d}  {i['experts_hit']:11d}  {i['rows_per_block']:2d}  {i['blocks']:6d}   {um:16.2f} ({us:6.2f})      {fm:20.2f} ({fs:6.2f})"
                  f"          {um / fm:8.3f}   {verdict}")


if __name__ == "__main__":
    main()
