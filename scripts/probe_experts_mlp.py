"""What the expert MLP of one MoE layer costs for one token in two fused launches against the unfused path (A16W4 g128 fp16).

    python scripts/probe_experts_mlp.py [--runs 3] [--replays 200]      the driver: starts the workers, prints the table
    python scripts/probe_experts_mlp.py --worker                        one process: a JSON line per (cell, variant)

Variants per cell (us per MoE layer, one token), each in a captured graph of its own:
  a   GemLiteExpertsMLP(x, ids, w): gate/up + GLU, down + combine — two launches
  b   y = gate_up(x, ids); h = silu(y[..., :I]) * y[..., I:]; z = down(h, ids); out = (z * w.unsqueeze(-1)).sum(-2) — GemLiteExperts.forward
      and torch ops, what runs without the fused forms
  c   gate_up.forward_glu(x, ids) alone            cu  gate_up(x, ids) + silu * mul          cr  gate_up(x, ids) alone, the raw launch
  d   down.forward_combine(h, ids, w) alone        du  down(h, ids) + the weighted sum       dr  down(h, ids) alone, the raw launch
A graph holds `steps` layers, step i on the experts (i * top_k + j) % E, with one tiny elementwise kernel between two steps in every variant;
a graph of the separators alone is subtracted.  Timing as scripts/probe_experts.py: device events around `--replays` replays after 20
warm-up replays of every graph of the cell, three windows per process (their median is the process's figure), `--runs` processes; the
table gives the median over runs and the spread (max - min).  Every cell first checks the fused output against the unfused one."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# (label, hidden H, intermediate I, top_k, E)
CELLS = [("qwen3-30b-a3b H2048 I768 top8 E128", 2048, 768, 8, 128),
         ("mixtral H4096 I14336 top2 E8", 4096, 14336, 2, 8),
         ("H4096 I4096 top2 E16", 4096, 4096, 2, 16),
         ("H4096 I4096 top4 E16", 4096, 4096, 4, 16),
         ("H4096 I4096 top8 E16", 4096, 4096, 8, 16)]
VARIANTS = ("a", "b", "c", "cu", "cr", "d", "du", "dr")


def worker(replays):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
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

    def time_graph(g):
        windows = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) * 1000.0 / replays)  # us per replay
        return statistics.median(windows)

    for label, H, I, top_k, E in CELLS:
        gate_up, down = make_experts(2 * I, H, E, 1), make_experts(H, I, E, 2)
        mlp = GemLiteExpertsMLP(gate_up, down)
        steps = max(1, min(E // top_k, 16))
        ids = [torch.tensor([[(i * top_k + j) % E for j in range(top_k)]], dtype=torch.int64, device=dev) for i in range(steps)]
        gen = torch.Generator().manual_seed(1)
        x = (torch.randn(1, H, generator=gen) * 0.5).to(tdt).to(dev)
        w = torch.softmax(torch.randn(1, top_k, generator=gen), -1).to(tdt).to(dev)
        h0 = gate_up.forward_glu(x, ids[0])
        sep = torch.zeros(64, device=dev)

        def unfused_glu(i):
            y = gate_up(x, ids[i])
            return F.silu(y[..., :I]) * y[..., I:]

        def unfused_combine(h, i):
            return (down(h, ids[i]) * w.unsqueeze(-1)).sum(-2)

        def stepper(fn):
            def step():
                out = []
                for i in range(steps):
                    out.append(fn(i))
                    sep.add_(1.0)
                return out
            return step

        fns = {"a": lambda i: mlp(x, ids[i], w), "b": lambda i: unfused_combine(unfused_glu(i), i),
               "c": lambda i: gate_up.forward_glu(x, ids[i]), "cu": unfused_glu,
               "cr": lambda i: gate_up(x, ids[i]),
               "d": lambda i: down.forward_combine(h0, ids[i], w), "du": lambda i: unfused_combine(h0, i), "dr": lambda i: down(h0, ids[i]),
               "sep": lambda i: None}
        graphs = {v: capture(stepper(fn)) for v, fn in fns.items()}
        torch.cuda.synchronize()
        ya, yb = graphs["a"][1], graphs["b"][1]
        err = max(float((ya[i].float() - yb[i].float()).abs().max()) for i in range(steps))
        ref = max(float(yb[i].float().abs().max()) for i in range(steps))
        assert err <= 2e-2 * ref + 1e-3, (label, err, ref)
        t_sep = time_graph(graphs["sep"][0])
        for v in VARIANTS:
            t = time_graph(graphs[v][0])
            print(json.dumps({"cell": label, "variant": v, "us_per_layer": (t - t_sep) / steps, "sep_us": t_sep / steps, "steps": steps,
                              "max_abs_diff_a_b": err, "max_abs_b": ref}), flush=True)
        del graphs, mlp, gate_up, down


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays)
    rows, info = {}, {}
    for run in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays)], stdout=subprocess.PIPE,
                           text=True, timeout=600)
        if p.returncode != 0:
            sys.exit(f"worker failed with {p.returncode}")
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                rows.setdefault((r["cell"], r["variant"]), []).append(r["us_per_layer"])
                info[r["cell"]] = r
    print(f"probe_experts_mlp: {a.runs} runs, {a.replays} replays per window; us per MoE layer, one token: median over runs (spread = max - min)")
    for label, *_ in CELLS:
        i = info[label]
        print(f"\n{label}   steps/graph {i['steps']}   separator {i['sep_us']:.2f} us/step   "
              f"max |a - b| {i['max_abs_diff_a_b']:.3e} at max |b| {i['max_abs_b']:.3e}")
        med = {}
        for v in VARIANTS:
            vals = rows[(label, v)]
            med[v] = (statistics.median(vals), max(vals) - min(vals))
            print(f"  variant {v:>2}: {med[v][0]:8.3f} us/layer   spread {med[v][1]:.3f}   runs {' '.join(f'{t:.3f}' for t in vals)}")
        for fused, unfused, what in (("a", "b", "the MLP"), ("c", "cu", "gate/up + GLU"), ("d", "du", "down + combine")):
            gap, spread = med[unfused][0] - med[fused][0], max(med[fused][1], med[unfused][1])
            print(f"  {what}: {unfused} - {fused} = {gap:+.3f} us (larger spread {spread:.3f}): "
                  f"{'fused is ahead by more than the spread' if gap > spread else 'fused is NOT ahead by more than the spread'}")


if __name__ == "__main__":
    main()
