"""What the MXFP4 experts launch (gemv_mxw4_experts_kernel) costs against the per-expert route it replaces; one token.

    python scripts/probe_experts_mx.py [--runs 3] [--replays 200]      the driver: starts the workers, prints the table
    python scripts/probe_experts_mx.py --worker                        one process: a JSON line per (cell, dtype, variant)

Variants per cell and dtype (us per slot = per expert GEMV), the method of scripts/probe_experts.py:
  1    experts(x, ids) on MXFP4 stacks: ONE launch, the ids a device tensor
  2    top_k captured layer(x) calls on experts chosen ON THE HOST, the same A16W4_MXFP layers (ex.expert(e)): the only route before
  3    the INT4 g128 experts launch on the same shape: a yardstick of bytes moved, not a target
  w4 / w8 / w16   variant 1 with the block size forced (Qwen down and Mixtral gate/up; "glu w*": the GLU launch of the Mixtral gate/up pair)
  mlp  GemLiteExpertsMLP.forward on MXFP4 stacks (GLU launch, down launch, combine launch), us per token
  mlp-chain   the same MLP as forward + torch SwiGLU + forward + torch combine, us per token
A captured graph holds `steps` steps, step i on the experts (i * top_k + j) % E, with one tiny elementwise kernel between two steps in
every variant; its own graph is timed and subtracted.  Timing: device events around `--replays` replays after 20 warm-up replays of
every graph of the cell, three windows per process (their median is the process's figure); `--runs` processes; the table gives the
median over the processes and the spread (max - min)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# (label, N, K, top_k, E, force the block sizes)
CELLS = [("qwen3-30b-a3b gate/up 768x2048", 768, 2048, 8, 128, True),
         ("qwen3-30b-a3b down 2048x768", 2048, 768, 8, 128, True),
         ("mixtral gate/up 14336x4096", 14336, 4096, 2, 8, True),
         ("mixtral down 4096x14336", 4096, 14336, 2, 8, True),
         ("4096x4096 top2", 4096, 4096, 2, 16, True),
         ("4096x4096 top4", 4096, 4096, 4, 16, True),
         ("4096x4096 top8", 4096, 4096, 8, 16, True)]
# (label, hidden, intermediate, top_k, E)
MLPS = [("qwen3-30b-a3b mlp", 2048, 768, 8, 128), ("mixtral mlp", 4096, 14336, 2, 8)]


def worker(replays):
    sys.path.insert(0, ROOT)
    import torch
    from gemlite_amd import DType, GemLiteExperts, GemLiteExpertsMLP, GemLiteLinear, experts as X, helper
    dev = "cuda:0"

    def mx_experts(N, K, E, tdt, seed=0):
        """Random codes and scale bytes (2^-9 .. 2^-1) in the layout from_layers gives: [E, K/2, N] and [E, N, K/32] views."""
        g = torch.Generator(device=dev).manual_seed(seed)
        one = helper.A16W4_MXFP(device=dev, dtype=tdt).from_weights(torch.zeros(16, 256, dtype=torch.uint8), torch.full((16, 8), 127, dtype=torch.uint8))
        ex = GemLiteExperts()
        ex.load_state_dict({
            "W_q": torch.randint(0, 256, (E, N, K // 2), dtype=torch.uint8, device=dev, generator=g).transpose(1, 2), "bias": None,
            "scales": torch.randint(118, 127, (E, K // 32, N), dtype=torch.uint8, device=dev, generator=g).transpose(1, 2),
            "zeros": one.zeros.data, "metadata": torch.tensor(one.get_meta_args(), dtype=torch.int32),
            "orig_shape": torch.tensor([N, K], dtype=torch.int32), "n_experts": torch.tensor(E, dtype=torch.int32)})
        return ex

    def int_experts(N, K, E, tdt):
        g = torch.Generator(device=dev).manual_seed(0)
        dt = DType.FP16 if tdt == torch.float16 else DType.BF16
        one = GemLiteLinear(4, 128, 256, 16, dt, dt).pack(torch.zeros(16, 256, dtype=torch.uint8, device=dev), torch.ones(32, 1, device=dev).to(tdt),
                                                          torch.ones(32, 1, device=dev).to(tdt))
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

    def rotation(E, top_k):
        steps = max(1, min(E // top_k, 16))
        host_ids = [[(i * top_k + j) % E for j in range(top_k)] for i in range(steps)]
        return steps, host_ids, [torch.tensor([row], dtype=torch.int64, device=dev) for row in host_ids]

    sep = torch.zeros(64, device=dev)

    def stepper(fn, steps):
        def step():
            out = []
            for i in range(steps):
                out.append(fn(i))
                sep.add_(1.0)
            return out
        return step

    def report(cell, dtype, graphs, steps, per_step, extra=None):
        t_sep = time_graph(graphs.pop("sep")[0])
        for variant, (g, _) in graphs.items():
            t = time_graph(g)
            print(json.dumps(dict({"cell": cell, "dtype": dtype, "variant": variant, "us": (t - t_sep) / (steps * per_step)}, **(extra or {}))), flush=True)

    for tdt, tname in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
        for label, N, K, top_k, E, force in CELLS:
            ex, ix = mx_experts(N, K, E, tdt), int_experts(N, K, E, tdt)
            steps, host_ids, dev_ids = rotation(E, top_k)
            x = (torch.randn(1, K, generator=torch.Generator().manual_seed(1)) * 0.5).to(tdt).to(dev)
            graphs = {"1": capture(stepper(lambda i: ex(x, dev_ids[i]), steps)),
                      "2": capture(stepper(lambda i: [ex.expert(e)(x) for e in host_ids[i]], steps)),
                      "3": capture(stepper(lambda i: ix(x, dev_ids[i]), steps)),
                      "sep": capture(stepper(lambda i: None, steps))}
            if force:
                for w in (4, 8, 16):
                    X.MX_WAVES_OVERRIDE = w
                    graphs[f"w{w}"] = capture(stepper(lambda i: ex(x, dev_ids[i]), steps))
                X.MX_WAVES_OVERRIDE = None
            y1, y2 = graphs["1"][1], graphs["2"][1]
            dev_rel = max(float((y1[i][0, j].float() - y2[i][j][0].float()).abs().max() / y2[i][j][0].float().abs().mean())
                          for i in range(steps) for j in range(top_k))
            assert dev_rel < 0.05, (label, dev_rel)  # (the two routes sum K in different orders: close, not bit-identical)
            if force:
                assert all(torch.equal(a, b) for w in (4, 8, 16) for a, b in zip(y1, graphs[f"w{w}"][1])), label  # the bits do not depend on the block size
            report(label, tname, graphs, steps, top_k, {"max_dev_vs_layers": dev_rel})
            del graphs, ex, ix, y1, y2
        # the GLU launch of the Mixtral gate/up pair, block sizes forced
        gu = mx_experts(2 * 14336, 4096, 8, tdt)
        steps, _, dev_ids = rotation(8, 2)
        x = (torch.randn(1, 4096, generator=torch.Generator().manual_seed(1)) * 0.05).to(tdt).to(dev)
        graphs = {"glu": capture(stepper(lambda i: gu.forward_glu(x, dev_ids[i]), steps)), "sep": capture(stepper(lambda i: None, steps))}
        for w in (4, 8, 16):
            X.MX_WAVES_OVERRIDE = w
            graphs[f"glu w{w}"] = capture(stepper(lambda i: gu.forward_glu(x, dev_ids[i]), steps))
        X.MX_WAVES_OVERRIDE = None
        report("mixtral [gate; up] 28672x4096 GLU", tname, graphs, steps, 2)
        del graphs, gu
        for label, hidden, inter, top_k, E in MLPS:
            mlp = GemLiteExpertsMLP(mx_experts(2 * inter, hidden, E, tdt, 1), mx_experts(hidden, inter, E, tdt, 2))
            steps, _, dev_ids = rotation(E, top_k)
            x = (torch.randn(1, hidden, generator=torch.Generator().manual_seed(1)) * 0.05).to(tdt).to(dev)
            w = torch.rand(1, top_k, device=dev)

            def chain(i):
                y = mlp.gate_up(x, dev_ids[i]).float()
                h = (torch.nn.functional.silu(y[..., :inter]) * y[..., inter:]).to(tdt)
                return (mlp.down(h, dev_ids[i]).float() * w.unsqueeze(-1)).sum(-2).to(tdt)

            graphs = {"mlp": capture(stepper(lambda i: mlp(x, dev_ids[i], w), steps)), "mlp-chain": capture(stepper(chain, steps)),
                      "sep": capture(stepper(lambda i: None, steps))}
            report(label, tname, graphs, steps, 1)
            del graphs, mlp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays)
    rows, order = {}, []
    for run in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays)], stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"worker failed with {p.returncode}")
        print(f"process {run + 1} of {a.runs} done", file=sys.stderr, flush=True)
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                key = (r["cell"], r["dtype"])
                if key not in order:
                    order.append(key)
                rows.setdefault(key, {}).setdefault(r["variant"], []).append(r["us"])
    print(f"probe_experts_mx: {a.runs} processes, {a.replays} replays per window; us per slot (mlp: per token): median over processes (spread = max - min)")
    for key in order:
        print(f"\n{key[0]}   {key[1]}")
        med = {}
        for v, vals in rows[key].items():
            med[v] = (statistics.median(vals), max(vals) - min(vals))
            print(f"  {v:>9}: {med[v][0]:8.3f} us   spread {med[v][1]:.3f}   runs {' '.join(f'{t:.3f}' for t in vals)}")
        for a_, b_ in (("1", "2"), ("mlp", "mlp-chain")):
            if a_ in med and b_ in med:
                gap, spread = med[b_][0] - med[a_][0], max(med[a_][1], med[b_][1])
                verdict = "ahead by more than three spreads" if gap > 3 * spread else ("ahead, within three spreads" if gap > 0 else "BEHIND")
                print(f"  {b_} - {a_} = {gap:+.3f} us (spread {spread:.3f}): {verdict}")


if __name__ == "__main__":
    main()
