"""What the router's top-k costs in ONE launch (gemlite_amd.experts_topk) against the chain of torch ops it replaces, both in captured graphs.

    python scripts/probe_experts_topk.py [--runs 3] [--replays 200] [--windows 5]     the driver: starts the workers, prints the table
    python scripts/probe_experts_topk.py --worker                                      one process: a JSON line per (cell, path)

Paths per cell (E experts, top_k, T tokens, bf16 logits), each in a captured graph of its own that holds `STEPS` back-to-back steps on
STEPS different logits tensors (us per step = replay time / STEPS):
  softmax   launch: experts_topk(l, k)                        chain: softmax(l.float()) -> topk -> v / v.sum -> ids.to(int32)
  sigmoid   launch: experts_topk(l, k, 'sigmoid', bias=b,     chain: s = sigmoid(l.float()); topk(s + b) -> s.gather -> w / w.sum -> w * scale
            scale=2.5)
Whole MLP (one token, A16W4 g128 fp16, the Qwen3-30B-A3B and Mixtral cells of scripts/probe_experts_mlp.py; step i routes to the experts
(i top_k + j) % E through its logits):
  mlp       launch: mlp.forward_routed(x, l, router)          chain: the softmax chain, then mlp(x, ids, w)
Timing: device events around `--replays` replays after 20 warm-up replays of both graphs of a cell; `--windows` windows per path,
ALTERNATING launch / chain / launch / chain (their median is the process's figure); `--runs` processes.  The table gives the median over
runs and the run-to-run spread (max - min) of both paths, and says whether the launch is ahead by more than three spreads.  Every cell
first checks the launch's ids against the chain's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CELLS = [(128, 8), (8, 2), (256, 8), (512, 10)]  # (E, top_k)
TOKENS = (1, 8, 64, 256)
# (label, hidden H, intermediate I, top_k, E)
MLP_CELLS = [("qwen3-30b-a3b H2048 I768 top8 E128", 2048, 768, 8, 128), ("mixtral H4096 I14336 top2 E8", 4096, 14336, 2, 8)]
STEPS = 16


def worker(replays, windows):
    sys.path.insert(0, ROOT)
    import torch
    from gemlite_amd import DType, ExpertsRouter, GemLiteExperts, GemLiteExpertsMLP, GemLiteLinear, experts_topk
    dev = "cuda:0"

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

    def window(g):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            g.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1000.0 / replays / STEPS  # us per step

    def alternate(ga, gb):
        a, b = [], []
        for _ in range(windows):
            a.append(window(ga))
            b.append(window(gb))
        return statistics.median(a), statistics.median(b)

    def softmax_chain(l, k):
        v, i = torch.topk(torch.softmax(l.float(), -1), k, dim=-1)
        return i.to(torch.int32), v / v.sum(-1, keepdim=True)

    def sigmoid_chain(l, k, b, scale):
        s = torch.sigmoid(l.float())
        _, i = torch.topk(s + b, k, dim=-1)
        w = s.gather(-1, i)
        return i.to(torch.int32), w / w.sum(-1, keepdim=True) * scale

    def report(cell, path, t_launch, t_chain):
        print(json.dumps({"cell": cell, "path": path, "launch_us": t_launch, "chain_us": t_chain}), flush=True)

    gen = torch.Generator().manual_seed(0)
    for E, k in CELLS:
        bias = (torch.randint(-4, 5, (E,), generator=gen).float() / 8).to(dev)
        for T in TOKENS:
            # distinct logits per row (a permutation of a grid bf16 holds exactly for E <= 256, near-exactly above), one tensor per step
            ls = [torch.stack([(torch.randperm(E, generator=gen).float() - E / 2) * (8.0 / E) for _ in range(T)]).to(torch.bfloat16).to(dev)
                  for _ in range(STEPS)]
            for path, launch, chain in (
                    ("softmax", lambda l: experts_topk(l, k), lambda l: softmax_chain(l, k)),
                    ("sigmoid", lambda l: experts_topk(l, k, "sigmoid", True, 2.5, bias), lambda l: sigmoid_chain(l, k, bias, 2.5))):
                ga, ka = capture(lambda: [launch(l) for l in ls])
                gb, kb = capture(lambda: [chain(l) for l in ls])
                torch.cuda.synchronize()
                if path == "softmax" and E <= 256:  # (tie-free in bf16 and the key is the logit: the ids are decided)
                    assert all(torch.equal(ka[i][0], kb[i][0]) for i in range(STEPS)), (E, k, T, path)
                    assert all(torch.allclose(ka[i][1], kb[i][1], rtol=1e-4, atol=1e-7) for i in range(STEPS)), (E, k, T, path)
                else:  # (fp32 keys sigmoid + bias a rounding apart may swap two neighbours between the two paths)
                    same = sum(float((ka[i][0] == kb[i][0]).float().mean()) for i in range(STEPS)) / STEPS
                    assert same >= 0.98, (E, k, T, path, same)
                report(f"E{E} top{k} T{T}", path, *alternate(ga, gb))
                del ga, gb, ka, kb

    tdt = torch.float16

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

    for label, H, I, k, E in MLP_CELLS:
        mlp = GemLiteExpertsMLP(make_experts(2 * I, H, E, 1), make_experts(H, I, E, 2))
        router = ExpertsRouter(k)
        x = (torch.randn(1, H, generator=gen) * 0.5).to(tdt).to(dev)
        ls = []
        for i in range(STEPS):
            l = torch.randn(1, E, generator=gen) * 0.25
            l[0, [(i * k + j) % E for j in range(k)]] += 10.0  # step i routes to the experts (i k + j) % E
            ls.append(l.to(tdt).to(dev))

        def chain(l):
            ids, w = softmax_chain(l, k)
            return mlp(x, ids, w)

        ga, ka = capture(lambda: [mlp.forward_routed(x, l, router) for l in ls])
        gb, kb = capture(lambda: [chain(l) for l in ls])
        torch.cuda.synchronize()
        for i in range(STEPS):
            ref = float(kb[i].float().abs().max())
            assert float((ka[i].float() - kb[i].float()).abs().max()) <= 2e-2 * ref + 1e-3, (label, i)
        report(label, "mlp", *alternate(ga, gb))
        del ga, gb, ka, kb, mlp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays, a.windows)
    rows, order = {}, []
    for run in range(a.runs):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays), "--windows", str(a.windows)],
                           stdout=subprocess.PIPE, text=True, timeout=900)
        if p.returncode != 0:
            sys.exit(f"worker failed with {p.returncode}")
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line)
                key = (r["cell"], r["path"])
                if key not in rows:
                    order.append(key)
                rows.setdefault(key, []).append((r["launch_us"], r["chain_us"]))
    print(f"probe_experts_topk: {a.runs} runs, {a.windows} alternating windows of {a.replays} replays per path; {STEPS} steps per graph; "
          "us per step: median over runs (run-to-run spread = max - min)")
    print(f"{'cell':<38}{'path':<9}{'launch':>10}{'spread':>8}{'chain':>10}{'spread':>8}{'chain - launch':>16}   verdict")
    wins = 0
    for key in order:
        la, ch = [v[0] for v in rows[key]], [v[1] for v in rows[key]]
        ml, mc, sl, sc = statistics.median(la), statistics.median(ch), max(la) - min(la), max(ch) - min(ch)
        gap, spread = mc - ml, max(sl, sc)
        verdict = ("launch ahead by more than three spreads" if gap > 3 * spread else
                   "launch BEHIND by more than three spreads" if -gap > 3 * spread else "within three spreads")
        wins += gap > 3 * spread
        print(f"{key[0]:<38}{key[1]:<9}{ml:10.3f}{sl:8.3f}{mc:10.3f}{sc:8.3f}{gap:16.3f}   {verdict}")
    print(f"the launch is ahead by more than three spreads in {wins} of {len(order)} cells")


if __name__ == "__main__":
    main()
