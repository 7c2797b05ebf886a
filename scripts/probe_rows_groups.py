"""What grouping the few-row rows kernel under capture buys or costs (A16W4 g128 fp16, M = 8 / 16 / 32 / 64): graph-replayed steps of
n INDEPENDENT layers on one x, grouped (the default) against GEMLITE_HIP_CAPTURE_GROUP_ROWS=0, every run its own process, versions
alternating, and — with --parent-root — one run of a build of the parent commit (a tree that holds its own gemlite_amd package).

    python scripts/probe_rows_groups.py [--runs 3] [--replays 200] [--parent-root DIR]      the driver: starts the workers, prints the table
    python scripts/probe_rows_groups.py --worker [--root DIR]                               one process: a JSON line per cell

Cells: 4 and 16 layers of 4096 x 4096, 4 layers of 1024 x 4096 (N x K; 64 blocks per launch), 2 layers of 4096 x 11008 (M <= 32).
A captured graph holds `steps` such steps on DISTINCT layers (so that a replay streams more weights than the 256 MB of Infinity Cache
keep: HBM-cold, like the headline) with one tiny elementwise kernel between two steps, which is what keeps the steps apart in both
versions (a model's norm or activation); its cost is in both versions' figures and is printed next to them ("sep": the same graph
without the layers, per step).  Timing: device events around `--replays` replays after 20 warm-up replays, three windows per process
(their median is the process's figure); us per layer = window / (replays x steps x n).  Every cell also checks that the replayed
outputs of the last step are bit-identical to eager."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
# (label, N, K, layers per step, steps per graph, Ms)
CELLS = [("4096x4096 n=4", 4096, 4096, 4, 12, (8, 16, 32, 64)),
         ("4096x4096 n=16", 4096, 4096, 16, 3, (8, 16, 32, 64)),
         ("1024x4096 n=4", 1024, 4096, 4, 40, (8, 16, 32, 64)),
         ("4096x11008 n=2", 4096, 11008, 2, 8, (8, 16, 32))]


def worker(root, replays):
    sys.path.insert(0, root)
    import ctypes as C
    import torch
    import gemlite_amd
    from gemlite_amd import GemLiteLinear, _hip
    dev, tdt = "cuda:0", torch.float16
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt]
    lib = _hip.load()

    def stats():
        seen, joined = C.c_uint64(0), C.c_uint64(0)
        lib.gemlite_hip_capture_group_stats(C.byref(seen), C.byref(joined))
        return seen.value, joined.value

    def make_layers(n, N, K):
        g = torch.Generator().manual_seed(0)
        out = []
        for _ in range(n):
            lin = GemLiteLinear(4, 128, K, N, code, code)
            W_q = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8).to(dev)
            s = (torch.rand(N * K // 128, 1, generator=g) * 0.002 + 0.0005).to(tdt).to(dev)
            z = (torch.rand(N * K // 128, 1, generator=g) * 15).to(tdt).to(dev)
            lin.pack(W_q, s, z, None, fma_mode=True)
            out.append(lin)
        return out

    def time_graph(step):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        j0 = stats()[1]
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            keep = step()
        joined = stats()[1] - j0
        for _ in range(20):
            g.replay()
        torch.cuda.synchronize()
        windows = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(replays):
                g.replay()
            e1.record()
            e1.synchronize()
            windows.append(e0.elapsed_time(e1) * 1000.0 / replays)  # us per replay
        return statistics.median(windows), joined, keep

    for label, N, K, n, steps, Ms in CELLS:
        lins = make_layers(n * steps, N, K)
        sep = torch.zeros(64, device=dev)
        for M in Ms:
            x = (torch.randn(M, K, generator=torch.Generator().manual_seed(M)) * 0.5).to(tdt).to(dev)
            name = lib.gemlite_hip_kernel_name(C.byref(gemlite_amd.core._call_args(
                x, *lins[0].get_tensor_args(), None, lins[0].get_meta_args(), -1, None, False, 0x1000, (N, 1)))).decode()

            def step():
                outs = []
                for i in range(steps):
                    outs.append([lin(x) for lin in lins[i * n:(i + 1) * n]])
                    sep.add_(1.0)
                return outs[-1]

            def step_sep():
                for i in range(steps):
                    sep.add_(1.0)

            us, joined, outs = time_graph(step)
            us_sep, _, _ = time_graph(step_sep)
            want = [lin(x) for lin in lins[(steps - 1) * n:]]
            torch.cuda.synchronize()
            exact = all(torch.equal(o, w) for o, w in zip(outs, want))
            print("CELL " + json.dumps({"cell": label, "M": M, "kernel": name, "us_per_layer": us / (steps * n), "sep_us_per_step": us_sep / steps,
                                        "joined": joined, "launches": steps * n, "exact": exact}), flush=True)


def run_worker(root, env_extra, replays):
    env = dict(os.environ, **env_extra)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--root", root, "--replays", str(replays)], env=env,
                         capture_output=True, text=True, timeout=300)
    if out.returncode != 0:
        raise SystemExit(f"worker failed ({out.returncode}):\n{out.stdout[-2000:]}\n{out.stderr[-4000:]}")
    return [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CELL ")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a.root, a.replays)
    runs = {"grouped": [], "ungrouped": []}
    for r in range(a.runs):  # alternating, each run its own process
        for version, env in (("grouped", {}), ("ungrouped", {"GEMLITE_HIP_CAPTURE_GROUP_ROWS": "0"})) if r % 2 == 0 else \
                (("ungrouped", {"GEMLITE_HIP_CAPTURE_GROUP_ROWS": "0"}), ("grouped", {})):
            runs[version].append(run_worker(a.root, env, a.replays))
            print(f"# run {r} {version}: done", flush=True)
    parent = run_worker(a.parent_root, {}, a.replays) if a.parent_root else None
    print(f"\nus per layer, median of {a.runs} processes [min .. max]; each process: median of 3 windows of {a.replays} replays")
    print(f"{'cell':<16} {'M':>3} {'kernel':<28} {'ungrouped':>22} {'grouped':>22} {'g/u':>6} {'parent':>7} {'sep/step':>8} {'joined':>9} exact")
    for i, c in enumerate(runs["grouped"][0]):
        col = {}
        for v in ("ungrouped", "grouped"):
            xs = [run[i]["us_per_layer"] for run in runs[v]]
            col[v] = (statistics.median(xs), min(xs), max(xs))
        fmt = lambda t: f"{t[0]:6.2f} [{t[1]:5.2f} .. {t[2]:5.2f}]"
        exact = all(run[i]["exact"] for v in runs for run in runs[v])
        print(f"{c['cell']:<16} {c['M']:>3} {c['kernel']:<28} {fmt(col['ungrouped']):>22} {fmt(col['grouped']):>22} {col['grouped'][0] / col['ungrouped'][0]:6.3f} "
              f"{(parent[i]['us_per_layer'] if parent else float('nan')):7.2f} {c['sep_us_per_step']:8.2f} {c['joined']:>4}/{c['launches']:<4} {exact}")
    print("RAW " + json.dumps({"grouped": runs["grouped"], "ungrouped": runs["ungrouped"], "parent": parent}))


if __name__ == "__main__":
    main()
