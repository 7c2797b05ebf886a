"""What one experts launch with ids on the device costs against what a graph could do before it (A16W4 g128 fp16, one token).

    python scripts/probe_experts.py [--runs 3] [--replays 200]      the driver: starts the workers, prints the table
    python scripts/probe_experts.py --worker                        one process: a JSON line per (cell, variant)

Variants per cell (us per slot = per expert GEMV):
  1  experts(x, ids): ONE launch, the ids a device tensor (measured in both kinds of process: "1" ungrouped process, "1g" grouped process)
  2  top_k captured layer(x) calls on the experts chosen ON THE HOST, GEMLITE_HIP_NO_CAPTURE_GROUPS=1: the parent's ungrouped path
  3  the same with capture grouping on (its own process: the variable is read once)
  4  Qwen gate/up only, the graph-safe fallback of the parent: all E experts run (us per step / top_k, i.e. per USEFUL slot)
A captured graph holds `steps` steps, step i on the experts (i * top_k + j) % E, with one tiny elementwise kernel between two steps in every
variant (a model's activation; it keeps the steps of variants 2 / 3 apart).  Timing: device events around `--replays` replays after 20
warm-up replays of every graph of the cell, three windows per process (their median is the process's figure); the processes of the two
kinds alternate, `--runs` of each; the table gives the median over runs and the spread (max - min).  Every cell first checks that the
experts launch is bit-identical to the per-expert calls where those run the decode3 kernel."""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# (label, N, K, top_k, E, also run all E experts)
CELLS = [("qwen3-30b-a3b gate/up 768x2048", 768, 2048, 8, 128, True),
         ("qwen3-30b-a3b down 2048x768", 2048, 768, 8, 128, False),
         ("mixtral gate/up 14336x4096", 14336, 4096, 2, 8, False),
         ("mixtral down 4096x14336", 4096, 14336, 2, 8, False),
         ("4096x4096 top2", 4096, 4096, 2, 16, False),
         ("4096x4096 top4", 4096, 4096, 4, 16, False),
         ("4096x4096 top8", 4096, 4096, 8, 16, False)]


def worker(replays):
    sys.path.insert(0, ROOT)
    import ctypes as C
    import torch
    import gemlite_amd
    from gemlite_amd import DType, GemLiteExperts, GemLiteLinear, _hip
    dev, tdt = "cuda:0", torch.float16
    lib = _hip.load()
    grouped = lib.gemlite_hip_capture_group_max() >= 2

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

    for label, N, K, top_k, E, all_experts in CELLS:
        ex = make_experts(N, K, E)
        steps = max(1, min(E // top_k, 16))
        host_ids = [[(i * top_k + j) % E for j in range(top_k)] for i in range(steps)]
        dev_ids = [torch.tensor([row], dtype=torch.int64, device=dev) for row in host_ids]
        x = (torch.randn(1, K, generator=torch.Generator().manual_seed(1)) * 0.5).to(tdt).to(dev)
        sep = torch.zeros(64, device=dev)
        lin0 = ex.expert(0)
        name = lib.gemlite_hip_kernel_name(C.byref(gemlite_amd.core._call_args(
            x, *lin0.get_tensor_args(), None, lin0.get_meta_args(), -1, None, False, 0x1000, (N, 1)))).decode()

        def step_experts():
            out = []
            for i in range(steps):
                out.append(ex(x, dev_ids[i]))
                sep.add_(1.0)
            return out

        def step_layers():
            out = []
            for i in range(steps):
                out.append([ex.expert(e)(x) for e in host_ids[i]])
                sep.add_(1.0)
            return out

        def step_sep():
            for _ in range(steps):
                sep.add_(1.0)

        all_ids = torch.arange(E, dtype=torch.int64, device=dev).view(1, E)

        def step_all():
            out = []
            for _ in range(steps):
                out.append(ex(x, all_ids))
                sep.add_(1.0)
            return out

        graphs = {"1g" if grouped else "1": capture(step_experts), "3" if grouped else "2": capture(step_layers), "sep": capture(step_sep)}
        if all_experts and not grouped:
            graphs["4"] = capture(step_all)
        torch.cuda.synchronize()
        y1, y2 = graphs["1g" if grouped else "1"][1], graphs["3" if grouped else "2"][1]
        same = all(torch.equal(y1[i][0, j], y2[i][j][0]) for i in range(steps) for j in range(top_k))
        assert same or not name.startswith("gemv_w4_decode3_kernel"), label
        t_sep = time_graph(graphs["sep"][0])
        for variant, (g, _) in graphs.items():
            if variant == "sep":
                continue
            t = time_graph(g)
            print(json.dumps({"cell": label, "variant": variant, "us_per_slot": (t - t_sep) / (steps * top_k), "us_per_step": (t - t_sep) / steps,
                              "sep_us": t_sep / steps, "steps": steps, "single_layer_kernel": name, "bit_identical": same}), flush=True)
        del graphs, ex


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--replays", type=int, default=200)
    a = ap.parse_args()
    if a.worker:
        return worker(a.replays)
    rows = {}
    info = {}
    for run in range(a.runs):
        for off in (True, False):  # the two kinds of process alternate
            env = dict(os.environ)
            env.pop("GEMLITE_HIP_NO_CAPTURE_GROUPS", None)
            if off:
                env["GEMLITE_HIP_NO_CAPTURE_GROUPS"] = "1"
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--replays", str(a.replays)], env=env, stdout=subprocess.PIPE,
                               text=True, timeout=600)
            if p.returncode != 0:
                sys.exit(f"worker failed with {p.returncode}")
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    rows.setdefault((r["cell"], r["variant"]), []).append(r["us_per_slot"])
                    info[r["cell"]] = r
    print(f"probe_experts: {a.runs} runs per kind of process, {a.replays} replays per window; us per slot: median over runs (spread = max - min)")
    for label, *_ in CELLS:
        i = info[label]
        print(f"\n{label}   single-layer kernel: {i['single_layer_kernel']}   steps/graph {i['steps']}   separator {i['sep_us']:.2f} us/step   "
              f"bit-identical to the per-expert calls: {i['bit_identical']}")
        med = {}
        for v in ("1", "1g", "2", "3", "4"):
            if (label, v) in rows:
                vals = rows[(label, v)]
                med[v] = (statistics.median(vals), max(vals) - min(vals))
                print(f"  variant {v:>2}: {med[v][0]:7.3f} us/slot   spread {med[v][1]:.3f}   runs {' '.join(f'{t:.3f}' for t in vals)}")
        if "1" in med and "2" in med:
            gap, spread = med["2"][0] - med["1"][0], max(med["1"][1], med["2"][1])
            print(f"  variant 2 - variant 1 = {gap:+.3f} us/slot (spread {spread:.3f}): {'ahead by more than the spread' if gap > spread else 'NOT ahead by more than the spread'}")
        if "1g" in med and "3" in med:
            print(f"  variant 1 / variant 3 = {med['1g'][0] / med['3'][0]:.3f} (data-dependent addressing against the best fixed-pointer form)")


if __name__ == "__main__":
    main()
