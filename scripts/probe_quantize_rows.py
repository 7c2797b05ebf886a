"""Device time of the channel-wise 8-bit weight quantiser, bf16 -> int8 / e4m3fn, one process:
  (k) the kernel: one gemlite_hip_quantize_rows launch (quant_utils._quantize_rows, the rule the processors pass);
  (t) the torch sequence the processors ran before (quant_utils._quantize_rows_torch, seven launches) on the same GPU tensor.
Both are timed with torch events around the whole call — the only clock (t) has — and (k) also per launch with the library's profile
events (bench_utils.kernel_device_us).  Warm: the same weight every time (a weight below 256 MiB is then served from the Infinity Cache).
HBM-cold: every timed call takes another copy of the weight, out of a set of at least 768 MiB that is walked once, behind a 1 GiB
flush (the rotation of DESIGN section 5).  GB/s counts the weight read once and the codes and scales written: N K (in + 1) + 4 N bytes;
"of peak" is against 8 TB/s.  It also counts the bytes in which (t) differs from (k) under each scale rule.
Usage: python scripts/probe_quantize_rows.py [N K]..."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from gemlite_amd import quant_utils as Q  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402

HBM_PEAK_GBS = 8000.0
COLD_SET_BYTES = 768 << 20


def event_us(fn, args, iters, warmup_arg=None):
    """median device us of fn(arg) over `iters` calls, arg = args[i % len(args)]; one untimed call on warmup_arg first"""
    if warmup_arg is not None:
        fn(warmup_arg)
    times = []
    for i in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(args[i % len(args)])
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def bits(t):
    return t.view(torch.uint8) if t.element_size() == 1 else t.view(torch.int32)


def main():
    shapes = [(4096, 4096), (8192, 8192), (11008, 4096), (4096, 14336), (16384, 16384), (4096, 128)]
    if len(sys.argv) > 2:
        shapes = [(int(sys.argv[i]), int(sys.argv[i + 1])) for i in range(1, len(sys.argv) - 1, 2)]
    _hip.load()
    dev = torch.device("cuda", 0)
    rule = Q.ROWS_SCALE_RULE
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    print(f"# {torch.cuda.get_device_properties(0).name}; bf16 -> channel-wise 8-bit; us = device time (median of torch events around the call; "
          f"'launch' = mean of the library's per-launch events); GB/s = (N K 3 + 4 N) / us; scale rule {rule}", flush=True)
    for N, K in shapes:
        torch.manual_seed(0)
        nbytes = N * K * 3 + 4 * N
        ncopies = max(2, -(-COLD_SET_BYTES // (N * K * 2)))
        Ws = [(torch.randn(N, K, device=dev) * 0.05).to(torch.bfloat16) for _ in range(ncopies)]
        cold_iters = min(ncopies - 1, 20) if ncopies > 2 else 6  # two copies: each is a cold set of its own (>= 384 MiB)
        for qdt in (torch.int8, torch.float8_e4m3fn):
            kern = lambda W: Q._quantize_rows(W, qdt, torch.float32, rule)  # noqa: E731
            tor = lambda W: Q._quantize_rows_torch(W, qdt)  # noqa: E731
            qt, st = tor(Ws[0])
            diff = []
            for r in (0, 1):
                qk, sk = Q._quantize_rows(Ws[0], qdt, torch.float32, r)
                diff.append((int((bits(qk) != bits(qt)).sum()), int((bits(sk) != bits(st)).sum())))
            del qt, st, qk, sk
            big = N * K > (1 << 26)
            warm_k = event_us(kern, [Ws[-1]], 20, Ws[-1])
            warm_t = event_us(tor, [Ws[-1]], 5 if big else 20, Ws[-1])
            warm_l = kernel_device_us(lambda: kern(Ws[-1]), iters=20)
            flush.zero_()
            cold_k = event_us(kern, Ws[:-1], cold_iters)
            flush.zero_()
            cold_t = event_us(tor, Ws[:-1], cold_iters)
            i = [0]

            def next_cold():
                i[0] += 1
                return kern(Ws[(i[0] - 1) % (ncopies - 1)])

            flush.zero_()
            cold_l = kernel_device_us(next_cold, iters=cold_iters, warmup=0)
            gbs = lambda us: nbytes / us / 1e3  # noqa: E731
            name = "int8" if qdt == torch.int8 else "e4m3fn"
            print(f"{N} x {K} {name}: {nbytes / 1e6:.1f} MB moved; torch on the GPU differs from the kernel in (codes, scales): rule 0 {diff[0]}, "
                  f"rule 1 {diff[1]}")
            for tag, k, t, l in (("warm", warm_k, warm_t, warm_l), ("cold", cold_k, cold_t, cold_l)):
                print(f"  {tag}: kernel {k:9.1f} us {gbs(k):6.0f} GB/s = {gbs(k) / HBM_PEAK_GBS:.2f} of peak (launch {l:9.1f} us {gbs(l):6.0f} GB/s = "
                      f"{gbs(l) / HBM_PEAK_GBS:.2f}) | torch {t:9.1f} us | torch / kernel = {t / k:.1f} x", flush=True)
        del Ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
