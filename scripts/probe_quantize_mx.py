"""Device time and peak memory of the block-scaled weight quantiser (gemlite_hip_quantize_mx), bf16 -> MXFP8 / MXFP4 / NVFP4, in three forms,
one process:
  (a) the fused launch: the layer's own tensors (elements two codes per byte for the fp4 formats, scale bytes [K/g, N]);
  (b) the unpacked launch (one code per byte, scales [N * K/g, 1]), then what pack() does today: pack_weights_over_cols to bytes and the
      [K/g, N] transpose of the scales;
  (c) the torch code of WeightQuantizerMXFP on the GPU (what from_linear ran before the kernel existed), then the same pack().
(a) and the launch of (b) are timed per launch with the library's profile events (bench_utils.kernel_device_us); all three also with torch
events around the whole sequence, which is the only clock (c) has.  GB/s counts the input read once and the elements and scales written;
"of peak" is against 8 TB/s.  "peak MB" is torch.cuda.max_memory_allocated() above what was allocated before the call (the outputs included).
It also counts the bytes in which (c), torch ops on the GPU, differs from the kernel.
Usage: python scripts/probe_quantize_mx.py [N K]..."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from gemlite_amd import quant_utils as Q  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402
from gemlite_amd.bitpack import pack_weights_over_cols  # noqa: E402

HBM_PEAK_GBS = 8000.0


def layer_tensors(q, s, N, K, fmt):
    """pack()'s work on the quantiser's return: bytes [N, K/2] for the fp4 formats, scale bytes [K/g, N]"""
    if fmt != "mxfp8":
        q, _ = pack_weights_over_cols(q.view(N, K), W_nbits=4, packing_bitwidth=8, transpose=False)
    return q.view(N, -1), s.view(torch.uint8).view(N, -1).t().contiguous()


def torch_path(W, fmt):
    """WeightQuantizerMXFP's torch code on W's device, whatever the kernel would take"""
    keep = Q._takes_mx_kernel
    Q._takes_mx_kernel = lambda *a, **k: False
    try:
        wq = Q.WeightQuantizerMXFP(device=W.device)
        fn = {"mxfp8": wq.quantize_mxfp8, "mxfp4": wq.quantize_mxfp4, "nvfp4": wq.quantize_nvfp4}[fmt]
        return fn(W, index=True)
    finally:
        Q._takes_mx_kernel = keep


def event_us(fn, iters=10, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    times.sort()
    return times[len(times) // 2]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 1e6


def main():
    shapes = [(4096, 4096), (8192, 28672)]
    if len(sys.argv) > 2:
        shapes = [(int(sys.argv[i]), int(sys.argv[i + 1])) for i in range(1, len(sys.argv) - 1, 2)]
    _hip.load()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_properties(0).name}; bf16 -> block-scaled; us = device time, GB/s = (input + elements + scales) / us", flush=True)
    for N, K in shapes:
        torch.manual_seed(0)
        W = (torch.randn(N, K, device=dev) * 0.05).to(torch.bfloat16)
        big = N * K > (1 << 26)
        for fmt, (_, g) in Q.MX_FORMATS.items():
            out_bytes = (N * K if fmt == "mxfp8" else N * K // 2) + N * (K // g)
            nbytes = N * K * 2 + out_bytes
            fused = lambda: Q._quantize_mx(W, fmt, layer_layout=True)  # noqa: E731
            plain = lambda: Q._quantize_mx(W, fmt, layer_layout=False)  # noqa: E731
            unfused = lambda: layer_tensors(*plain(), N, K, fmt)  # noqa: E731
            torch_all = lambda: layer_tensors(*torch_path(W, fmt), N, K, fmt)  # noqa: E731
            qa, sa = fused()
            qb, sb = unfused()
            qc, sc = torch_all()
            same_ab = torch.equal(qa.view(torch.uint8), qb.view(torch.uint8)) and torch.equal(sa, sb)
            dq = int((qa.view(torch.uint8) != qc.view(torch.uint8)).sum())
            ds = int((sa != sc).sum())
            del qb, sb, qc, sc
            a_k = kernel_device_us(fused, iters=20)
            b_k = kernel_device_us(plain, iters=20)
            a_e = event_us(fused)
            b_e = event_us(unfused)
            c_q = event_us(lambda: torch_path(W, fmt), iters=3 if big else 10, warmup=1)
            c_e = event_us(torch_all, iters=3 if big else 10, warmup=1)
            a_m, c_m = peak_mb(fused), peak_mb(torch_all)
            gbs = lambda us: nbytes / us / 1e3  # noqa: E731
            print(f"{N} x {K} {fmt}: {nbytes / 1e6:.1f} MB moved, outputs {out_bytes / 1e6:.1f} MB; (a) == (b): {same_ab}; "
                  f"torch ops on the GPU differ from (a) in {dq} element bytes, {ds} scale bytes")
            print(f"  (a) fused launch            kernel {a_k:9.1f} us {gbs(a_k):6.0f} GB/s = {gbs(a_k) / HBM_PEAK_GBS:.2f} of peak | events {a_e:9.1f} us"
                  f" | peak {a_m:8.1f} MB")
            print(f"  (b) unpacked launch + pack() kernel {b_k:9.1f} us (launch alone) | events {b_e:9.1f} us {gbs(b_e):6.0f} GB/s")
            print(f"  (c) torch ops + pack()       quantise only: events {c_q:9.1f} us | with pack(): events {c_e:9.1f} us {gbs(c_e):6.0f} GB/s"
                  f" | peak {c_m:8.1f} MB | (c) / (a) = {c_e / a_e:.1f} x", flush=True)
            del qa, sa
        del W
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
