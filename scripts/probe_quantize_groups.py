"""Device time of the grouped INT weight quantiser (gemlite_hip_quantize_groups), fp16 -> 4-bit g128, in three forms, one process:
  (a) the fused launch: packed words + [K/g, N] metadata with folded zeros;
  (b) pack_bits = 0 (uint8 codes, [N * K/g, 1] metadata), then the existing gemlite_hip_pack_over_cols;
  (c) the same arithmetic in torch ops on the GPU (+ the existing pack kernel and the metadata transposes for the layer's layout).
(a) and (b) are timed per launch with the library's profile events (bench_utils.kernel_device_us); all three also with torch events
around the whole sequence, which is the only clock (c) has.  GB/s counts the input read once and the words and metadata written.
Usage: python scripts/probe_quantize_groups.py [N K]..."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402
from gemlite_amd.bitpack import pack_weights_over_cols  # noqa: E402
from gemlite_amd.quant_utils import _quantize_groups  # noqa: E402

NBITS, G, T = 4, 128, torch.float16


def torch_quantize(W):
    N, K = W.shape
    qmax = float(2 ** NBITS - 1)
    w = W.float().view(N, K // G, G)
    lo, hi = w.amin(dim=2, keepdim=True), w.amax(dim=2, keepdim=True)
    s = (hi - lo) / qmax
    s = torch.where(s < 2.0 ** -14, torch.ones_like(s), s)
    s_r = s.to(T).float()
    z_r = ((-lo) / s_r).to(T).float()
    q = torch.clamp(torch.round(w / s_r + z_r), 0.0, qmax).to(torch.uint8).view(N, K)
    return q, s_r.to(T).view(-1, 1), z_r.to(T).view(-1, 1)


def torch_layer_tensors(W):
    q, s, z = torch_quantize(W)
    N = W.shape[0]
    words, _ = pack_weights_over_cols(q, W_nbits=NBITS, packing_bitwidth=32, transpose=True)
    zf = (-z.float() * s.float()).to(T)
    return words, s.view(N, -1).t().contiguous(), zf.view(N, -1).t().contiguous()


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


def main():
    shapes = [(4096, 4096), (8192, 28672)]
    if len(sys.argv) > 2:
        shapes = [(int(sys.argv[i]), int(sys.argv[i + 1])) for i in range(1, len(sys.argv) - 1, 2)]
    _hip.load()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_properties(0).name}; fp16 -> {NBITS}-bit g{G}; us = device time, GB/s = (input + words + metadata) / us")
    for N, K in shapes:
        torch.manual_seed(0)
        W = (torch.randn(N, K, device=dev) * 0.05).to(torch.float16)
        nbytes = N * K * 2 + N * K * NBITS // 8 + 2 * 2 * N * (K // G)
        fused = lambda: _quantize_groups(W, NBITS, G, T, packed=True, fold_zeros=True)  # noqa: E731
        plain = lambda: _quantize_groups(W, NBITS, G, T, packed=False)  # noqa: E731
        q, s, z = plain()
        pack = lambda: pack_weights_over_cols(q, W_nbits=NBITS, packing_bitwidth=32, transpose=True)  # noqa: E731
        # same results first (faster and different is not faster)
        wa, sa, za = fused()
        wc, sc, zc = torch_layer_tensors(W)
        same = torch.equal(wa, pack()[0]) and torch.equal(wa, wc) and torch.equal(sa, sc) and torch.equal(za, zc)
        a_k = kernel_device_us(fused, iters=20)
        b_q, b_p = kernel_device_us(plain, iters=20), kernel_device_us(pack, iters=20)
        a_e = event_us(fused)
        b_e = event_us(lambda: (plain(), pack()))
        c_q = event_us(lambda: torch_quantize(W))
        c_e = event_us(lambda: torch_layer_tensors(W))
        gbs = lambda us: nbytes / us / 1e3  # noqa: E731
        print(f"{N} x {K}: {nbytes / 1e6:.1f} MB; (a) == (b) == (c): {same}")
        print(f"  (a) fused launch              kernel {a_k:9.1f} us {gbs(a_k):7.0f} GB/s | events {a_e:9.1f} us {gbs(a_e):7.0f} GB/s")
        print(f"  (b) codes + pack_over_cols    kernel {b_q:9.1f} + {b_p:.1f} = {b_q + b_p:.1f} us {gbs(b_q + b_p):7.0f} GB/s | events {b_e:9.1f} us {gbs(b_e):7.0f} GB/s")
        print(f"  (c) torch ops                 quantise only: events {c_q:9.1f} us | with pack + layout: events {c_e:9.1f} us {gbs(c_e):7.0f} GB/s")
        del W, q, s, z, wa, sa, za, wc, sc, zc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
