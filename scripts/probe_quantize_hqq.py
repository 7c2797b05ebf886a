"""Device time of the grouped INT weight quantiser with HQQ's zero-point optimiser (gemlite_hip_quantize_groups_hqq),
fp16 -> 4-bit, g = 64 and 128, the layer's packed form with folded zeros, one process:
  (a) the RTN launch (gemlite_hip_quantize_groups);
  (b) the new launch, HQQ's defaults (20 iterations, lp_norm 0.7, beta 10, kappa 1.01);
  (c) the same contract in torch ops on the same GPU, fp32 — what a user would otherwise run: per-group masks, one host
      synchronisation per iteration for the early exit — producing the unpacked codes and metadata only (no packing, no layout).
(a) and (b) are timed per launch with the library's profile events (bench_utils.kernel_device_us), (c) with torch events around the
whole sequence, the only clock it has; (b) is also given under that clock.  The summed |w - w^| of (b) and (c) against (a)'s, and the
share of groups on which (b) and (c) store another zero, are printed first: faster and different is not faster.
Usage: python scripts/probe_quantize_hqq.py [N K]..."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402
from gemlite_amd.quant_utils import _quantize_groups  # noqa: E402

NBITS, T = 4, torch.float16
HQQ = (20, 0.7, 10.0, 1.01)


def torch_hqq(W, g, iters=HQQ[0], lp_norm=HQQ[1], beta=HQQ[2], kappa=HQQ[3]):
    N, K = W.shape
    qmax = float(2 ** NBITS - 1)
    w = W.float().view(N * (K // g), g)
    lo, hi = w.amin(dim=1, keepdim=True), w.amax(dim=1, keepdim=True)
    s = (hi - lo) / qmax
    s = torch.where(s < 2.0 ** -14, torch.ones_like(s), s).to(T).float()
    ws = w / s

    def err(z):
        zr = z.to(T).float()
        return (w - (torch.clamp(torch.round(ws + zr), 0.0, qmax) - zr) * s).abs().sum(dim=1, keepdim=True)

    z = (-lo) / s
    best_z, best_E = z.clone(), err(z)
    alive = torch.ones_like(z, dtype=torch.bool)
    b = beta
    for _ in range(iters):
        if not bool(alive.any()):
            break
        q = torch.clamp(torch.round(ws + z), 0.0, qmax)
        r = w - (q - z) * s
        a = r.abs()
        shrunk = a - (torch.pow(a, lp_norm - 1.0) if lp_norm != 1.0 else 1.0) / b
        e = torch.sign(r) * torch.clamp_min(shrunk, 0.0)  # (a == 0: pow -> inf, shrunk -> -inf, e = 0)
        zn = (q - (w - e) / s).mean(dim=1, keepdim=True)
        En = err(zn)
        better = alive & (En < best_E)
        best_z, best_E, z = torch.where(better, zn, best_z), torch.where(better, En, best_E), torch.where(better, zn, z)
        alive = better
        b *= kappa
    z_r = best_z.to(T)
    q = torch.clamp(torch.round(ws + z_r.float()), 0.0, qmax).to(torch.uint8).view(N, K)
    return q, s.to(T), z_r


def event_us(fn, iters=5, warmup=1):
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


def summed_error(W, q, s, z, g):
    N, K = W.shape
    deq = (q.float().view(-1, g) - z.float().view(-1, 1)) * s.float().view(-1, 1)
    return float((W.float().view(-1, g) - deq).abs().double().sum())


def main():
    shapes = [(4096, 4096), (4096, 14336)]
    if len(sys.argv) > 2:
        shapes = [(int(sys.argv[i]), int(sys.argv[i + 1])) for i in range(1, len(sys.argv) - 1, 2)]
    _hip.load()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_properties(0).name}; fp16 -> {NBITS}-bit, Student-t(4) x 0.02 weights; HQQ defaults {HQQ}; us = device time")
    for N, K in shapes:
        for g in (64, 128):
            torch.manual_seed(0)
            W = (torch.distributions.StudentT(4.0).sample((N, K)) * 0.02).to(device=dev, dtype=torch.float16)
            rtn = lambda: _quantize_groups(W, NBITS, g, T, packed=True, fold_zeros=True)  # noqa: E731
            hqq = lambda: _quantize_groups(W, NBITS, g, T, packed=True, fold_zeros=True, hqq=HQQ)  # noqa: E731
            e_a = summed_error(W, *_quantize_groups(W, NBITS, g, T, packed=False), g)
            qb, sb, zb = _quantize_groups(W, NBITS, g, T, packed=False, hqq=HQQ)
            qc, sc, zc = torch_hqq(W, g)
            e_b, e_c = summed_error(W, qb, sb, zb, g), summed_error(W, qc, sc, zc, g)
            differ = float((zb.view(-1) != zc.view(-1)).float().mean())
            print(f"{N} x {K} g{g}: error / RTN's: (b) {e_b / e_a:.4f}  (c) {e_c / e_a:.4f}; (b) and (c) store another zero on "
                  f"{100 * differ:.2f} % of the groups; scales equal: {torch.equal(sb, sc)}")
            del qb, sb, zb, qc, sc, zc
            a_k, b_k = kernel_device_us(rtn, iters=20), kernel_device_us(hqq, iters=10)
            b_e = event_us(hqq)
            c_e = event_us(lambda: torch_hqq(W, g), iters=3)
            print(f"  (a) RTN launch        kernel {a_k:10.1f} us")
            print(f"  (b) HQQ launch        kernel {b_k:10.1f} us = {b_k / a_k:.1f} x (a) | events {b_e:10.1f} us")
            print(f"  (c) torch ops, fp32   events {c_e:10.1f} us = {c_e / b_k:.1f} x (b)")
            del W
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
