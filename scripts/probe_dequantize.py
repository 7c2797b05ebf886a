"""Device time and peak memory of the weight dequantiser (gemlite_hip_dequantize) to bf16, one process, in two forms:
  (a) the kernel: layer.dequantize(torch.bfloat16, out=...) — device time per launch from the library's profile events
      (bench_utils.kernel_device_us) and torch events around the call;
  (b) what the library offered for the same result before the kernel existed: gemlite_hip_unpack_over_cols + torch ops for the grouped INT
      layers, torch ops on the [K, N] view for channel-wise int8, and the torch code of WeightQuantizerMXFP.dequantize on the quantiser's
      return for the block-scaled formats — torch events around the whole sequence, and torch.cuda.max_memory_allocated() above what was
      allocated before the call (the result included).
GB/s counts the layer's tensors read once and the result written once; "of peak" is against 8 TB/s.  The last line of a shape is the general
(per-element) kernel on the same 4-bit weights packed into 8-bit words.
Usage: python scripts/probe_dequantize.py [N K]..."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import GemLiteLinear, _hip, helper  # noqa: E402
from gemlite_amd import quant_utils as Q  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402
from gemlite_amd.dtypes import DType  # noqa: E402

HBM_PEAK_GBS = 8000.0
BF16 = torch.bfloat16


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


def unpack(layer):
    N, K = layer.out_features, layer.in_features
    q = torch.empty((N, K), dtype=torch.uint8, device=layer.W_q.device)
    rc = _hip.load().gemlite_hip_unpack_over_cols(layer.W_q.data_ptr(), q.data_ptr(), N, K, layer.W_nbits, 32,
                                                  _hip.current_stream_handle(q.device))
    assert rc == 0
    return q


def torch_int(layer):
    """unpack kernel + torch ops: fma(q, s, z') of a folded layer in fp32, then the cast"""
    N, K, g = layer.out_features, layer.in_features, layer.group_size
    q = unpack(layer).view(N, K // g, g).float()
    s, z = layer.scales.t().float().unsqueeze(-1), layer.zeros.t().float().unsqueeze(-1)
    return torch.addcmul(z, q, s).reshape(N, K).to(BF16)


def torch_int8(layer):
    return (layer.W_q.t().float() * layer.scales.float().view(-1, 1)).to(BF16)


def torch_mx(wq, q, s, shape, dtype=BF16):
    keep = Q.WeightQuantizerMXFP._dequantize_kernel
    Q.WeightQuantizerMXFP._dequantize_kernel = lambda *a, **k: None
    try:
        return wq.dequantize(q, s, shape=shape, dtype=dtype)
    finally:
        Q.WeightQuantizerMXFP._dequantize_kernel = keep


def layer_bytes(layer):
    return sum(t.numel() * t.element_size() for t in (layer.W_q, layer.scales, layer.zeros))


def report(name, N, K, layer, other, other_name):
    out = torch.empty((N, K), dtype=BF16, device=layer.W_q.device)
    kern = lambda: layer.dequantize(BF16, out=out)  # noqa: E731
    want = other()
    same = bool(torch.equal(kern().view(torch.int16), want.view(torch.int16)))
    del want
    nbytes = layer_bytes(layer) + N * K * 2
    a_k, a_e = kernel_device_us(kern, iters=20), event_us(kern)
    big = N * K > (1 << 26)
    b_e = event_us(other, iters=3 if big else 5)
    a_m, b_m = peak_mb(lambda: layer.dequantize(BF16)), peak_mb(other)
    gbs = lambda us: nbytes / us / 1e3  # noqa: E731
    print(f"{N} x {K} {name}: {nbytes / 1e6:.1f} MB moved (result {N * K * 2 / 1e6:.1f} MB); (a) == (b) bit for bit: {same}")
    print(f"  (a) kernel                  {a_k:9.1f} us {gbs(a_k):6.0f} GB/s = {gbs(a_k) / HBM_PEAK_GBS:.2f} of peak | events {a_e:9.1f} us | peak {a_m:8.1f} MB")
    print(f"  (b) {other_name:<24}events {b_e:9.1f} us {gbs(b_e):6.0f} GB/s | peak {b_m:8.1f} MB | (b) / (a) = {b_e / a_e:.1f} x", flush=True)


def main():
    shapes = [(4096, 4096), (8192, 28672)]
    if len(sys.argv) > 2:
        shapes = [(int(sys.argv[i]), int(sys.argv[i + 1])) for i in range(1, len(sys.argv) - 1, 2)]
    _hip.load()
    dev = torch.device("cuda", 0)
    print(f"# {torch.cuda.get_device_properties(0).name}; layer -> bf16 [N, K]; us = device time, GB/s = (layer tensors + result) / us", flush=True)
    for N, K in shapes:
        torch.manual_seed(0)
        W = (torch.randn(N, K, device=dev) * 0.05).to(BF16)
        lin = lambda: torch.nn.Linear(K, N, bias=False, dtype=BF16, device=dev).requires_grad_(False)  # noqa: E731

        def from_w(proc, **kw):
            m = lin()
            m.weight.copy_(W)
            return proc.from_linear(m, **kw)

        layer = from_w(helper.A16W4_RTN_INT(device=dev), group_size=128)
        assert layer.W_group_mode == 4
        report("4-bit g128 mode 4", N, K, layer, lambda: torch_int(layer), "unpack + torch ops")
        layer = from_w(helper.A16W2_RTN_INT(device=dev), group_size=64)
        report("2-bit g64 mode 4", N, K, layer, lambda: torch_int(layer), "unpack + torch ops")
        layer = from_w(helper.A8W8_int8_dynamic(device=dev))
        report("A8W8 int8 channel-wise", N, K, layer, lambda: torch_int8(layer), "torch ops")
        wq = Q.WeightQuantizerMXFP(compute_dtype=BF16, device=dev)
        for name, proc, quant in (("MXFP8", helper.A16W8_MXFP(device=dev, dtype=BF16), wq.quantize_mxfp8),
                                  ("MXFP4", helper.A16W4_MXFP(device=dev, dtype=BF16), wq.quantize_mxfp4),
                                  ("NVFP4", helper.A4W4_NVFP_dynamic(device=dev, dtype=BF16), wq.quantize_nvfp4)):
            layer = from_w(proc)
            q, s = quant(W, index=True)
            post = 0.05 if layer.input_dtype == DType.NVFP4 else None
            other = (lambda: torch_mx(wq, q, s, (N, K))) if post is None else (lambda: (torch_mx(wq, q, s, (N, K), torch.float32) * post).to(BF16))
            report(name + (" (quantiser-level torch code, then * 0.05)" if post else ""), N, K, layer, other, "torch code")
            del q, s
        # the general path: the same 4-bit codes in 8-bit words
        qz = Q.WeightQuantizerINT(4, 128, dtype=BF16).quantize(W)
        layer = GemLiteLinear(4, group_size=128, in_features=K, out_features=N, input_dtype=DType.BF16, output_dtype=DType.BF16)
        layer.pack(*qz, packing_bitwidth=8)
        out = torch.empty((N, K), dtype=BF16, device=dev)
        us = kernel_device_us(lambda: layer.dequantize(BF16, out=out), iters=5, warmup=1)
        nbytes = layer_bytes(layer) + N * K * 2
        print(f"{N} x {K} 4-bit g128 in 8-bit words, general kernel: {us:9.1f} us {nbytes / us / 1e3:6.0f} GB/s", flush=True)
        del W, layer, out, qz
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
