"""Device time of 8- / 16-bit packed words against 32-bit words (the same W_q packed three ways, one process), and of the coverage kernel
that 8-bit words ran on before they had a word source (forced here with a W_q view one byte off, which no specialised kernel takes).
    python scripts/probe_pack_widths.py [--quick]
Prints one JSON line per (shape, M) and a table at the end."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gemlite_amd  # noqa: E402
from gemlite_amd import DType, GemLiteLinear  # noqa: E402
from gemlite_amd.bench_utils import kernel_device_us  # noqa: E402
from gemlite_amd.core import _hip_matmul, _static_args  # noqa: E402
from gemlite_amd import _hip  # noqa: E402
from oracle import gemlite_oracle as O  # noqa: E402

DEV = "cuda:0"
SHAPES = [(4, 4096, 4096), (4, 8192, 8192), (4, 11008, 4096), (4, 4096, 14336), (2, 8192, 8192)]  # (W_nbits, N, K), groups of 128
MS = (1, 16, 64, 256, 2048)
QUICK = "--quick" in sys.argv


def name_of(lin, M, w_q=None):
    a = _static_args(lin.W_q if w_q is None else w_q, lin.scales, lin.zeros, lin.get_meta_args())
    a.matmul_type, a.M = -1, M
    a.x = a.out = 0x1000
    a.stride_xm, a.stride_xk, a.stride_om, a.stride_on = lin.in_features, 1, lin.out_features, 1
    a.input_dtype = lin.input_dtype.value
    return _hip.load().gemlite_hip_kernel_name(_hip.C.byref(a)).decode()


def main():
    torch.cuda.set_device(0)
    rows = []
    for nbits, N, K in SHAPES:
        W_q, s, z = O.gen_data(N, K, nbits, 128, seed=0)
        layers = {}
        for pb in (32, 16, 8):
            lin = GemLiteLinear(nbits, 128, K, N, DType.FP16, DType.FP16)
            lin.pack(torch.from_numpy(W_q).to(DEV), torch.from_numpy(s).half().to(DEV), torch.from_numpy(z).half().to(DEV), packing_bitwidth=pb)
            layers[pb] = lin
        for M in MS:
            x = torch.from_numpy(O.gen_x(M, K, seed=M).astype(np.float32)).half().to(DEV)
            r = dict(W_nbits=nbits, N=N, K=K, M=M)
            for pb, lin in layers.items():
                meta = lin.get_meta_args()
                us = kernel_device_us(lambda: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, meta, -1), iters=30 if not QUICK else 10)
                r[f"b{pb}_us"], r[f"b{pb}_kernel"] = round(us, 2), name_of(lin, M)
            if nbits == 4 and N == 4096 and K == 4096 and M in (1, 16, 64, 256):
                lin = layers[8]
                buf = torch.empty(lin.W_q.numel() + 64, dtype=torch.uint8, device=DEV)
                wv = buf[1:1 + lin.W_q.numel()].view(lin.W_q.shape)
                wv.copy_(lin.W_q)
                meta = lin.get_meta_args()
                us = kernel_device_us(lambda: _hip_matmul(x, wv, lin.scales, lin.zeros, None, meta, -1), iters=5, warmup=1)
                r["coverage_b8_us"], r["coverage_kernel"] = round(us, 1), name_of(lin, M, wv)
            print(json.dumps(r), flush=True)
            rows.append(r)
        del layers
        torch.cuda.empty_cache()
    print("\n| W | N x K | M | 32-bit us | 16-bit us (x) | 8-bit us (x) | coverage 8-bit us |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        b32 = r["b32_us"]
        print(f"| {r['W_nbits']} | {r['N']} x {r['K']} | {r['M']} | {b32:.2f} | {r['b16_us']:.2f} ({r['b16_us'] / b32:.2f}) | "
              f"{r['b8_us']:.2f} ({r['b8_us'] / b32:.2f}) | {r.get('coverage_b8_us', '')} |")


if __name__ == "__main__":
    main()
