"""The zero-point optimiser of `gemlite_hip_quantize_groups_hqq` restated in numpy on the CPU, on top of
tests/quant_int_spec.py (lo / hi / s_r and the final codes are that file's).  ``dtype=np.float64`` is the oracle; ``np.float32``
is the arithmetic of the kernel — the same operations in the same form (w / s_r kept, 1 / s_r and 1 / beta_i as factors, E
compared as the sum over the group) — up to the order of the sums (``perm`` permutes the k of a group before every sum)
and the last bits of the power (``pow_ulp`` scales it by 1 + j 2^-23, j drawn from [-pow_ulp, pow_ulp] with a fixed seed).
``acc`` is the type the two sums of an iteration are accumulated and compared in: by default the kernel's rule, ``dtype`` for
g | 256 and float64 for every other group size (the wave form: thousands of fp32 terms, and one step of a 16-bit zero moves
their sum by less than fp32 resolves)."""
import numpy as np
import torch

from tests.quant_int_spec import THRESHOLD, rT

HQQ_DEFAULTS = dict(iters=20, lp_norm=0.7, beta=10.0, kappa=1.01)


def student_t_weights(N: int, K: int, dtype: torch.dtype, seed: int = 0) -> torch.Tensor:
    """Student-t(4) x 0.02: the heavy-tailed stand-in for trained weights."""
    return torch.from_numpy(np.random.default_rng(seed).standard_t(4, size=(N, K)) * 0.02).to(dtype)


def _round_meta(z: np.ndarray, T: torch.dtype) -> np.ndarray:
    """rT on an array of z's own float type (float64: one rounding, straight to T)."""
    return torch.from_numpy(np.ascontiguousarray(z)).to(T).to(torch.from_numpy(z).dtype).numpy()


def quantize_hqq_spec(W: torch.Tensor, nbits: int, g: int, T: torch.dtype, iters: int = 20, lp_norm: float = 0.7, beta: float = 10.0,
                      kappa: float = 1.01, dtype=np.float64, perm=None, pow_ulp: int = 0, acc=None):
    """W [N, K] (fp16 / bf16 / fp32, finite) -> (q uint8 [N, K], s_r fp32 [N, K/g], z_r fp32 [N, K/g], steps int [N, K/g]); s_r and
    z_r hold values of T, steps is the number of zeros a group accepted."""
    N, K = W.shape
    assert g % 32 == 0 and K % g == 0
    f = np.dtype(dtype).type
    acc = np.dtype(acc).type if acc is not None else (f if 256 % g == 0 else np.float64)  # the kernel's rule: see the module docstring
    qmax = float(2 ** nbits - 1)
    w32 = W.detach().cpu().float().reshape(N * (K // g), g)
    lo32, hi32 = w32.amin(dim=1, keepdim=True), w32.amax(dim=1, keepdim=True)
    s32 = (hi32 - lo32) / qmax
    s32 = torch.where(s32 < THRESHOLD, torch.ones_like(s32), s32)
    s_r32 = rT(s32, T)
    w, s, lo = w32.numpy().astype(f), s_r32.numpy().astype(f), lo32.numpy().astype(f)
    ws, inv_s, pm1 = w / s, f(1) / s, f(lp_norm) - f(1)
    rng = np.random.default_rng(1234)

    def total(x):
        return (x if perm is None else x[:, perm]).sum(axis=1, keepdims=True, dtype=acc)

    def Q(z):
        return np.clip(np.rint(ws + z), f(0), f(qmax))

    def E(z):
        zr = _round_meta(z, T)
        return total(np.abs(w - (Q(zr) - zr) * s))

    z = (-lo) / s
    best_z, best_E = z.copy(), E(z)
    alive = np.ones(z.shape, dtype=bool)
    steps = np.zeros(z.shape, dtype=np.int64)
    b = f(beta)
    for _ in range(iters):
        if not alive.any():
            break
        rb = f(1) / b
        q = Q(z)
        r = w - (q - z) * s
        a = np.abs(r)
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            pw = np.ones_like(a) if pm1 == 0 else np.exp2(pm1 * np.log2(a))  # a == 0: +inf, the shrunk magnitude is max(-inf, 0) = 0
            if pow_ulp:
                pw = pw * (f(1) + rng.integers(-pow_ulp, pow_ulp + 1, size=pw.shape).astype(f) * f(2.0 ** -23))
            e = np.copysign(np.maximum(a - pw * rb, f(0)), r)
        zn = (total((q - ws) + e * inv_s) / acc(g)).astype(f)
        En = E(zn)
        better = alive & (En < best_E)
        best_z, best_E, z = np.where(better, zn, best_z), np.where(better, En, best_E), np.where(better, zn, z)
        steps += better
        alive = better
        b = b * f(kappa)
    z_r = torch.from_numpy(_round_meta(best_z, T).astype(np.float32))
    q = torch.clamp(torch.round(w32 / s_r32 + z_r), 0.0, qmax)
    G = K // g
    return q.to(torch.uint8).reshape(N, K), s_r32.reshape(N, G), z_r.reshape(N, G), torch.from_numpy(steps).reshape(N, G)


def group_errors64(W: torch.Tensor, q: torch.Tensor, s_r: torch.Tensor, z_r: torch.Tensor, g: int) -> torch.Tensor:
    """sum_k |w - (q - z_r) s_r| per group in float64, [N, K/g]: the error of what a layer holding (q, s_r, z_r) computes."""
    N, K = W.shape
    w = W.detach().cpu().double().reshape(N, K // g, g)
    deq = (q.cpu().double().reshape(N, K // g, g) - z_r.cpu().double().reshape(N, K // g, 1)) * s_r.cpu().double().reshape(N, K // g, 1)
    return (w - deq).abs().sum(dim=2)
