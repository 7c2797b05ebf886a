"""The grouped INT weight quantiser's contract restated in torch ops on the CPU: what
`gemlite_hip_quantize_groups` is tested against.  Every step is one fp32 operation; `rT` rounds to the
16-bit metadata type (nearest even) and widens back."""
import torch

THRESHOLD = 2.0 ** -14


def rT(t: torch.Tensor, T: torch.dtype) -> torch.Tensor:
    return t.to(T).float()


def quantize_groups_spec(W: torch.Tensor, nbits: int, g: int, T: torch.dtype):
    """W [N, K] (fp16 / bf16 / fp32, any device) -> (q uint8 [N, K], s_r fp32 [N, K/g], z_r fp32 [N, K/g]) on the CPU;
    s_r and z_r hold values of T."""
    N, K = W.shape
    assert g % 32 == 0 and K % g == 0
    qmax = float(2 ** nbits - 1)
    w = W.detach().cpu().float().reshape(N, K // g, g)
    lo, hi = w.amin(dim=2, keepdim=True), w.amax(dim=2, keepdim=True)
    s = (hi - lo) / qmax
    s = torch.where(s < THRESHOLD, torch.ones_like(s), s)
    s_r = rT(s, T)
    z_r = rT((-lo) / s_r, T)
    q = torch.clamp(torch.round(w / s_r + z_r), 0.0, qmax)
    return q.to(torch.uint8).reshape(N, K), s_r.reshape(N, K // g), z_r.reshape(N, K // g)


def folded_zeros_spec(s_r: torch.Tensor, z_r: torch.Tensor, T: torch.dtype) -> torch.Tensor:
    return rT((-z_r) * s_r, T)


def half_spacing(z: torch.Tensor, T: torch.dtype) -> torch.Tensor:
    """Half the spacing of T at |z| (fp32 tensor of T values)."""
    mant, emin = (10, -14) if T == torch.float16 else (7, -126)
    e = torch.floor(torch.log2(z.abs().clamp_min(2.0 ** emin))).clamp_min(float(emin))
    return 0.5 * torch.pow(2.0, e - mant)


def error_bound(nbits: int, s_r: torch.Tensor, z_r: torch.Tensor, T: torch.dtype) -> torch.Tensor:
    """|(q - z_r) s_r - w| <= (max(0.5, qmax u) + h(z_r)) s_r: 0.5 the rounding of the code, qmax u how far hi can land
    past qmax before the clamp because s_r != s, h the rounding of z_r."""
    u = 2.0 ** -11 if T == torch.float16 else 2.0 ** -8
    qmax = float(2 ** nbits - 1)
    return (max(0.5, qmax * u) + half_spacing(z_r, T)) * s_r


def planted_weights(N: int, K: int, g: int, dtype: torch.dtype, seed: int = 0) -> torch.Tensor:
    """Random normal x 0.05 with a constant non-zero group, an all-zero group and a group of range 1e-4 planted (needs
    N >= 1 and K / g >= 1; the three land in the first rows / groups that exist)."""
    gen = torch.Generator().manual_seed(seed)
    W = (torch.randn(N, K, generator=gen) * 0.05).reshape(N, K // g, g)
    slots = [(r % N, (r // N) % (K // g)) for r in range(3)]
    W[slots[0]] = 0.0371
    W[slots[1]] = 0.0
    W[slots[2]] = 0.02 + 1e-4 * torch.rand(g, generator=gen)
    return W.reshape(N, K).to(dtype)
