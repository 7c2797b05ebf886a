"""The contract of `gemlite_hip_quantize_mx` (include/gemlite_hip.h) restated in torch, on the CPU: float weights
[N, K] -> block-scaled elements + one scale byte per block.  Every step is one fp32 operation; the power-of-two scale is taken from the
BITS of amax / qmax (exponent field, + 1 when the mantissa is not zero), not from log2.

    quantize_mx_spec(W, fmt) -> (elements uint8 [N, K], scale bytes uint8 [N, K/g], non-finite block mask bool [N, K/g])

elements: e4m3 bytes ("mxfp8") or one e2m1 code per byte ("mxfp4", "nvfp4"); `pack_nibbles` turns codes into the two-per-byte form.
`planted_weights_mx` builds the inputs of the tests: random rows at seven magnitudes plus blocks that sit on every edge of the contract."""
import torch

FORMATS = {"mxfp8": (0, 32), "mxfp4": (1, 32), "nvfp4": (2, 16)}
FP4_THRESHOLDS = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
E8M0_NAN, E4M3_NAN = 0xFF, 0x7F


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def fp4_codes(q: torch.Tensor) -> torch.Tensor:
    """c = number of thresholds strictly below |q| (a midpoint takes the lower value); + 8 for a negative q that does not round to zero"""
    a = q.abs()
    c = torch.zeros_like(q, dtype=torch.int32)
    for t in FP4_THRESHOLDS:
        c += (a > t).to(torch.int32)
    return torch.where((q < 0) & (c > 0), c + 8, c).to(torch.uint8)


def pack_nibbles(codes: torch.Tensor) -> torch.Tensor:
    """[N, K] codes -> [N, K/2] bytes, even k in the low nibble"""
    return codes[:, 0::2] | (codes[:, 1::2] << 4)


def quantize_mx_spec(W: torch.Tensor, fmt: str):
    _, g = FORMATS[fmt]
    assert W.dim() == 2 and W.shape[1] % 32 == 0 and W.device.type == "cpu"
    N, K = W.shape
    flat = W.float().reshape(-1, g)
    amax = flat.abs().amax(dim=1, keepdim=True)  # NaN if the block holds one
    bad = ~torch.isfinite(amax)
    if fmt == "nvfp4":
        t = (amax / _f32(6.0)) / _f32(0.05)
        s8 = torch.minimum(t, _f32(448.0)).to(torch.float8_e4m3fn)
        full = torch.maximum(s8.float() * _f32(0.05), _f32(1e-6))
        sb = torch.where(bad, torch.tensor(E4M3_NAN, dtype=torch.uint8), s8.view(torch.uint8))
        q = flat / full
    else:
        ideal = amax / _f32(448.0 if fmt == "mxfp8" else 6.0)
        bits = ideal.view(torch.int32)
        ex = (((bits >> 23) & 0xFF) + ((bits & 0x7FFFFF) != 0).to(torch.int32)).clamp(97, 254)
        sb = torch.where(bad, torch.tensor(E8M0_NAN, dtype=torch.uint8), ex.to(torch.uint8))
        q = flat / (ex << 23).view(torch.float32)
    if fmt == "mxfp8":
        el = q.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        el = fp4_codes(q)
    return el.reshape(N, K), sb.reshape(N, K // g), bad.reshape(N, K // g)


# ------------------------------------------------------------------------------------------------------------------------------------
def _ulp_up(v: torch.Tensor) -> torch.Tensor:
    """one unit in the last place of v's own type away from zero (finite v)"""
    it = {torch.float32: torch.int32, torch.float16: torch.int16, torch.bfloat16: torch.int16}[v.dtype]
    return (v.view(it) + 1).view(v.dtype)


def _planted_blocks(dtype: torch.dtype, gen: torch.Generator):
    """32-k blocks (two equal halves of 16, so that an NVFP4 block sees the same pattern), as fp32 values exact in `dtype`"""
    def fill(amax, second=None):  # amax first, (a second planted value), then smaller random values
        v = (torch.rand(16, generator=gen) * 1.5 - 0.75) * amax
        v = v.to(dtype).float()
        v[0] = amax
        if second is not None:
            v[5] = second
        return v

    mid = torch.tensor([6.0, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 1.75, -1.75, 2.5, -2.5, 3.5, -3.5, 5.0, -5.0, -6.0])
    ties = torch.tensor([448.0, 1.0625, -1.1875, 17.0, -19.0, 2.0 ** -10, -3 * 2.0 ** -10, 7 * 2.0 ** -10, 248.0, -1.0625, 2.125, 34.0, 0.53125,
                         -0.59375, 100.0, -448.0])
    tozero = torch.tensor([6.0, -0.25, -0.125, -0.2, -1e-3, -0.0, 0.1, -0.24, 0.25, -0.26, -1e-6, 0.0, -0.05, 0.2, -0.01, -3.0]).to(dtype).float()
    clamp = torch.tensor([3000.0, -3000.0, 100.0, -150.0, 22.0, -160.0, 10.0, 2500.0, -5.0, 0.0, 1.0, -78.0, 135.0, -135.0, 56.0, -1000.0])
    blocks = [mid, ties, tozero, clamp.to(dtype).float(), torch.zeros(16), mid * 2.0 ** -4, ties * 2.0 ** -3]
    for e in (-3, 0, 2):  # amax exactly qmax * 2^e (mantissa of amax / qmax zero: no + 1) and one ulp of the input type above
        for qmax in (448.0, 6.0):
            a = torch.tensor(qmax * 2.0 ** e, dtype=dtype)
            blocks.append(fill(a.float().item()))
            blocks.append(-fill(_ulp_up(a).float().item()))
    tiny = [2.0 ** -24] if dtype == torch.float16 else [2.0 ** -24, 2.0 ** -40, 3 * 2.0 ** -36]  # below the 2^-30 floor of the scale
    for a in tiny:
        v = torch.zeros(16)
        v[0], v[3], v[7] = a, -a, a / 2 if dtype != torch.float16 else 0.0
        blocks.append(v)
    if dtype != torch.float32:  # near the type's maximum: nothing overflows to Inf
        top = torch.finfo(dtype).max
        blocks.append(fill(top, second=-top))
        blocks.append(fill(_ulp_up(torch.tensor(top / 2, dtype=dtype)).float().item()))
    return [torch.cat([b, b]) for b in blocks]


def planted_weights_mx(N: int, K: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """[N, K] of `dtype` on the CPU: random rows at seven magnitudes, with the planted blocks spread over the matrix (as many as fit)."""
    assert K % 32 == 0
    gen = torch.Generator().manual_seed(seed)
    mags = torch.tensor([2.0 ** -16, 2.0 ** -10, 2.0 ** -5, 0.25, 1.0, 16.0, 512.0])
    W = torch.randn(N, K, generator=gen) * mags[torch.arange(N) % 7].unsqueeze(1)
    W = W.to(dtype).float().reshape(-1, 32)
    blocks = _planted_blocks(dtype, gen)
    nb = W.shape[0]
    step = max(1, nb // len(blocks))
    for i, b in enumerate(blocks[:nb]):
        W[i * step] = b
    out = W.reshape(N, K).to(dtype)
    assert torch.isfinite(out.float()).all() and torch.equal(out.float().reshape(-1, 32), W)  # every planted value is exact in dtype
    return out
