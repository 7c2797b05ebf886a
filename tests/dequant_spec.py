"""The contract of `gemlite_hip_dequantize` (include/gemlite_hip.h) restated in torch on the CPU: a layer's stored
tensors -> the weight W[N, K] it multiplies by.  Every step is one fp32 operation, then one round-to-nearest-even conversion:

    integer / plain layers   q = the code of the packed word, or the unpacked element, as fp32 (exact)
      W_group_mode 0: d = q | 1: d = q - z | 2: d = q * s | 3: d = (q - z) * s | 4: d = fmaf(q, s, z')
      channel_scale_mode 1 or 3: d = d * c[n]
    block-scaled layers      MXFP8 / MXFP4: d = elem * 2^(b - 127) (b = 0xFF: NaN);  NVFP4: d = elem * float(s8)
    post_scale != 1: d = d * post_scale;     out = round_to(fp16 | bf16 | fp32, d)

The fma of mode 4 is taken in float64 and rounded once to fp32.  That equals fmaf whenever the float64 sum is exact, which the Fast2Sum
identities (t - p) == z' and (t - z') == p prove for the data at hand: the restatement asserts them instead of assuming them (they hold
for metadata magnitudes in [2^-20, 2^20] or zero: q * s and z' of one element then span at most 19 + 11 significant bits)."""
import torch

E2M1 = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0, -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0], dtype=torch.float32)
MX_CODES = (14, 15, 16, 17, 18)  # DType.MXFP16 .. DType.NVFP4
NVFP4 = 18


def unpack_words(W_q: torch.Tensor, nbits: int) -> torch.Tensor:
    """packed words [K/e, N] (uint8 / int16 / int32, any strides) -> codes [N, K] int64; element i of a word at bits [nbits i, nbits (i + 1))"""
    bits = W_q.element_size() * 8
    e = bits // nbits
    w = W_q.detach().cpu().to(torch.int64) & ((1 << bits) - 1)
    q = torch.stack([(w >> (nbits * i)) & ((1 << nbits) - 1) for i in range(e)], dim=1)  # [K/e, e, N]
    return q.reshape(-1, w.shape[1]).t().contiguous()


def fma_once(q: torch.Tensor, s: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """fmaf(q, s, z) of fp32 tensors: the float64 product is exact (at most 24 + 24 bits), the float64 sum is asserted exact, one rounding"""
    p = q.double() * s.double()
    t = p + z.double()
    fin = torch.isfinite(t)
    assert torch.equal((t - p)[fin], z.double().expand_as(t)[fin]) and torch.equal((t - z.double())[fin], p[fin]), \
        "q * s + z' is not exact in float64 for this data: the restatement cannot stand for fmaf here"
    return t.float()


def dequant_int_spec(q, s, z, c, w_mode: int, out_dtype: torch.dtype, post_scale: float = 1.0) -> torch.Tensor:
    """q fp32 [N, K]; s, z fp32 broadcastable to [N, K] (or None); c fp32 [N] channel scales (or None)"""
    if w_mode == 0:
        d = q
    elif w_mode == 1:
        d = q - z
    elif w_mode == 2:
        d = q * s
    elif w_mode == 3:
        d = (q - z) * s
    elif w_mode == 4:
        d = fma_once(q, s.expand_as(q), z.expand_as(q))
    else:
        raise ValueError(w_mode)
    if c is not None:
        d = d * c.reshape(-1, 1)
    if post_scale != 1.0:
        d = d * torch.tensor(post_scale, dtype=torch.float32)
    return d.to(out_dtype)


def scale_values(scale_bytes: torch.Tensor, e4m3: bool) -> torch.Tensor:
    """block-scale bytes -> fp32: e8m0 2^(b - 127) with 0xFF = NaN, or e4m3fn"""
    b = scale_bytes.contiguous().view(torch.uint8)
    return b.view(torch.float8_e4m3fn).float() if e4m3 else b.view(torch.float8_e8m0fnu).float()


def dequant_mx_spec(elem: torch.Tensor, scale_bytes: torch.Tensor, group: int, e4m3_scales: bool, out_dtype: torch.dtype,
                    post_scale: float = 1.0) -> torch.Tensor:
    """elem fp32 [N, K] element values, scale_bytes uint8 [N, K / group]"""
    N, K = elem.shape
    d = (elem.reshape(N, K // group, group) * scale_values(scale_bytes, e4m3_scales).reshape(N, K // group, 1)).reshape(N, K)
    if post_scale != 1.0:
        d = d * torch.tensor(post_scale, dtype=torch.float32)
    return d.to(out_dtype)


def expand_groups(m: torch.Tensor, group: int, K: int) -> torch.Tensor:
    """metadata [K/g, N] (the layer's layout) -> fp32 [N, K]"""
    return m.detach().cpu().float().t().repeat_interleave(group, dim=1)[:, :K]


def layer_spec(W_q, scales, zeros, meta_args, out_dtype: torch.dtype) -> torch.Tensor:
    """What `GemLiteLinear.dequantize(out_dtype)` must return, from the layer's `get_tensor_args()` / `get_meta_args()` (any device)."""
    (_sa, nbits, group, _mask, e, in_dt, _out, _acc, _meta, c_mode, w_mode, _contig) = [int(v) for v in meta_args]
    W_q, scales, zeros = W_q.detach().cpu(), scales.detach().cpu(), zeros.detach().cpu()
    N, K = W_q.shape[1], W_q.shape[0] * e
    if in_dt in MX_CODES:
        if nbits == 8:
            elem = W_q.t().float()
        else:
            elem = E2M1[unpack_words(W_q, 4)] if e == 2 else E2M1[(W_q.t().to(torch.int64) & 15)]
        return dequant_mx_spec(elem.contiguous(), scales.contiguous().view(torch.uint8), group, in_dt == NVFP4, out_dtype,
                               0.05 if in_dt == NVFP4 else 1.0)
    q = unpack_words(W_q, nbits).float() if e > 1 else W_q.t().float()
    need_s, need_z = w_mode >= 2, w_mode in (1, 3, 4)
    s = expand_groups(scales, group, K) if need_s else None
    z = None
    if need_z:
        z = zeros.float().reshape(1, 1) if zeros.numel() == 1 else expand_groups(zeros, group, K)
    c = scales.float().reshape(-1)[:N] if c_mode in (1, 3) else None
    return dequant_int_spec(q, s, z, c, w_mode, out_dtype)


def same(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit equality of two float tensors, any NaN equal to any NaN"""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    na, nb = torch.isnan(a), torch.isnan(b)
    return bool(torch.equal(na, nb) and torch.equal(a.contiguous().view(it)[~na], b.contiguous().view(it)[~nb]))


def describe_mismatch(a: torch.Tensor, b: torch.Tensor) -> str:
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    bad = ~((a == b) | (torch.isnan(a) & torch.isnan(b)))
    idx = bad.nonzero()[:5].tolist()
    return f"{int(bad.sum())} of {a.numel()} differ, first at {idx}: " + ", ".join(f"{a[tuple(i)].item()} vs {b[tuple(i)].item()}" for i in idx)
