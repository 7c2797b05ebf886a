"""The contract of `gemlite_hip_quantize_rows` (include/gemlite_hip.h) restated in torch, on the CPU: float weights
[N, K] -> channel-wise symmetric 8-bit codes + one scale per row.  Every step is one fp32 operation on tensors (a CPU tensor divided by a
CPU tensor is a true division; no Python scalar takes part in the arithmetic).

    quantize_rows_spec(W, fmt, scale_rule, scale_dtype) -> (code bytes uint8 [N, K], scales [N, 1] of scale_dtype)

fmt: "int8" | "e4m3" | "e5m2".  scale_rule 0: s = amax / qmax; 1: s = amax * (1.0f / qmax).  A row that holds a NaN or an Inf gets a
non-finite scale (its codes are unspecified in the contract; here they are whatever torch leaves).
`planted_weights_rows` builds the inputs of the tests: random rows over thirty binades plus rows that sit on every edge of the contract."""
import torch

FORMATS = {"int8": (0, torch.int8, 127.0, -128.0), "e4m3": (1, torch.float8_e4m3fn, 448.0, -448.0),
           "e5m2": (2, torch.float8_e5m2, 57344.0, -57344.0)}  # name -> (format code, torch dtype, qmax, qmin)
BY_DTYPE = {v[1]: k for k, v in FORMATS.items()}


def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def row_scale(amax: torch.Tensor, fmt: str, scale_rule: int) -> torch.Tensor:
    """fp32 amax -> fp32 scale; torch.maximum keeps a NaN"""
    qmax = _f32(FORMATS[fmt][2])
    s = amax / qmax if scale_rule == 0 else amax * (_f32(1.0) / qmax)
    return torch.maximum(s, _f32(1e-6))


def quantize_rows_spec(W: torch.Tensor, fmt: str, scale_rule: int, scale_dtype: torch.dtype = torch.float32):
    _, qdt, qmax, qmin = FORMATS[fmt]
    assert W.dim() == 2 and W.device.type == "cpu" and scale_rule in (0, 1)
    Wf = W.float()  # exact
    s = row_scale(Wf.abs().amax(dim=1, keepdim=True), fmt, scale_rule)
    q = torch.minimum(torch.maximum(Wf / s, _f32(qmin)), _f32(qmax))
    codes = torch.round(q).to(torch.int8) if fmt == "int8" else q.to(qdt)  # round: half to even; .to(fp8): one RNE conversion
    return codes.view(torch.uint8), s.to(scale_dtype)


# ------------------------------------------------------------------------------------------------------------------------------------
def _rule_differs(qmax: float):
    """the smallest amax m / 128, m in 128 .. 255 (exact in bf16, fp16 and fp32), whose scale differs between the two rules"""
    fmt = {127.0: "int8", 448.0: "e4m3", 57344.0: "e5m2"}[qmax]
    a = torch.arange(128, 256, dtype=torch.float32) / 128
    differ = row_scale(a, fmt, 0).view(torch.int32) != row_scale(a, fmt, 1).view(torch.int32)
    assert differ.any(), f"no amax in [1, 2) separates the scale rules for qmax = {qmax}"
    return float(a[differ][0])


RULE_DIFFERS = {"int8": _rule_differs(127.0), "e4m3": 1.5, "e5m2": _rule_differs(57344.0)}  # per format: an amax for which rule 0 != rule 1
for _fmt, _a in RULE_DIFFERS.items():  # (qmax 448: 0.75, 1.5, 3.0, the same significand)
    assert row_scale(_f32(_a), _fmt, 0).view(torch.int32) != row_scale(_f32(_a), _fmt, 1).view(torch.int32), (_fmt, _a)

# ties of the three code formats when the scale is 1: int8 halves; e4m3 17 -> 16, 19 -> 20, 1.0625 -> 1.0, 1.1875 -> 1.25, subnormal results
# 2^-10 -> 0, 3 * 2^-10 -> 2^-8; e5m2 4.5 -> 4, 5.5 -> 6, 9 -> 8, 11 -> 12, subnormal results 2^-17 -> 0, 3 * 2^-17 -> 2^-15
TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 17.0, -19.0, 2.0 ** -10, -3 * 2.0 ** -10, 1.0625, -1.1875, 4.5, 5.5, -9.0, 11.0, 2.0 ** -17,
        -3 * 2.0 ** -17, 7 * 2.0 ** -10, 126.5, -126.5]


def _planted_rows(K: int, dtype: torch.dtype, gen: torch.Generator):
    """rows of K fp32 values, every one exact in `dtype`"""
    def fill(amax, at=0, sign=1.0):  # amax at column `at`, smaller random values elsewhere
        v = ((torch.rand(K, generator=gen) * 1.5 - 0.75) * amax).to(dtype).float()
        v[at % K] = sign * amax
        return v

    def ties(qmax):  # amax = qmax: s = 1 under rule 0
        v = fill(qmax)
        t = torch.tensor(TIES)
        n = min(K - 1, t.numel())
        v[1:1 + n] = t[:n]
        return v

    negz = fill(3.0, at=K // 2)
    negz[0::3] = -0.0
    negz[K // 2] = 3.0
    rows = [ties(127.0), ties(448.0), torch.zeros(K), fill(2.0 ** -14), fill(5.0, at=K // 2, sign=-1.0), fill(3.0, at=0), fill(3.0, at=K - 1),
            negz, ties(57344.0)]
    rows += [fill(RULE_DIFFERS[fmt], at=K // 3) for fmt in FORMATS]
    return rows


def planted_weights_rows(N: int, K: int, dtype: torch.dtype, seed: int) -> torch.Tensor:
    """[N, K] of `dtype` on the CPU: random rows whose magnitude changes row by row from 2^-20 to 2^10, and the planted rows — int8 /
    e4m3 / e5m2 ties under amax = qmax, an all-zero row, a row under the 1e-6 floor, a negative amax, amax in the first / last column,
    -0.0 elements, an amax that separates the scale rules per format — spread over the matrix, as many as N - 1 allows (row 0 stays
    random; which ones a small N gets rotates with the seed)."""
    gen = torch.Generator().manual_seed(seed)
    mags = 2.0 ** (((torch.arange(N) * 7 + seed) % 31) - 20).float()
    W = (torch.randn(N, K, generator=gen) * mags.unsqueeze(1)).to(dtype).float()
    rows = _planted_rows(K, dtype, gen)
    rows = rows[seed % len(rows):] + rows[:seed % len(rows)]
    fit = rows[:max(0, N - 1)]
    step = max(1, (N - 1) // max(1, len(fit)))
    for i, r in enumerate(fit):
        W[1 + i * step] = r
    out = W.to(dtype)
    assert torch.isfinite(out.float()).all() and torch.equal(out.float(), W)  # every planted value is exact in dtype
    return out
