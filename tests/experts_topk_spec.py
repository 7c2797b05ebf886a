"""The router's top-k restated in numpy float64: what gemlite_hip_experts_topk has to select and what its weights
approximate.  No test in itself; tests/test_experts_topk_cpu.py checks it against torch, tests/test_experts_topk_gpu.py the kernel against it.

Ids: a stable arg-sort of the negated key — descending key, the lower index among equal keys (-0 == +0) — with NaN mapped above +inf.
The key is the logit (softmax; sigmoid without a bias) or sigmoid(logit) + bias.  Weights: softmax of the logits over the selected experts
(renormalize) or over all of them, or sigmoid(logit) (never the bias), divided by the sum over the selected with renormalize; then * scale."""
import numpy as np
import torch


def to_f64(t) -> np.ndarray:
    """A tensor's values as float64 (exact for fp16 / bf16 / fp32)."""
    return t.detach().cpu().to(torch.float64).numpy()


def sigmoid64(l: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-l))


def keys(logits, scoring="softmax", bias=None) -> np.ndarray:
    """float64 [tokens, E]: what the selection orders by."""
    l = to_f64(logits).reshape(-1, logits.shape[-1])
    if scoring == "sigmoid" and bias is not None:
        return sigmoid64(l) + to_f64(bias)[None, :]
    return l


def select(key: np.ndarray, top_k: int) -> np.ndarray:
    """int64 [tokens, top_k]: the stable arg-sort of the negated key, NaN above +inf."""
    neg = np.where(np.isnan(key), -np.inf, -key)           # NaN first ...
    neg = np.where(np.isinf(key) & (key > 0), -1.7e308, neg)  # ... then +inf (float64 keys of 32-bit inputs never reach 1.7e308)
    neg = neg + 0.0                                         # -0 -> +0
    return np.argsort(neg, axis=-1, kind="stable")[:, :top_k].astype(np.int64)


def topk(logits, top_k, scoring="softmax", renormalize=True, scale=1.0, bias=None):
    """-> (ids int64 [tokens, top_k], weights float64 [tokens, top_k]) of logits [..., E], rows flattened."""
    l = to_f64(logits).reshape(-1, logits.shape[-1])
    ids = select(keys(logits, scoring, bias), top_k)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if scoring == "softmax":
            p = np.exp(l - l.max(axis=-1, keepdims=True))
            sel = np.take_along_axis(p, ids, axis=-1)
            w = sel / (sel.sum(-1, keepdims=True) if renormalize else p.sum(-1, keepdims=True))
        else:
            sel = np.take_along_axis(sigmoid64(l), ids, axis=-1)
            w = sel / sel.sum(-1, keepdims=True) if renormalize else sel
        return ids, w * float(scale)


def exact_pool() -> torch.Tensor:
    """2816 distinct float64 values that fp16, bf16 and fp32 all hold exactly: the bf16 numbers with 2^-7 <= |v| <= 16, ascending."""
    pos = torch.arange(0x3C00, 0x4180, dtype=torch.int32).to(torch.int16).view(torch.bfloat16).to(torch.float64)
    return torch.cat([-pos.flip(0), pos])


def tie_free_logits(T, E, dtype, seed) -> torch.Tensor:
    """[T, E] logits without ties, |l| <= 16: each row a random permutation of E values spread evenly over exact_pool()."""
    g = torch.Generator().manual_seed(seed)
    pool = exact_pool()
    base = pool[torch.linspace(0, pool.numel() - 1, E).round().long()]
    assert base.unique().numel() == E
    return torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)]).to(dtype)


def grid_logits(T, E, dtype, seed, span=8.0) -> torch.Tensor:
    """[T, E] logits, each row a random permutation of the grid (i - E/2) * span / E rounded to `dtype` (distinct in fp16 for E <= 1024)."""
    g = torch.Generator().manual_seed(seed)
    base = ((torch.arange(E, dtype=torch.float64) - E / 2) * span / E).to(dtype)
    return torch.stack([base[torch.randperm(E, generator=g)] for _ in range(T)])


def eighths_bias(E, seed) -> torch.Tensor:
    """float32 [E]: multiples of 1/8 in [-0.5, 0.5]."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (E,), generator=g).to(torch.float32)) / 8
