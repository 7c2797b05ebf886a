"""Every K order of the unsplit 8-bit tiles, launched and compared bit for bit (`pytest -m gpu`).

The row tiles of a weight column tile of gemm_a8w8_sq_kernel<64x64> / <128x128>, gemm_mx_*_sq_kernel<64x64> and of the narrow 64 x 64 tiles of
gemm_wn_mma_kernel (weight-only 8-bit layers) may walk their K steps in different orders (KOrder, csrc/gl_async.h; `rot` in
gemm_wn_mma_kernel.inc).  tests/test_k_order_cpu.py checks the rule; this module checks its USE: that the prologue and the refill of the LDS
ring, both operands and the block scales map the same step, for every row tile, under both block maps, with fewer steps than stages, fewer
groups than row tiles, runs with a tail and a partial last group.  Each of those slips drops, doubles or mismatches a K step for SOME row
tiles, so the result is compared with a CPU reference in which every K step matters and nothing is rounded twice:

  * int8: random codes; the reference is the exact integer product of the tensors the kernel reads (evaluated in float64: every partial sum
    is an integer below 2^53), times the power-of-two scales, rounded once to the output type.  |sum| < 2^24 is asserted, so the kernel's
    int32 -> fp32 conversion is exact too.  The streaming kernel (tuning[0] = 1) is a second reference.
  * fp8 and block-scaled: elements are small integers (and halves for e2m1) times powers of two, block and channel scales are powers of two,
    and the exponent of a block is a function of (k // 32, row) with period 7 along k — a scale or an operand taken from another K step is
    wrong by a factor of two or more.  The test computes sum |terms| over the smallest unit of any term for every output and asserts it is
    below 2^24: every fp32 partial sum is then exact IN ANY ORDER, and the float64 reference rounded once is the only acceptable result.
    Dynamic layers are fed with the quantiser's own (x_q, scales_x); the reference is built from those tensors.

The kernel is also launched with GEMLITE_TF_NO_K_ROTATION: that run must equal the reference like every other order."""
import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import _hip, helper as H
from gemlite_amd.core import _call_args, _hip_matmul
from gemlite_amd.quant_utils import scale_activations_mxfp4, scale_activations_mxfp8, scale_activations_per_token
from oracle import mx_oracle as MX
from tests.test_k_order_cpu import NO_K_ROTATION, REQUESTS_FIRST, ROUND5_EPILOGUE, kernel_k_steps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KSTEP = kernel_k_steps()
STEPS = (1, 2, 3, 5, 8, 9, 13)
F16, B16 = torch.float16, torch.bfloat16
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
RAN = {}  # spec id -> {(kernel name, order label, mode)}


class Spec:
    def __init__(self, fam, kind, tuning, tdt, name, post=False):
        self.fam, self.kind, self.tuning, self.tdt, self.name, self.post = fam, kind, tuning, tdt, name, post
        self.bm = 128 if fam == "sq128" else 64
        self.id = f"{fam}-{kind}{'-post' if post else ''}-t{tuning[2]}-{str(tdt)[6:]}"
        # two N per kernel: 8 column tiles (the XCD block map) and 3 (the plain one)
        self.ns = (8 * self.bm, 3 * self.bm)
        # mtiles 2, 3, 4, 5, 8 (128-row tiles: 2, 3, 5), every last tile ragged
        self.ms = (129, 300, 577) if fam == "sq128" else (65, 129, 193, 300, 449)
        # K in steps of the kernel's own K step (the 128 x 128 tiles walk 128-byte steps but their planner wants K % 256 == 0: 2 .. 26 steps)
        self.ks = tuple(max(KSTEP[fam], 256) * s for s in STEPS)
        self.dynamic = kind.startswith("mx") and not kind.startswith("mx16")

    def orders(self):
        o = [("plain", NO_K_ROTATION), ("planner", 0)] + [(f"g{g}", g << 24) for g in (1, 2, 3, 4)] + [("g15", 15 << 24)]
        if self.fam == "sq64":
            o += [("requests_first_plain", REQUESTS_FIRST | NO_K_ROTATION), ("requests_first_planner", REQUESTS_FIRST),
                  ("requests_first_g2", REQUESTS_FIRST | (2 << 24))]
        if self.fam == "narrow":
            o += [("round5_epilogue_planner", ROUND5_EPILOGUE), ("round5_epilogue_plain", ROUND5_EPILOGUE | NO_K_ROTATION)]
        return o

    def mode(self, N, M, t3):
        """the order the kernel must report for this launch (the planner's rule at these small shapes, include/gemlite_hip.h)"""
        mtiles = (M + self.bm - 1) // self.bm
        if (t3 & NO_K_ROTATION) or mtiles < 2:
            return -1
        xcd_map = (N // self.bm) % 8 == 0
        g = (t3 >> 24) & 15
        if self.fam == "narrow":
            return 0 if xcd_map else -1
        if g:
            return g
        if self.fam == "sq128":
            return 1 if (self.kind != "int8" and xcd_map) else -1
        return 0 if xcd_map else -1

    def modes_wanted(self):
        if self.fam == "narrow":
            return {-1, 0}
        return {-1, 1, 2, 3, 4, 15} | (set() if self.fam == "sq128" else {0})


SPECS = [Spec("sq64", k, (5, 0, st), (F16, B16, F16)[st - 2], "gemm_a8w8_sq_kernel<64x64>") for k in ("int8", "e4m3", "e5m2") for st in (2, 3, 4)]
SPECS += [Spec("sq128", k, (10, 0, st), (F16, B16)[st - 4], "gemm_a8w8_sq_kernel<128x128>") for k in ("int8", "e4m3", "e5m2") for st in (4, 5)]
SPECS += [Spec("mx_sq", k, (6, 0, st), tdt, f"gemm_mx_a{k[2]}w{k[3]}_sq_kernel<64x64>", post)
          for k, post, st, tdt in (("mx88", False, 4, B16), ("mx88", True, 2, F16), ("mx84", False, 3, F16), ("mx84", True, 4, B16), ("mx44", False, 2, B16))]
SPECS += [Spec("narrow", "a16w8i", (2, 1, 32), F16, "gemm_a16w8_kernel<64x64>"), Spec("narrow", "a16w8f", (2, 1, 32), B16, "gemm_a16w8_kernel<64x64>"),
          Spec("narrow", "mx16w8", (2, 1, 32), F16, "gemm_a16w8_mxfp_kernel<64x64>")]


# ---------------------------------------------------------------------------------------------------- data (CPU, deterministic)
def _ints(R, K, seed, lo, hi):
    return torch.randint(lo, hi + 1, (R, K), generator=torch.Generator().manual_seed(seed), dtype=torch.int32)


def _block_exps(R, K, a, b, period=7):
    """[R, K / 32] exponents 0 .. period - 1: blocks 4 or 8 apart (one K step) differ unless they are a multiple of `period` steps apart"""
    kb, r = torch.arange(K // 32).view(1, -1), torch.arange(R).view(-1, 1)
    return (kb * a + r * b) % period


E2M1 = torch.tensor([0, 0.5, 1, 1.5, 2, 3, 4, 6, -0.0, -0.5, -1, -1.5, -2, -3, -4, -6])
E2M1_DRAW = torch.tensor([0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13], dtype=torch.uint8)  # 0, +-0.5 .. +-3


def _pow2(e):
    return torch.exp2(e.double())


class Data:
    """master weights [N_max, K_max] and activations [M_max, K_max] of one spec; every shape of the spec is a corner of them"""

    def __init__(self, s, seed):
        self.s = s
        N, M, K = max(s.ns), max(s.ms), max(s.ks)
        n, m = torch.arange(N), torch.arange(M)
        we = _block_exps(N, K, 3, 5).repeat_interleave(32, 1)
        xe = _block_exps(M, K, 5, 3).repeat_interleave(32, 1)
        self.sw = _pow2((n % 4) - 10).view(-1, 1)   # channel scales (where the layer has them)
        self.sx = _pow2((m % 3) - 2).view(-1, 1)    # token scales (where the test passes them)
        k = s.kind
        if k == "int8":
            self.w = _ints(N, K, seed, -127, 127).to(torch.int8)
            self.x = _ints(M, K, seed + 1, -127, 127).to(torch.int8)
        elif k in FP8:
            self.w = (_ints(N, K, seed, -3, 3).double() * _pow2(we)).float().to(FP8[k])
            self.x = (_ints(M, K, seed + 1, -3, 3).double() * _pow2(xe)).float().to(FP8[k])
        else:
            if k == "a16w8i":
                self.w = (_ints(N, K, seed, -3, 3) * (1 << (we % 6))).to(torch.int8)
            elif k == "a16w8f":
                self.w = (_ints(N, K, seed, -3, 3).double() * _pow2(we)).float().to(torch.float8_e4m3fn)
            else:  # block-scaled weights: small integers (e2m1: and halves) with the exponent in the e8m0 block scale
                self.w_scales = ((118 if s.post else 124) + _block_exps(N, K, 3, 5)).to(torch.uint8)
                if k[3] == "8" or k == "mx16w8":
                    self.w = _ints(N, K, seed, -3, 3).float().to(torch.float8_e4m3fn)
                else:
                    self.w = E2M1_DRAW[torch.randint(0, len(E2M1_DRAW), (N, K), generator=torch.Generator().manual_seed(seed))]
            # (one fp32 scale per token: the elements keep their exponents inside e4m3, so the unit is 1 and the weights' scales are lower instead)
            x = _ints(M, K, seed + 1, -3, 3).double() * _pow2(xe - (0 if s.post else 6))
            if s.post:  # amax = 448 * 2^j makes the token scale the power of two 2^j, j = 0 / 1 by row
                x[m, (m * 7) % 256] = 448.0 * _pow2(m % 2)
            self.x = x.float().to(s.tdt)
            assert torch.equal(self.x.double(), x)

    def layer(self, N, K):
        s, k = self.s, self.s.kind
        w = self.w[:N, :K].contiguous().to(DEV)
        if k == "int8":
            return H.A8W8_int8_dynamic(device=DEV, dtype=s.tdt).from_weights(w, scales=self.sw[:N].float().to(DEV))
        if k in FP8:
            return H.A8W8_dynamic(device=DEV, dtype=s.tdt, fp8=FP8[k]).from_weights(w, scales=self.sw[:N].float().to(DEV))
        if k == "a16w8i":
            return H.A16W8(device=DEV, dtype=s.tdt).from_weights(w, scales=self.sw[:N].to(s.tdt).to(DEV))
        if k == "a16w8f":
            return H.A16W8_FP8(device=DEV, dtype=s.tdt).from_weights(w, scales=self.sw[:N].to(s.tdt).to(DEV))
        sc = self.w_scales[:N, :K // 32].contiguous().to(DEV)
        if k == "mx16w8":
            return H.A16W8_MXFP(device=DEV, dtype=s.tdt).from_weights(w, sc)
        if k == "mx44":
            return H.A4W4_MXFP_dynamic(device=DEV, dtype=s.tdt).from_weights(w, scales=sc)
        return H.A8Wn_MXFP_dynamic(device=DEV, dtype=s.tdt, post_scale=s.post, W_nbits=int(k[3])).from_weights(w, scales=sc)

    def feed(self, M, K):
        """(x as the kernel reads it, scales_x or None) on the device"""
        s, x = self.s, self.x[:M, :K].contiguous().to(DEV)
        if s.kind == "int8" or s.kind in FP8:
            return x, self.sx[:M].float().to(DEV)
        if not s.dynamic:
            return x, None
        if s.post:
            return scale_activations_per_token(x, w_dtype=torch.float8_e4m3fn)
        return (scale_activations_mxfp4 if s.kind == "mx44" else scale_activations_mxfp8)(x)


def _bytes(t):
    return t.contiguous().view(torch.uint8).cpu().numpy()


def weights_f64(s, lin):
    """([N, K] float64 values of the tensors the kernel reads, [N] channel scales)"""
    N = lin.out_features
    if s.kind.startswith("mx"):
        from tests.test_mx_gpu import _weights_nk
        wv, ws = _weights_nk(lin)
        return wv.astype(np.float64) * np.repeat(MX.e8m0_decode(ws), 32, axis=1), np.ones(N)
    return lin.W_q.data.t().double().cpu().numpy(), lin.scales.data.double().cpu().numpy().reshape(-1)


def acts_f64(s, xq, sx, M, K):
    """([M, K] float64 values of the activations the kernel reads, block scales applied; [M] token scales)"""
    if not s.dynamic:
        return xq.double().cpu().numpy(), (np.ones(M) if sx is None else sx.double().cpu().numpy().reshape(-1))
    if s.post:
        return MX.fp8_e4m3_decode(_bytes(xq)).astype(np.float64), sx.double().cpu().numpy().reshape(-1)
    xv = MX.fp4_unpack(_bytes(xq)) if s.kind == "mx44" else MX.fp8_e4m3_decode(_bytes(xq))
    return xv.astype(np.float64) * np.repeat(MX.e8m0_decode(_bytes(sx)[:M]), 32, axis=1), np.ones(M)


def _unit(a):
    """per row: the smallest power of two any non-zero element of the row is a multiple of (elements are multiples of 2^-40)"""
    i = np.rint(np.abs(a) * 2.0 ** 40).astype(np.int64)
    assert np.array_equal(i.astype(np.float64) * 2.0 ** -40, np.abs(a))
    low = (i & -i).astype(np.float64)
    low[i == 0] = np.inf
    return low.min(axis=1) * 2.0 ** -40


def assert_order_proof(tag, X, W):
    """sum |terms| / (smallest unit of a term) < 2^24 for every output: every fp32 partial sum of the terms is exact in any order"""
    load = (np.abs(X) @ np.abs(W).T) / (_unit(X).reshape(-1, 1) * _unit(W).reshape(1, -1))
    assert float(load.max()) < 2.0 ** 24, (tag, float(load.max()) / 2.0 ** 24)


def reference(s, X, sx, W, sw):
    acc = X @ W.T  # float64: exact (integers of some unit below 2^53)
    if s.kind == "int8":
        assert float(np.abs(acc).max()) < 2.0 ** 24  # the int32 sum converts to fp32 exactly
    y = torch.from_numpy(acc * sx.reshape(-1, 1) * sw.reshape(1, -1))
    y32 = y.float()
    assert torch.equal(y32.double(), y) and bool(torch.isfinite(y32).all())  # powers of two: nothing rounded so far
    out = y32.to(s.tdt)                                                      # ... the ONE rounding
    assert bool(torch.isfinite(out).all())
    return out


def _query(lin, x, sx, tuning):
    a = _call_args(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, tuning, False, 0x1000, (lin.out_features, 1))
    lib = _hip.load()
    return lib.gemlite_hip_kernel_name(_hip.C.byref(a)).decode(), lib.gemlite_hip_k_order_mode(_hip.C.byref(a))


def _strided(x):
    wide = torch.zeros(x.shape[0], x.shape[1] + 64, dtype=torch.uint8, device=x.device).view(x.dtype) if x.dtype == torch.uint8 else \
        torch.zeros(x.shape[0], x.shape[1] + 64, dtype=x.dtype, device=x.device)
    wide[:, :x.shape[1]] = x
    return wide[:, :x.shape[1]]


# ---------------------------------------------------------------------------------------------------- every order, bit for bit
@pytest.mark.parametrize("s", SPECS, ids=[s.id for s in SPECS])
def test_every_k_order_equals_the_exact_reference(s):
    d = Data(s, seed=1000 + SPECS.index(s))
    ran = RAN.setdefault(s.id, set())
    bad = []
    for N in s.ns:
        for K in s.ks:
            lin = d.layer(N, K)
            W, sw = weights_f64(s, lin)
            for M in (s.ms if N == s.ns[0] else s.ms[1:3]):
                x, sx = d.feed(M, K)
                X, sxv = acts_f64(s, x, sx, M, K)
                if s.kind != "int8" and (N, K, M) == (max(s.ns), max(s.ks), max(s.ms)):
                    assert_order_proof(s.id, X, W)  # (every other shape is a corner of this one: fewer terms, no smaller unit)
                    if s.dynamic:  # the quantiser kept the data exact
                        assert np.array_equal(X * sxv.reshape(-1, 1), d.x[:M, :K].double().numpy()), s.id
                ref = reference(s, X, sxv, W, sw).to(DEV)
                outs, labels = [], []
                for label, t3 in s.orders():
                    tuning = s.tuning + (t3,)
                    name, mode = _query(lin, x, sx, tuning)
                    assert name == s.name and mode == s.mode(N, M, t3), (s.id, N, K, M, label, name, mode)
                    outs.append(_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, tuning))
                    labels.append(label)
                    ran.add((name, label, mode))
                if (N, K, M) == (s.ns[0], s.ks[3], 300):  # strided activations, once per kernel
                    outs.append(_hip_matmul(_strided(x), lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, s.tuning + (2 << 24,)))
                    labels.append("g2_strided_x")
                if s.kind == "int8":  # the second reference
                    assert _query(lin, x, sx, (1, 0, 0, 0))[0] == "kmajor_matmul_kernel"
                    outs.append(_hip_matmul(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, (1, 0, 0, 0)))
                    labels.append("streaming")
                Y = torch.stack(outs)
                wrong = (Y != ref.unsqueeze(0)) | ~torch.isfinite(Y)
                if bool(wrong.any()):
                    for i in wrong.flatten(1).any(1).nonzero().flatten().tolist():
                        rows = wrong[i].any(1).nonzero().flatten()
                        cols = wrong[i].any(0).nonzero().flatten()
                        bad.append(f"N={N} K={K} ({K // KSTEP[s.fam]} steps) M={M} {labels[i]}: {int(wrong[i].sum())} wrong outputs, row tiles "
                                   f"{sorted(set((rows // s.bm).tolist()))}, column tiles {sorted(set((cols // s.bm).tolist()))[:8]}")
    assert not bad, f"{s.id}: {len(bad)} launches differ from the exact reference:\n" + "\n".join(bad[:40])
    # every order ran on this kernel, in every mode it can report
    assert {l for _, l, _ in ran} == {l for l, _ in s.orders()} and {m for _, _, m in ran} == s.modes_wanted(), (s.id, sorted(ran))
    assert {n for n, _, _ in ran} == {s.name}


# ---------------------------------------------------------------------------------------------------- random data at the parity gates
RANDOM = [(s.fam, s.kind, s.post, s.tuning[:2], s.name) for s in SPECS]
RANDOM = sorted(set(RANDOM))


@pytest.mark.parametrize("tdt", [F16, B16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("fam,kind,post,t01,name", RANDOM, ids=[f"{r[0]}-{r[1]}{'-post' if r[2] else ''}" for r in RANDOM])
def test_forced_groups_on_random_data_against_the_oracle(fam, kind, post, t01, name, tdt):
    """one random-data case per kernel and forced group against the float64 oracle at the gates of DESIGN §4 (ragged row tiles, a tail of groups)"""
    from tests.test_gpu_parity import _compare, _oracle_from_layer
    from tests.test_mx_gpu import _check, _oracle
    bm = 128 if fam == "sq128" else 64
    N, K, M = 8 * bm, 9 * 256, 300
    g = torch.Generator().manual_seed(len(kind) * 7 + bm)
    W = (torch.randn(N, K, generator=g) / 30).to(tdt)
    W[:, :64] *= 8  # blocks with very different scales
    x = (torch.randn(M, K, generator=g) / 4).to(tdt).to(DEV)
    C = gemlite_amd.core
    code = gemlite_amd.dtypes.TORCH_TO_DTYPE[tdt].value
    for grp in (1, 2, 3, 4):
        tuning = t01 + ({"sq64": 4, "sq128": 4, "mx_sq": 4, "narrow": 32}[fam], grp << 24)
        want = 0 if fam == "narrow" else grp
        if kind.startswith("mx"):
            proc = {"mx16w8": lambda: H.A16W8_MXFP(device=DEV, dtype=tdt), "mx44": lambda: H.A4W4_MXFP_dynamic(device=DEV, dtype=tdt)}.get(
                kind, lambda: H.A8Wn_MXFP_dynamic(device=DEV, dtype=tdt, post_scale=post, W_nbits=int(kind[3])))()
            lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=tdt)
            lin.weight.data = W.to(DEV)
            layer = proc.from_linear(lin, del_orig=False)
            ref = _oracle(layer, x)
            C.TUNING_OVERRIDE = tuning
            try:
                y = layer(x)
            finally:
                C.TUNING_OVERRIDE = None
            if kind == "mx16w8":
                xq, sx = x, None
            elif post:
                xq, sx = scale_activations_per_token(x, w_dtype=torch.float8_e4m3fn)
            else:
                xq, sx = (scale_activations_mxfp4 if kind == "mx44" else scale_activations_mxfp8)(x)
            assert _query(layer, xq, sx, tuning) == (name, want), (kind, grp, _query(layer, xq, sx, tuning))
            _check(f"k-order random {kind} post={post} g{grp} {tdt}", y, ref, tdt)
        elif kind.startswith("a16"):
            layer = (H.A16W8 if kind == "a16w8i" else H.A16W8_FP8)(device=DEV, dtype=tdt).from_weights(W)
            assert _query(layer, x, None, tuning) == (name, want)
            y = _hip_matmul(x, layer.W_q, layer.scales, layer.zeros, None, layer.get_meta_args(), -1, tuning)
            _compare(f"k-order random {kind} g{grp} {tdt}", y, _oracle_from_layer(layer, x), code)
        else:
            qdt = torch.int8 if kind == "int8" else FP8[kind]
            proc = H.A8W8_int8_dynamic(device=DEV, dtype=tdt) if kind == "int8" else H.A8W8_dynamic(device=DEV, dtype=tdt, fp8=qdt)
            layer = proc.from_weights(W)
            xq, sx = scale_activations_per_token(x, qdt)
            assert _query(layer, xq, sx, tuning) == (name, want)
            y = _hip_matmul(xq, layer.W_q, layer.scales, layer.zeros, sx, layer.get_meta_args(), -1, tuning)
            y_or = (xq.double().cpu().numpy() @ layer.W_q.data.double().cpu().numpy()) * (
                sx.double().cpu().numpy() * layer.scales.data.double().cpu().numpy().reshape(1, -1))
            _compare(f"k-order random {kind} g{grp} {tdt}", y, y_or, code, abs_gate=5e-3 if kind != "int8" else 1e-3)


# ---------------------------------------------------------------------------------------------------- one-hot: names the wrong k rows
ONE_HOT = [("sq64", "int8"), ("sq64", "fp8"), ("sq128", "int8"), ("sq128", "fp8"), ("mx_sq", "A8W8_MXFP_dynamic"), ("mx_sq", "A8W4_MXFP_dynamic"),
           ("mx_sq", "A4W4_MXFP_dynamic"), ("narrow", "int8"), ("narrow", "fp8"), ("narrow", "A16W8_MXFP")]


@pytest.mark.parametrize("fam,kind", ONE_HOT, ids=[f"{f}-{k}" for f, k in ONE_HOT])
def test_one_hot_sweep_under_forced_groups_of_two_steps_with_three_row_tiles(fam, kind):
    """the one-hot sweep of tests/test_structured_exact_gpu.py (every k hot once, outputs = the dequantised matrix) with three row tiles under
    groups of two steps (the narrow tiles: under their rotation): a full run, a tail group and a lone last step (64-row tiles; 128-row: three
    full runs).  Its failure message names the k rows that went wrong."""
    from tests import test_structured_exact_gpu as SE
    bm = 128 if fam == "sq128" else 64
    N, K, M = 8 * bm, 9 * 256, (300 if bm == 128 else 160)
    tdt = B16
    tuning = {"sq64": (5, 0, 3, 2 << 24), "sq128": (10, 0, 5, 2 << 24), "mx_sq": (6, 0, 3, 2 << 24), "narrow": (2, 1, 32, 0)}[fam]
    want = 0 if fam == "narrow" else 2
    C = gemlite_amd.core
    if kind in ("int8", "fp8") and fam != "narrow":
        lin, E = SE._coded_a8w8(N, K, kind, tdt)
        qdt = torch.int8 if kind == "int8" else torch.float8_e4m3fn
        sx = torch.ones(M, 1, dtype=torch.float32, device=DEV)
        assert _query(lin, torch.empty(M, K, dtype=qdt, device=DEV), sx, tuning)[1] == want
        Y = SE._sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, sx, lin.get_meta_args(), -1, tuning), M, K, qdt)
        SE._exact(f"k-order one-hot {fam} {kind}", Y, E.to(tdt).float())
        return
    if kind in ("int8", "fp8"):
        k, n = torch.arange(K).view(1, K), torch.arange(N).view(N, 1)
        sc = torch.pow(2.0, ((n % 4) - 2).float())
        if kind == "int8":
            Wq = (((k * 3 + n * 5 + (k >> 6)) % 255) - 127).to(torch.int8)
            lin = H.A16W8(device=DEV, dtype=tdt).from_weights(Wq.to(DEV), scales=sc.to(tdt).to(DEV))
        else:
            b = ((k * 3 + n * 5 + (k >> 6)) % 256).to(torch.uint8)
            b[(b & 0x7F) == 0x7F] = 0x3A
            Wq = b.view(torch.float8_e4m3fn)
            lin = H.A16W8_FP8(device=DEV, dtype=tdt).from_weights(Wq.to(DEV), scales=sc.to(tdt).to(DEV))
        E = (Wq.float() * sc).t().contiguous().to(tdt).float()
        assert _query(lin, torch.empty(M, K, dtype=tdt, device=DEV), None, tuning) == ("gemm_a16w8_kernel<64x64>", want)
        Y = SE._sweep(lambda x: _hip_matmul(x, lin.W_q, lin.scales, lin.zeros, None, lin.get_meta_args(), -1, tuning), M, K, tdt)
        SE._exact(f"k-order one-hot narrow {kind}", Y, E)
        return
    from tests.test_mx_gpu import _kernel_name, _weights_nk
    g = torch.Generator().manual_seed(11)
    W = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-3, 4, (N, 1), generator=g).float())
    lin = torch.nn.Linear(K, N, bias=False, device=DEV, dtype=tdt)
    lin.weight.data = W.to(tdt).to(DEV)
    lin.weight.requires_grad = False
    kw = dict(post_scale=False) if kind.startswith("A8W") else {}
    layer = getattr(H, kind)(device=DEV, dtype=tdt, **kw).from_linear(lin, del_orig=False)
    wv, ws = _weights_nk(layer)
    E = torch.from_numpy((wv.astype(np.float64) * np.repeat(np.exp2(ws.astype(np.float64) - 127.0), 32, axis=1)).astype(np.float32)).t().contiguous()
    assert torch.equal(E.to(tdt).float(), E)
    name = _kernel_name(layer, torch.empty(M, K), tuning)
    assert ("_sq_kernel<64x64>" in name) if fam == "mx_sq" else (name == "gemm_a16w8_mxfp_kernel<64x64>"), name
    C.TUNING_OVERRIDE = tuning
    try:
        Y = SE._sweep(lambda x: layer(x), M, K, tdt)
    finally:
        C.TUNING_OVERRIDE = None
    SE._exact(f"k-order one-hot {fam} {kind}", Y, E)


def test_every_kernel_and_order_pair_ran():
    """runs last in this module: of the kernels whose sweep ran in this process, every (kernel, order) pair was launched"""
    for s in SPECS:
        if s.id in RAN:
            assert {l for _, l, _ in RAN[s.id]} == {l for l, _ in s.orders()}, (s.id, sorted(RAN[s.id]))
            assert {m for _, _, m in RAN[s.id]} == s.modes_wanted(), (s.id, sorted(RAN[s.id]))
