"""Tables, input builders and gates of tests/test_experts_range_gpu.py, and their self-tests without a GPU.

The experts launches (gemlite_hip_forward_experts, gemlite_hip_forward_experts_fused with the GLU and COMBINE epilogues) are not planned
launches, so none of the sweeps over tests/test_abi_bounds_cpu.py::CASES reaches them.  The GPU module runs them over magnitudes,
non-finite inputs, strides and the corners of their domain with a two-stage reference, and neither stage is taken from the code under test:
  members    the unfused launch, slot by slot, against float64 x @ W.T (+ bias) with W rebuilt from the codes, scales and zeros this
             module generated and KEPT on the CPU (host_experts / w64): test_magnitude_range_gpu.row_gate per slot with the decode
             kernels' tolerance (tol_for);
  epilogues  the fused launch against float64 arithmetic on the unfused launch's rounded outputs, with the bounds derived in
             tests/test_experts_fused_gpu.py: 1 ulp (GLU), 1 ulp + top_k 2^-23 sum |w y| (COMBINE), elementwise.
Everything the GPU module chooses is chosen here from the float64 reference alone: the x scale of the deep-gate token (DEEP), the
amplitudes of the fp16 overflow launches (OVERFLOW), the |y_ref| limits of the magnitude launches, the largest in-expert strides."""
import ctypes as C

import numpy as np
import pytest
import torch

from gemlite_amd import DType, GemLiteExperts, GemLiteLinear, _hip
from tests import test_magnitude_range_gpu as MR
from tests import test_nonfinite_cpu as NF
from tests.test_experts_cpu import query, request
from tests.test_experts_fused_gpu import ROWS, check_combine, check_glu, ulp
from tests.test_gpu_parity import REL_TOL

E = 8
F16, B16 = torch.float16, torch.bfloat16
OUT_CODE = {F16: DType.FP16.value, B16: DType.BF16.value}


def tol_for(dtype):
    """the decode kernels' tolerance by output type (test_magnitude_range_gpu.tol_of: exact unpack, fp32 sums)"""
    return MR.EXACT_TOL if dtype == F16 else REL_TOL[OUT_CODE[dtype]]


# ------------------------------------------------------------------------------------------------ experts whose numbers stay on the CPU
class Host:
    """n experts as generated: q [n, N, K] codes, s [n, N, K / gs] scales in `dtype` (None: W_group_mode 1), z tensor zeros of the same
    shape / one int / None, b [n, N] bias or None; `mode` is the W_group_mode pack() selects for them."""


def host_experts(N, K, gs, dtype, zeros="tensor", bias=False, n=E, seed=0, factor=1.0, scales=True, fma=True):
    g = torch.Generator().manual_seed(seed * 1000 + N + K + gs)
    h = Host()
    h.N, h.K, h.gs, h.dtype, h.n, h.fma = N, K, gs, dtype, n, fma
    h.q = torch.randint(0, 16, (n, N, K), dtype=torch.uint8, generator=g)
    s = (torch.rand(n, N, K // gs, generator=g) * 0.02 + 0.005) * factor
    h.s = s.to(dtype) if scales else None
    z = torch.rand(n, N, K // gs, generator=g) * 4 + 6
    if dtype == F16 and factor < 1:
        z = z.round()  # (test_magnitude_range_gpu.scaled_layer: integer zero points under the small factor)
    h.z = z.to(dtype) if zeros == "tensor" else (8 if zeros == "int" else None)
    h.b = (torch.rand(n, N, generator=g) - 0.5).to(dtype) if bias else None
    if h.s is None:
        assert h.z is not None
        h.mode = 1
    elif h.z is None:
        h.mode = 2
    else:
        h.mode = 4 if (zeros == "tensor" and fma) else 3
    return h


def w64(h, e):
    """float64 W [N, K] of expert e from the codes, scales and zeros as generated (mode 4 folds z' = round(-z s) at pack time)"""
    q = h.q[e].double().numpy()
    up = lambda t: np.repeat(t.double().numpy(), h.gs, axis=1)  # noqa: E731
    z = 0.0 if h.z is None else (float(h.z) if isinstance(h.z, int) else up(h.z[e]))
    if h.mode == 1:
        return q - z
    if h.mode == 2:
        return q * up(h.s[e])
    if h.mode == 3:
        return (q - z) * up(h.s[e])
    zf = (-h.z[e].float() * h.s[e].float()).to(h.dtype)
    return q * up(h.s[e]) + up(zf)


def ref_slots(h, x2, ids, spx):
    """float64 [slots, N]: slot s is expert ids[s] on row s // spx of x2 [rows, K] (a 16-bit tensor), + bias; an invalid id gives zeros"""
    xs = x2.double().cpu().numpy()
    W = {}
    out = np.zeros((len(ids), h.N))
    with np.errstate(invalid="ignore", over="ignore"):
        for s, e in enumerate(ids):
            if 0 <= e < h.n:
                if e not in W:
                    W[e] = w64(h, e)
                out[s] = W[e] @ xs[s // spx] + (0.0 if h.b is None else h.b[e].double().numpy())
    return out


def to_experts(h, device):
    """GemLiteExperts of `h` through GemLiteLinear.pack; gs == K is channel-wise to pack(), so those experts are restacked with the
    grouped modes (W_group_mode 2 / 3 with one K-long group, channel_scale_mode 0) set in the meta args"""
    code = DType.FP16 if h.dtype == F16 else DType.BF16
    layers = []
    for e in range(h.n):
        s = None if h.s is None else h.s[e].reshape(-1, 1).to(device)
        z = h.z if not isinstance(h.z, torch.Tensor) else h.z[e].reshape(-1, 1).to(device)
        b = None if h.b is None else h.b[e].to(device)
        layers.append(GemLiteLinear(4, h.gs, h.K, h.N, code, code).pack(h.q[e].to(device), s, z, b, fma_mode=h.fma))
    if h.gs < h.K or h.s is None:
        ex = GemLiteExperts.from_layers(layers, del_orig=True)
    else:
        assert h.mode in (2, 3) and layers[0].channel_scale_mode == 1
        meta = layers[0].get_meta_args()
        meta[9], meta[10] = 0, h.mode
        stack = lambda name: torch.stack([getattr(l, name).data for l in layers]).contiguous()  # noqa: E731
        zeros = stack("zeros") if layers[0].zeros.numel() > 1 else layers[0].zeros.data
        ex = GemLiteExperts._from_stacked(meta, stack("W_q"), stack("scales"), zeros, None if h.b is None else stack("bias"), h.N, h.K)
    assert ex.get_meta_args()[10] == h.mode and ex.get_meta_args()[9] == 0, ex.get_meta_args()
    return ex


# ------------------------------------------------------------------------------------------------ part 1: magnitudes per slot
SHAPES = [(16, 256), (48, 768), (256, 4352), (32, 4352)]        # N: one tile .. 16 tiles (the pair map); K: 1, 3 and 17 chunks
GLU_SHAPES = [(32, 256), (256, 768), (256, 4352)]               # N % 32 == 0
MAG_IDS = [[5, 2], [2, 7], [0, 5]]                              # the unfused launch and GLU: 6 slots, x per slot
COMBINE_TOP_KS = (3, 16)
SCALE_SHAPE = (256, 768)                                        # all three kernels (GLU: N % 32 == 0)


def glu_scale_slots(dtype, which):
    """the slots of the weight-scale launch that GLU takes: with fp16 scales x 100 the non-zero-mean row has |gate|, |up| up to 1100, and
    silu(gate) up reaches 1.4e5 — fp16 overflow, the subject of OVERFLOW below (test_magnitude_launches_... recomputes the rest)"""
    return [0, 1, 2, 4, 5] if (dtype == F16 and which == "large") else list(range(6))


def combine_ids(top_k, T, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, E, (T, top_k), generator=g)


def combine_weights(T, top_k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.rand(T, top_k, generator=g) + 0.05
    return w / w.sum(-1, keepdim=True)


def profile_x(rows, K, dtype, seed):
    """[len(rows), K]: one profile of test_magnitude_range_gpu per row"""
    rng = np.random.default_rng(seed)
    return torch.from_numpy(np.stack([MR.profile_row(p, K, rng) for p in rows])).to(dtype)


def mag_launches(slots, dtype, profs=None):
    """[launch][slot] -> profile, as test_magnitude_range_gpu.launch_rows deals them"""
    return MR.launch_rows(slots, MR.profiles_for(dtype) if profs is None else profs)


# ------------------------------------------------------------------------------------------------ part 2: deep gates
# Token 0 is N(0, 0.5) scaled until its gate values span +-100 (as the +-60 test of test_experts_fused_gpu.py does); a Gaussian row puts
# next to nothing into [-97, -89], so tokens 1 .. 3 are the "mean" profile (every rowsum of W has the same sign: the zeros sit half a
# code above the codes' mean) scaled until the MEAN gate of their first expert is -91, -93, -95.  All scales come from ref_slots.
DEEP_SHAPE = (256, 4352)
DEEP_ROWS = (0, 1)               # rows of test_experts_fused_gpu.ROWS: fp16 without bias, bf16 with bias
DEEP_IDS = [[5, 2], [2, 7], [7, 0], [0, 5]]
DEEP_MEANS = (-91.0, -93.0, -95.0)
DEEP_WINDOW = (-97.0, -89.0)


def deep_x(h):
    """[4, K] in h.dtype, from the float64 reference alone"""
    K, I = h.K, h.N // 2
    x = torch.cat([(torch.randn(1, K, generator=torch.Generator().manual_seed(4)) * 0.5).to(h.dtype), profile_x(["mean"] * 3, K, h.dtype, 5)])
    first = [row[0] for row in DEEP_IDS]
    bias = np.zeros((4, I)) if h.b is None else np.stack([h.b[e, :I].double().numpy() for e in first])
    lin = ref_slots(h, x, first, 1)[:, :I] - bias  # the part of the gate that scales with x
    x = x.double()
    x[0] *= 104.0 / min(lin[0].max(), -lin[0].min())  # (|bias| <= 0.5)
    for t, m in enumerate(DEEP_MEANS, 1):
        x[t] *= (m - bias[t].mean()) / lin[t].mean()
    return x.to(h.dtype)


def deep_count(gate):
    gate = np.asarray(gate, np.float64)
    return int(((gate >= DEEP_WINDOW[0]) & (gate <= DEEP_WINDOW[1])).sum())


# ------------------------------------------------------------------------------------------------ part 3: non-finite inputs
NONFINITE_SHAPE = (256, 768)  # GLU and COMBINE alike; 6 slots with x per slot
GLU_CLASS = {F16: dict(c=512.0, s_gate=1.0), B16: dict(c=1e35, s_gate=16.0)}


def glu_class_experts(dtype):
    """One hand-made expert, N = 32, K = 256, one scalar zero 8, scales s_gate on the gate half: gate column n has every code 9 (n even:
    W = +s) or 7 (n odd: W = -s), every up column code 8 (W = 0), so with x = c the gate is +-256 c s_gate — beyond the output type —
    and up is the bias alone: 1.5, -2.25, 0 by column mod 3 (so each sign of the gate meets each class of up)."""
    h = host_experts(32, 256, 128, dtype, zeros="int", bias=True, n=1)
    n = torch.arange(32)
    h.q[0] = torch.where(n < 16, torch.where(n % 2 == 0, 9, 7), 8).to(torch.uint8)[:, None].expand(32, 256)
    h.s[0] = torch.where(n < 16, GLU_CLASS[dtype]["s_gate"], 0.015).to(dtype)[:, None].expand(32, 2)
    up = torch.tensor([1.5, -2.25, 0.0])[(n - 16) % 3]
    h.b[0] = torch.where(n < 16, torch.zeros(32), up).to(dtype)
    return h


def glu_class_expected(g, u):
    """float64 g / (1 + exp(-g)) * u with IEEE rules for the non-finite classes: +Inf * u = sign(u) Inf (u = 0: NaN), -Inf / Inf = NaN"""
    with np.errstate(all="ignore"):
        return g / (1.0 + np.exp(-g)) * u


# fp16 outputs around 65504.  A: the amplitude of the N(0, A) x rows; COMBINE sums top_k = 3 members with weights (2, -2, 2) (exact in
# fp16), GLU multiplies two members.  Chosen on the CPU from ref_slots alone: the smallest multiple of 1000 (COMBINE) / of 50 (GLU)
# at which 15 % of every output row lies beyond 65520 (test_overflow_amplitudes_straddle_the_threshold recomputes the shares, and that
# the members themselves stay finite).
OVERFLOW_SHAPE = (256, 768)
OVERFLOW_W = (2.0, -2.0, 2.0)
OVERFLOW = {"combine": 7000.0, "glu": 200.0}
OVERFLOW_TOL = 2.0 ** -11  # the band of overflow_classes: 4 tol = 2^-9, a few fp16 ulps on either side of the threshold


def overflow_x(kind, K):
    g = torch.Generator().manual_seed(31 if kind == "glu" else 32)
    return (torch.randn(2, 3, K, generator=g) * OVERFLOW[kind]).to(F16)


OVERFLOW_IDS = [[5, 2, 6], [1, 7, 0]]


def epilogue_overflow_gate(got, ref, bound):
    """per-row records for an fp16 epilogue output against its float64 reference, classes by NF.overflow_classes: over -> exactly
    +-Inf with the reference's sign, under -> finite and |got - ref| <= bound (the epilogue's own elementwise bound), band -> anything"""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    recs = []
    for m in range(got.shape[0]):
        over, under = NF.overflow_classes(ref[m], OVERFLOW_TOL)
        want = np.where(ref[m] > 0, np.inf, -np.inf)
        with np.errstate(invalid="ignore"):
            bad_over = over & ~(np.isinf(got[m]) & (got[m] == want))
            bad_under = under & ~(np.isfinite(got[m]) & (np.abs(got[m] - ref[m]) <= bound[m]))
        recs.append(dict(row=m, over=int(over.sum()), under=int(under.sum()), over_not_inf=int(bad_over.sum()),
                         under_wrong=int(bad_under.sum()), ok=not bad_over.any() and not bad_under.any()))
    return recs


def glu_f64(y):
    half = y.shape[-1] // 2
    g, u = y[..., :half], y[..., half:]
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g)) * u


# ------------------------------------------------------------------------------------------------ part 6: the in-expert 32-bit edge
EDGE_N, EDGE_K, EDGE_GS = 32, 256, 32  # (N % 32 == 0: GLU runs there too)


def edge_stride_wk(K=EDGE_K):
    """the largest admitted stride_wk (elements, a multiple of 4): rows * stride_wk * 4 < 2^32 with rows = K / 8 packed rows"""
    return ((1 << 32) // (K // 8 * 4) - 1) // 4 * 4


def edge_stride_meta_g(N=EDGE_N, K=EDGE_K, gs=EDGE_GS):
    """the largest admitted stride_meta_g (elements, a multiple of 4): (K / gs) * stride_meta_g * 2 + N * 2 < 2^32"""
    return (((1 << 32) - 2 * N - 1) // (K // gs * 2)) // 4 * 4


# ================================================================================================ self-tests
def test_w64_is_the_layers_own_dequantisation_in_every_mode():
    """The float64 W against the one spelled out per element, and to_experts() on the CPU selects the mode host_experts() names."""
    for kw, mode in ((dict(), 4), (dict(fma=False), 3), (dict(zeros="int"), 3), (dict(zeros="none"), 2), (dict(scales=False), 1),
                     (dict(scales=False, zeros="int"), 1)):
        for dtype in (F16, B16):
            h = host_experts(16, 256, 64, dtype, n=2, bias=True, **kw)
            assert h.mode == mode
            W = w64(h, 1)
            n, k = 5, 130
            q = float(h.q[1, n, k])
            s = 1.0 if h.s is None else float(h.s[1, n, k // 64])
            z = 0.0 if h.z is None else (8.0 if isinstance(h.z, int) else float(h.z[1, n, k // 64]))
            want = q * s + float((-h.z[1, n, k // 64].float() * h.s[1, n, k // 64].float()).to(dtype)) if mode == 4 else (q - z) * s
            assert W[n, k] == want, (kw, dtype)
            ex = to_experts(h, "cpu")
            assert ex.get_meta_args()[10] == mode and ex.num_experts == 2
    h = host_experts(16, 256, 256, F16, zeros="int", n=2)  # one K-long group
    ex = to_experts(h, "cpu")
    assert tuple(ex.scales.shape) == (2, 1, 16) and ex.get_meta_args()[2] == 256 and ex.get_meta_args()[9:11] == [0, 3]
    assert torch.equal(ex.scales[1, 0], h.s[1, :, 0])


def test_ref_slots_reads_the_row_of_each_slot_and_gives_zero_rows_for_invalid_ids():
    h = host_experts(16, 256, 32, B16, bias=True, n=3)
    x = profile_x(["amp1e-1", "amp10"], 256, B16, 0)
    y = ref_slots(h, x, [2, -1, 0, 3], 2)
    assert np.array_equal(y[0], w64(h, 2) @ x[0].double().numpy() + h.b[2].double().numpy())
    assert np.array_equal(y[2], w64(h, 0) @ x[1].double().numpy() + h.b[0].double().numpy())
    assert not y[1].any() and not y[3].any()


def test_the_row_gate_and_the_epilogue_gates_reject_a_wrong_array():
    rng = np.random.default_rng(0)
    y_ref = rng.standard_normal((4, 64))
    y_ref[2] *= 1e-4  # a small row among ordinary ones
    y = torch.from_numpy(y_ref).to(F16)
    assert all(r["ok"] for r in MR.row_gate(y.double().numpy(), y_ref, OUT_CODE[F16], tol_for(F16)))
    wrong = y.double().numpy().copy()
    wrong[2] = 0.0  # the small row came back zero: invisible to a whole-output mean, not to the row gate
    assert [r["ok"] for r in MR.row_gate(wrong, y_ref, OUT_CODE[F16], tol_for(F16))] == [True, True, False, True]
    # GLU: the correctly rounded float64 result passes, the same moved by two ulps in one element does not
    for dtype in (F16, B16):
        yy = (torch.randn(3, 64, generator=torch.Generator().manual_seed(1)) * 3).to(dtype)
        ref = glu_f64(yy.double().numpy())
        out = torch.from_numpy(ref).to(dtype)
        check_glu(out, yy, dtype, "self-test")
        bad = out.clone()
        bad[1, 7] = float(ref[1, 7] + 2.5 * np.sign(ref[1, 7]) * ulp(ref[1, 7], dtype))
        with pytest.raises(AssertionError):
            check_glu(bad, yy, dtype, "self-test, two ulps off")
        # a flushed deep gate: silu(-90) * u is a normal bf16 number and far below fp16's smallest subnormal
        yy[0, 0], yy[0, 32] = -90.0, 50.0
        ref = glu_f64(yy.double().numpy())
        out = torch.from_numpy(ref).to(dtype)
        check_glu(out, yy, dtype, "self-test, deep gate")
        out[0, 0] = 0.0
        if dtype == B16:
            with pytest.raises(AssertionError):
                check_glu(out, yy, dtype, "self-test, deep gate flushed")
        else:
            check_glu(out, yy, dtype, "self-test, deep gate flushed")
        # COMBINE
        y3 = (torch.randn(2, 3, 32, generator=torch.Generator().manual_seed(2))).to(dtype)
        w = combine_weights(2, 3, 0)
        ref = (w.double().numpy()[..., None] * y3.double().numpy()).sum(-2)
        out = torch.from_numpy(ref).to(dtype)
        check_combine(out, y3, w, dtype, "self-test")
        bad = out.clone()
        bad[1, 3] = float(ref[1, 3] + 3.0 * ulp(ref[1, 3], dtype))
        with pytest.raises(AssertionError):
            check_combine(bad, y3, w, dtype, "self-test, off")
        nan = out.clone()
        nan[0, 0] = float("nan")
        with pytest.raises(AssertionError):
            check_combine(nan, y3, w, dtype, "self-test, NaN")


def test_the_epilogue_overflow_gate_accepts_the_cast_and_rejects_a_clamp_and_a_wrong_value():
    rng = np.random.default_rng(3)
    ref = rng.standard_normal((2, 512)) * 60000.0
    with np.errstate(over="ignore"):
        got = ref.astype(np.float32).astype(np.float16).astype(np.float64)
    bound = ulp(ref, F16)
    assert NF.shares_ok(NF.overflow_shares(ref, OVERFLOW_TOL))
    assert all(r["ok"] for r in epilogue_overflow_gate(got, ref, bound))
    recs = epilogue_overflow_gate(np.clip(got, -NF.F16_MAX, NF.F16_MAX), ref, bound)
    assert not any(r["ok"] for r in recs) and all(r["over_not_inf"] == r["over"] for r in recs)
    off = got.copy()
    j = int(np.argmin(np.abs(ref[1])))
    off[1, j] += 3 * bound[1, j]
    assert [r["ok"] for r in epilogue_overflow_gate(off, ref, bound)] == [True, False]
    flipped = got.copy()
    flipped[0, int(np.argmax(ref[0]))] = -np.inf
    assert [r["ok"] for r in epilogue_overflow_gate(flipped, ref, bound)] == [False, True]


def test_isolation_works_on_the_bits_of_a_slot_table():
    clean = np.arange(6 * 16, dtype=np.int16).reshape(6, 16)
    y = clean.copy()
    y[3] = -1
    assert NF.isolation_gate(y, clean, 3) == []
    y[5, 0] ^= 1
    assert NF.isolation_gate(y, clean, 3) == [5]
    assert NF.launches(6) == [(0, "nan"), (3, "inf"), (5, "inf-inf")]


@pytest.mark.parametrize("dtype", [F16, B16], ids=["fp16", "bf16"])
def test_magnitude_launches_hold_every_profile_and_stay_below_the_limit(dtype):
    """|y_ref| < Y_LIMIT for every launch of part 1, from the float64 reference alone (the largest shapes of each kernel)"""
    row = 0 if dtype == F16 else 1
    _, gs, zeros, bias, _ = ROWS[row]
    profs = MR.profiles_for(dtype)
    assert ("subnormal" in profs) == (dtype == F16)
    for (N, K) in (SHAPES[2], SHAPES[0]):
        h = host_experts(N, K, gs, dtype, zeros, bias)
        launches = mag_launches(6, dtype)
        assert {p for l in launches for p in l} == set(profs)
        for li, rows in enumerate(launches):
            y = ref_slots(h, profile_x(rows, K, dtype, 10 + li), [e for r in MAG_IDS for e in r], 1)
            assert np.isfinite(y).all() and float(np.abs(y).max()) < MR.Y_LIMIT, (N, K, li, float(np.abs(y).max()))
    rows, = mag_launches(16, dtype)  # top_k = 16: amplitude 1e-4 and amplitude 10 inside one token, so inside one block
    assert {"amp1e-4", "amp10"} <= set(rows)
    # the weight-scale sweep: its profiles under both factors
    N, K = SCALE_SHAPE
    for which, factor in zip(("small", "large"), MR.scale_factors(dtype)):
        h = host_experts(N, K, gs, dtype, zeros, bias, factor=factor)
        rows, = mag_launches(6, dtype, MR.SCALE_PROFILES)
        y = ref_slots(h, profile_x(rows, K, dtype, 20), [e for r in MAG_IDS for e in r], 1)
        assert float(np.abs(y).max()) < MR.Y_LIMIT, (factor, float(np.abs(y).max()))
        slots = glu_scale_slots(dtype, which)
        assert len(slots) >= 5 and (dtype == B16 or float(np.abs(glu_f64(y[slots])).max()) < NF.F16_MAX / 2)
    if dtype == F16:  # GLU of the profile launches stays inside fp16
        for (N, K) in GLU_SHAPES:
            h = host_experts(N, K, gs, dtype, zeros, bias)
            for li, rows in enumerate(mag_launches(6, dtype)):
                y = ref_slots(h, profile_x(rows, K, dtype, 10 + li), [e for r in MAG_IDS for e in r], 1)
                assert float(np.abs(glu_f64(y)).max()) < NF.F16_MAX / 2


@pytest.mark.parametrize("row", DEEP_ROWS)
def test_deep_gate_inputs_put_sixteen_gates_between_minus_97_and_minus_89(row):
    dtype, gs, zeros, bias, _ = ROWS[row]
    N, K = DEEP_SHAPE
    h = host_experts(N, K, gs, dtype, zeros, bias)
    x = deep_x(h)
    assert bool(torch.isfinite(x).all())
    y = ref_slots(h, x, [e for r in DEEP_IDS for e in r], 2)
    gate = y[:, :N // 2]
    assert deep_count(gate) >= 16, deep_count(gate)
    assert gate[0].max() >= 100 and gate[0].min() <= -100  # token 0, first expert: both ends
    assert float(np.abs(y).max()) < MR.Y_LIMIT
    print(f"deep gates row {row}: {deep_count(gate)} of {gate.size} gate values in [-97, -89], min {gate.min():.1f}, max {gate.max():.1f}")


def test_glu_class_experts_give_infinite_gates_and_the_hand_made_up_values():
    for dtype in (F16, B16):
        h = glu_class_experts(dtype)
        W = w64(h, 0)
        s = GLU_CLASS[dtype]["s_gate"]
        assert np.array_equal(W[:16], np.where(np.arange(16) % 2 == 0, s, -s)[:, None] * np.ones((16, 256))) and not W[16:].any()
        c = GLU_CLASS[dtype]["c"]
        x = torch.full((1, 256), c).to(dtype)
        y = ref_slots(h, x, [0], 1)[0]
        big = 65520.0 if dtype == F16 else float(torch.finfo(B16).max) * (1 + 2.0 ** -9)
        assert (np.abs(y[:16]) > big).all() and np.array_equal(y[16:19], [1.5, -2.25, 0.0])
        inf = np.where(np.arange(16) % 2 == 0, np.inf, -np.inf)
        want = glu_class_expected(inf, y[16:])
        # gate +Inf: sign(u) Inf, NaN where u = 0; gate -Inf: NaN
        assert want[0] == np.inf and want[4] == -np.inf and np.isnan(want[2]) and np.isnan(want[1::2]).all()


def overflow_refs(kind):
    """(float64 member rows [6, N], float64 epilogue rows) of the overflow launch of `kind`, from the reference alone"""
    N, K = OVERFLOW_SHAPE
    dtype, gs, zeros, bias, _ = ROWS[0]
    h = host_experts(N, K, gs, dtype, zeros, bias)
    y = ref_slots(h, overflow_x(kind, K).view(6, K), [e for r in OVERFLOW_IDS for e in r], 1)
    if kind == "glu":
        return y, glu_f64(y)
    return y, (np.asarray(OVERFLOW_W)[None, :, None] * y.reshape(2, 3, N)).sum(1)


@pytest.mark.parametrize("kind", ["combine", "glu"])
def test_overflow_amplitudes_straddle_the_threshold(kind):
    y, ref = overflow_refs(kind)
    assert float(np.abs(y).max()) < NF.F16_MAX * (1 - 4 * tol_for(F16)), float(np.abs(y).max())  # every member stays finite
    shares = NF.overflow_shares(ref, OVERFLOW_TOL)
    print(f"overflow {kind}: (over, under, band) per row {[tuple(round(v, 3) for v in s) for s in shares]}")
    assert NF.shares_ok(shares) and all(over >= 0.15 for over, _, _ in shares), shares


def test_wide_slots_are_finite_and_below_the_wide_limit():
    dtype, gs, zeros, bias, _ = ROWS[1]
    N, K = SHAPES[1]
    h = host_experts(N, K, gs, dtype, zeros, bias)
    x = NF.make_wide_x(NF.WIDE_PROFILES * 2, K, 7)
    y = ref_slots(h, x, [5, 2, 6, 1, 7, 0], 1)
    assert np.isfinite(y).all() and float(np.abs(y).max()) < NF.WIDE_Y_LIMIT


def test_the_query_answers_at_the_in_expert_addressing_edge():
    wk, mg = edge_stride_wk(), edge_stride_meta_g()
    assert wk == (1 << 25) - 4 and mg == (1 << 28) - 8
    assert (EDGE_K // 8) * wk * 4 < 1 << 32 <= (EDGE_K // 8) * (wk + 4) * 4
    assert (EDGE_K // EDGE_GS) * mg * 2 + EDGE_N * 2 < 1 << 32 <= (EDGE_K // EDGE_GS) * (mg + 4) * 2 + EDGE_N * 2
    for field, edge in (("stride_wk", wk), ("stride_meta_g", mg)):
        e = request(EDGE_N, EDGE_K, EDGE_GS, scalar_zero=True)
        setattr(e.layer, field, edge)
        assert query(e) == _hip.OK, field
        setattr(e.layer, field, edge + 4)
        assert query(e) == _hip.ERR_BAD_SHAPE, field
    # the 64-bit strides of part 6 and the slot counts of part 5 are inside the domain
    e = request(EDGE_N, EDGE_K, EDGE_GS)
    e.stride_expert_meta = e.stride_expert_bias = 1 << 32
    e.stride_x_row = e.stride_out_slot = 1 << 31
    e.n_slots, e.slots_per_x_row = 65535, 1 << 40
    assert query(e) == _hip.OK
    e.stride_x_row = 0
    assert query(e) == _hip.OK
    f = _hip.ExpertsFusedArgs()
    f.struct_size = C.sizeof(_hip.ExpertsFusedArgs)
    f.epilogue, f.activation, f.experts = _hip.EXPERTS_COMBINE, _hip.ACT_SILU, e
    f.weights, f.weights_dtype, f.slots_per_token = 0x80000, DType.FP32.value, 16
    f.experts.n_slots = 4095 * 16
    assert _hip.load().gemlite_hip_experts_fused_query(C.byref(f)) == _hip.OK
