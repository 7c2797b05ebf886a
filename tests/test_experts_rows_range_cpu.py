"""Builders, tables and bookkeeping of tests/test_experts_rows_range_gpu.py, and their self-tests without a GPU.

gemlite_hip_experts_route / gemlite_hip_forward_experts_rows admit 4096 experts and 65535 slots; tests/test_experts_rows_gpu.py runs 8
experts and at most 280 slots.  The GPU module runs the two launches where their loops take a second pass, where the prefix sum of the
route crosses waves, where a 64-bit base or a 32-bit offset sits at its edge, and over the gather's own layouts.  Everything it chooses is
chosen here:
  big_stack        E experts that all differ, synthesised as stacked tensors (GemLiteLinear.pack 4096 times is too slow);
  id patterns      PATTERNS / random_ids, each with a self-test that it is what its name says and that it stays inside Bmax;
  chunks_of        the slots of every bucket in chunks of R with ONE stable argsort (the oracle of the GPU module walks these; the
                   list version of tests/test_experts_rows_gpu.py::oracle_rows is O(E n) in Python), fast_table: a right table from them;
  rows edges       the largest stride_wk / stride_meta_g experts_rows_plan admits, pinned with gemlite_hip_experts_rows_query."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

from gemlite_amd import DType, GemLiteExperts, GemLiteLinear, _hip, experts as X
from tests.test_experts_range_cpu import EDGE_GS, EDGE_K, edge_stride_meta_g, edge_stride_wk
from tests.test_experts_rows_cpu import HEADER, blocks_max, blocks_used, buckets_of, check_table, make_table, query, rows_request

F16, B16 = torch.float16, torch.bfloat16
HIGH = (1 << 32) + 1                               # an int64 id whose low dword is a valid expert
ROUTE_THREADS, ROUTE_PER_THREAD, WAVE0 = 1024, 5, 320  # experts_route.hip: thread t owns buckets 5 t .. 5 t + 4, wave 0 the first 320
SCALE_E = (128, 319, 320, 1023, 1024, 4096)        # 319: wave 0 exactly full; 320: the invalid bucket alone in wave 1; 1023 / 1024: either
                                                   # side of the second pass of the per-bucket loops (E + 1 > 1024); 4096: the maximum
SCALE_R = (16, 64)
RANDOM_N = (1023, 1024, 1025, 4097, 65535)         # around one pass of the slot loops, several passes, the maximum
SMALL = dict(N=16, K=256, gs=64)                   # the stack of parts 1 and 2: 4096 experts take 8 MB


# ------------------------------------------------------------------------------------------------ a stack of many experts
def big_stack(E, N, K, gs, dtype, zeros="tensor", bias=False, seed=0, device="cpu"):
    """GemLiteExperts of E experts that all differ: ONE layer packed the usual way gives the metadata and the trailing shapes and dtypes,
    the stacked tensors are synthesised — W_q [E, K / 8, N] uniformly random int32 words (every word is a valid packing of eight 4-bit
    codes), scales in [0.005, 0.025) and zero points in [6, 10) as tests/test_experts_gpu.py::make_experts has them (W_group_mode 4 holds
    -z s, as pack() folds it), a random bias."""
    g = torch.Generator().manual_seed(seed * 1000 + E + N + K + gs)
    dt = DType.FP16 if dtype == F16 else DType.BF16
    lin = GemLiteLinear(4, gs, K, N, dt, dt).pack(
        torch.randint(0, 16, (N, K), dtype=torch.uint8, generator=g), (torch.rand(N * K // gs, 1, generator=g) * 0.02 + 0.005).to(dtype),
        (torch.rand(N * K // gs, 1, generator=g) * 4 + 6).to(dtype) if zeros == "tensor" else 8,
        (torch.rand(N, generator=g) - 0.5).to(dtype) if bias else None)
    meta = lin.get_meta_args()
    assert tuple(lin.W_q.shape) == (K // 8, N) and lin.W_q.dtype == torch.int32 and tuple(lin.scales.shape) == (K // gs, N)
    W_q = torch.randint(-(1 << 31), 1 << 31, (E,) + tuple(lin.W_q.shape), dtype=torch.int64, generator=g).to(torch.int32)
    s = torch.rand((E,) + tuple(lin.scales.shape), generator=g) * 0.02 + 0.005
    if lin.zeros.numel() > 1:
        assert lin.zeros.shape == lin.scales.shape and lin.zeros.dtype == dtype and meta[10] in (3, 4)
        z = torch.rand((E,) + tuple(lin.zeros.shape), generator=g) * 4 + 6
        z = (-z.to(dtype).float() * s.to(dtype).float()).to(dtype) if meta[10] == 4 else z.to(dtype)
    else:
        z = lin.zeros.data
    b = (torch.rand(E, N, generator=g) - 0.5).to(dtype) if bias else None
    return GemLiteExperts._from_stacked(meta, W_q.to(device), s.to(dtype).to(device), z.to(device), None if b is None else b.to(device), N, K)


# ------------------------------------------------------------------------------------------------ id patterns (flat int64 arrays)
def invalid_ids(n, E, ids64):
    """n ids outside [0, E): -1, E and, for int64, one with a high dword whose low dword is a valid expert"""
    kinds = [-1, E] + ([HIGH] if ids64 else [])
    return np.array([kinds[i % len(kinds)] for i in range(n)], dtype=np.int64)


def every_bucket_once(E, R, ids64, rng):
    return rng.permutation(np.concatenate((np.arange(E), invalid_ids(1, E, ids64))))  # n = E + 1: the most blocks per slot


def all_on_the_last_expert(E, R, ids64, rng):
    return np.full(ROUTE_THREADS + 2 * R + 1, E - 1, dtype=np.int64)  # (two passes of the slot loops onto one counter)


def all_invalid(E, R, ids64, rng):
    return invalid_ids(ROUTE_THREADS + 76, E, ids64)


def _counted(experts, rng):
    """each of `experts` 1 + e % 3 times, shuffled"""
    return rng.permutation(np.repeat(experts, 1 + experts % 3))


def only_beyond_wave_0(E, R, ids64, rng):
    """experts >= 320 only: first[] of every later wave sums earlier waves that hold nothing"""
    return _counted(np.arange(WAVE0, E), rng)


def only_wave_0(E, R, ids64, rng):
    """the complement: the earlier waves own every populated bucket — and the invalid bucket, in the last populated wave, sums them all"""
    return np.concatenate((_counted(np.arange(min(WAVE0, E)), rng), invalid_ids(3, E, ids64)))


def exact_multiples(E, R, ids64, rng):
    """at most 300 experts spread over [0, E), the last one among them, R or 2 R slots each: no padding row anywhere"""
    experts = np.unique(np.linspace(0, E - 1, min(E, 300)).astype(np.int64))
    return rng.permutation(np.repeat(experts, R * (1 + np.arange(len(experts)) % 2)))


PATTERNS = {"every bucket once": every_bucket_once, "all on the last expert": all_on_the_last_expert, "all invalid": all_invalid,
            "only experts >= 320": only_beyond_wave_0, "only experts < 320": only_wave_0, "exact multiples of R": exact_multiples}


def patterns_for(E, R, ids64, seed=0):
    """name -> flat ids; the pattern beyond wave 0 exists where there is an expert there"""
    rng = np.random.default_rng(seed + E + R)
    return {name: f(E, R, ids64, rng) for name, f in PATTERNS.items() if name != "only experts >= 320" or E > WAVE0}


def random_ids(E, n, ids64, seed=0):
    """uniformly random ids, every 7th one invalid (the flat ids of a top_k = 8 router; n need not be a multiple of 8)"""
    ids = np.random.default_rng(seed + E + n).integers(0, E, n)
    bad = np.arange(n) % 7 == 3
    ids[bad] = invalid_ids(int(bad.sum()), E, ids64)
    return ids


def ids_tensor(ids, dtype, device):
    return torch.from_numpy(np.asarray(ids, dtype=np.int64)).to(dtype).to(device)


# ------------------------------------------------------------------------------------------------ the slots of every bucket, in chunks of R
def chunks_of(ids, E, R):
    """[(bucket, slots)] in ascending bucket order, the slots of a bucket ascending in chunks of at most R: ONE stable argsort"""
    b = buckets_of(ids, E)
    order = np.argsort(b, kind="stable")
    counts = np.bincount(b, minlength=E + 1)
    ends = np.cumsum(counts)
    out = []
    for e in np.nonzero(counts)[0]:
        lo, hi = int(ends[e] - counts[e]), int(ends[e])
        out.extend((int(e), order[i:min(i + R, hi)]) for i in range(lo, hi, R))
    return out


def chunks_of_slow(ids, E, R):
    """the same by the list comprehension of tests/test_experts_rows_gpu.py::oracle_rows"""
    flat = buckets_of(ids, E).tolist()
    out = []
    for e in range(E + 1):
        slots = [s for s, v in enumerate(flat) if v == e]
        out.extend((e, slots[i:i + R]) for i in range(0, len(slots), R))
    return out


def fast_table(ids, E, R):
    """tests/test_experts_rows_cpu.py::make_table from chunks_of (make_table itself is O(E n) in Python)"""
    n, bmax = len(ids), blocks_max(len(ids), E, R)
    table = np.full(HEADER + bmax + bmax * R, -7, dtype=np.int64)
    table[:HEADER] = 0
    chunks = chunks_of(ids, E, R)
    for blk, (e, slots) in enumerate(chunks):
        table[HEADER + blk] = e
        row = table[HEADER + bmax + blk * R:HEADER + bmax + (blk + 1) * R]
        row[:] = -1
        row[:len(slots)] = slots
    table[0] = len(chunks)
    assert n >= 1
    return table


# ------------------------------------------------------------------------------------------------ the rows launch's in-expert 32-bit edges
ROWS_EDGE_N, ROWS_EDGE_K, ROWS_EDGE_GS = 256, EDGE_K, EDGE_GS  # N > K / 2: the row the extent ends in moves the edge of stride_wk


def rows_edge_stride_wk(N=ROWS_EDGE_N, K=ROWS_EDGE_K):
    """the largest stride_wk (elements, a multiple of 4) experts_rows_plan admits: the rows kernel counts the row the extent ends in,
    K / 8 * stride_wk * 4 + N * 4 < 2^32 (experts_plan alone stops at edge_stride_wk(): K / 8 * stride_wk * 4 < 2^32)"""
    return (((1 << 32) - 4 * N - 1) // (K // 8 * 4)) // 4 * 4


def rows_edge_stride_meta_g(N=ROWS_EDGE_N, K=ROWS_EDGE_K, gs=ROWS_EDGE_GS):
    """the rows rule for the metadata is experts_plan's: (K / gs * stride_meta_g + N) * 2 < 2^32"""
    return edge_stride_meta_g(N, K, gs)


# ================================================================================================ self-tests
STACKS = [(4096, F16, "tensor", True), (1024, B16, "tensor", False), (320, F16, "int", True), (128, B16, "int", False)]


@pytest.mark.parametrize("E,dtype,zeros,bias", STACKS, ids=[f"E{s[0]}-{str(s[1])[6:]}-z{s[2]}-b{int(s[3])}" for s in STACKS])
def test_big_stack_is_inside_the_domain_views_its_slices_and_no_two_experts_are_alike(E, dtype, zeros, bias):
    ex = big_stack(E, dtype=dtype, zeros=zeros, bias=bias, **SMALL)  # (_from_stacked runs _check_domain: a refusal raises here)
    N, K, gs = SMALL["N"], SMALL["K"], SMALL["gs"]
    assert ex.num_experts == E and (ex.out_features, ex.in_features) == (N, K)
    assert tuple(ex.W_q.shape) == (E, K // 8, N) and tuple(ex.scales.shape) == (E, K // gs, N) and ex.scales.dtype == dtype
    assert (ex.bias is not None) == bias and ex.zeros.numel() == (E * (K // gs) * N if zeros == "tensor" else 1)
    assert ex.get_meta_args()[10] == (4 if zeros == "tensor" else 3) and ex.get_meta_args()[2] == gs
    ex._check_domain(ex.W_q, ex.scales, ex.zeros, ex.bias)
    for R in SCALE_R:
        assert ex.rows_per_block(65535, R) == R
    for e in (0, 1, E // 2, E - 1):
        lin = ex.expert(e)
        assert lin.W_q.data_ptr() == ex.W_q[e].data_ptr() and torch.equal(lin.W_q, ex.W_q[e]) and torch.equal(lin.scales, ex.scales[e])
        assert lin.get_meta_args() == ex.get_meta_args() and (bias is False or torch.equal(lin.bias, ex.bias[e]))
    assert len(np.unique(ex.W_q.reshape(E, -1).numpy(), axis=0)) == E, "two experts share a W_q slice"
    assert len(np.unique(ex.scales.reshape(E, -1).view(torch.int16).numpy(), axis=0)) == E
    if bias:
        assert len(np.unique(ex.bias.view(torch.int16).numpy(), axis=0)) == E
    # the synthesised numbers are what make_experts packs: every code 0 .. 15, scales and zero points in its ranges
    codes = (ex.W_q[:8].reshape(-1, 1) >> (4 * torch.arange(8, dtype=torch.int32))) & 15
    assert sorted(codes.unique().tolist()) == list(range(16))
    s = ex.scales.float()
    assert 0.005 <= float(s.min()) and float(s.max()) <= 0.0251
    if zeros == "tensor":
        z = -ex.zeros.float() / s
        assert 5.9 <= float(z.min()) and float(z.max()) <= 10.1
        W = (codes.float() - z[:8].mean()) * s.mean()  # (the magnitude of a weight: what make_experts gives)
        assert 0.01 < float(W.abs().mean()) < 0.2


@pytest.mark.parametrize("E", SCALE_E)
def test_the_stack_of_the_routing_tests_is_inside_the_domain_at_every_expert_count(E):
    ex = big_stack(E, dtype=F16, zeros="int", bias=False, **SMALL)
    ex._check_domain(ex.W_q, ex.scales, ex.zeros, ex.bias)
    lib = _hip.load()
    for R in SCALE_R:
        for n in (E + 1,) + RANDOM_N:
            assert ex.rows_per_block(n, R) == R
            r = X._rows_args(X._stand_in_args(ex.bias, ex.get_tensor_args(), ex.get_meta_args(), n), R, None)
            r.workspace, r.workspace_bytes = 0x1000, lib.gemlite_hip_experts_rows_workspace_bytes(n, E, R)
            assert r.workspace_bytes == 4 * X.rows_workspace_ints(n, E, R) > 0 and query(r) == _hip.OK, (E, R, n)
    assert not bool((ex.W_q[0] == ex.W_q[E - 1]).all()) and ex.expert(E - 1).W_q.data_ptr() == ex.W_q[E - 1].data_ptr()


@pytest.mark.parametrize("ids64", [False, True], ids=["int32", "int64"])
@pytest.mark.parametrize("E", SCALE_E)
def test_every_id_pattern_is_what_its_name_says_and_stays_inside_bmax(E, ids64):
    for R in SCALE_R:
        pats = patterns_for(E, R, ids64)
        assert set(pats) == set(PATTERNS) - (set() if E > WAVE0 else {"only experts >= 320"})
        for name, ids in pats.items():
            assert ids.dtype == np.int64 and 1 <= len(ids) <= 65535 and blocks_used(ids, E, R) <= blocks_max(len(ids), E, R), name
            if not ids64:
                assert (ids >= -(1 << 31)).all() and (ids < 1 << 31).all(), name
        counts = {name: np.bincount(buckets_of(ids, E), minlength=E + 1) for name, ids in pats.items()}
        c = counts["every bucket once"]
        assert (c == 1).all() and len(pats["every bucket once"]) == E + 1 and blocks_used(pats["every bucket once"], E, R) == E + 1
        assert not np.array_equal(pats["every bucket once"], np.sort(pats["every bucket once"]))  # shuffled
        c = counts["all on the last expert"]
        assert c[E - 1] == c.sum() > ROUTE_THREADS and c[E - 1] % R != 0
        c = counts["all invalid"]
        assert c[E] == c.sum() > ROUTE_THREADS
        assert set(pats["all invalid"].tolist()) == ({-1, E, HIGH} if ids64 else {-1, E})
        if E > WAVE0:
            c = counts["only experts >= 320"]
            assert not c[:WAVE0].any() and (c[WAVE0:E] >= 1).all() and c[E] == 0 and len(set(c[WAVE0:E].tolist())) == min(3, E - WAVE0)
        c = counts["only experts < 320"]
        assert (c[:min(WAVE0, E)] >= 1).all() and not c[WAVE0:E].any() and c[E] == 3
        c = counts["exact multiples of R"]
        assert (c % R == 0).all() and c[E - 1] > 0 and c[0] > 0 and c[E] == 0 and (c > 0).sum() == min(E, 300) and set(c.tolist()) == {0, R, 2 * R}
        assert blocks_used(pats["exact multiples of R"], E, R) * R == len(pats["exact multiples of R"])
    for n in RANDOM_N:
        ids = random_ids(E, n, ids64)
        b = buckets_of(ids, E)
        assert len(ids) == n and (b[np.arange(n) % 7 == 3] == E).all() and (b[np.arange(n) % 7 != 3] < E).all()
        assert blocks_used(ids, E, 16) <= blocks_max(n, E, 16) and blocks_used(ids, E, 64) <= blocks_max(n, E, 64)
        if n >= 8 * E:
            assert (np.bincount(b, minlength=E + 1)[:E] > 0).mean() > 0.9  # nearly every expert is populated


def test_the_thread_that_owns_a_bucket_and_the_edges_the_expert_counts_sit_on():
    owner = lambda bucket: bucket // ROUTE_PER_THREAD  # noqa: E731
    assert ROUTE_PER_THREAD == -(-(4096 + 1) // ROUTE_THREADS) and WAVE0 == 64 * ROUTE_PER_THREAD
    assert owner(319) == 63 and owner(320) == 64                   # E = 319: buckets 0 .. 319 fill wave 0; E = 320: bucket 320 opens wave 1
    assert owner(4095) == owner(4096) == 819 and owner(4094) == 818  # thread 819 owns the last two buckets of the maximum
    assert 1023 + 1 <= ROUTE_THREADS < 1024 + 1                    # the `e += ROUTE_THREADS` loops: a second pass from E = 1024
    assert _hip.EXPERTS_ROWS_MAX_EXPERTS == 4096 == max(SCALE_E) and X.MAX_SLOTS == 65535 == max(RANDOM_N)


def test_the_grouping_by_one_argsort_is_the_list_version():
    for E, n, R, ids64 in ((8, 300, 16, True), (40, 2000, 64, False), (330, 700, 16, True)):
        ids = random_ids(E, n, ids64, seed=3)
        fast, slow = chunks_of(ids, E, R), chunks_of_slow(ids, E, R)
        assert len(fast) == len(slow) == blocks_used(ids, E, R)
        for (e, slots), (e2, slots2) in zip(fast, slow):
            assert e == e2 and slots.tolist() == slots2
        assert np.array_equal(fast_table(ids, E, R), make_table(ids, E, R))
    assert chunks_of(np.array([-1, HIGH, 2]), 2, 16)[0][0] == 2 and chunks_of(np.array([-1, HIGH, 2]), 2, 16)[0][1].tolist() == [0, 1, 2]


def test_check_table_stays_quick_and_strict_at_the_maximum():
    """n = 65535 over 4096 experts, blocks of 16: the gate of the GPU module, timed on a right table (printed, not asserted: the budget
    is seconds, the figure tenths of one) and held against single wrong entries at the far end of the table."""
    E, n, R = 4096, 65535, 16
    ids = random_ids(E, n, True)
    t0 = time.perf_counter()
    table = fast_table(ids, E, R)
    t1 = time.perf_counter()
    used = check_table(table, ids, E, R)
    t2 = time.perf_counter()
    print(f"n = {n}, E = {E}, R = {R}: {used} blocks of {blocks_max(n, E, R)}; fast_table {t1 - t0:.3f} s, check_table {t2 - t1:.3f} s")
    assert used == blocks_used(ids, E, R) > E
    bmax = blocks_max(n, E, R)
    last = HEADER + used - 1
    for change in (lambda t: t.__setitem__(last, t[last] - 1),                                  # the last block labelled with its neighbour
                   lambda t: t.__setitem__(HEADER + bmax + (used - 1) * R, t[HEADER + bmax]),   # a slot twice, another missing
                   lambda t: t.__setitem__(0, used + 1)):
        bad = table.copy()
        change(bad)
        with pytest.raises(AssertionError):
            check_table(bad, ids, E, R)


def test_the_rows_query_answers_at_the_in_expert_edges():
    wk, mg = rows_edge_stride_wk(), rows_edge_stride_meta_g()
    N, K, gs = ROWS_EDGE_N, ROWS_EDGE_K, ROWS_EDGE_GS
    rows = K // 8
    assert wk % 4 == 0 and rows * wk * 4 + N * 4 < 1 << 32 <= rows * (wk + 4) * 4 + N * 4
    assert wk == edge_stride_wk(K) - 8 == (1 << 25) - 12  # experts_plan alone admits two steps more: the rows rule counts the row the extent ends in
    assert mg % 4 == 0 and (K // gs * mg + N) * 2 < 1 << 32 <= (K // gs * (mg + 4) + N) * 2 and mg == (1 << 28) - 36
    lib = _hip.load()
    for field, edge in (("stride_wk", wk), ("stride_meta_g", mg)):
        r = rows_request(16, N=N, K=K, gs=gs)
        setattr(r.experts.layer, field, edge)
        assert query(r) == _hip.OK, field
        setattr(r.experts.layer, field, edge + 4)
        assert query(r) == _hip.ERR_BAD_SHAPE, field
    r = rows_request(16, N=N, K=K, gs=gs)
    r.experts.layer.stride_wk = edge_stride_wk()  # between the two rules
    assert lib.gemlite_hip_experts_query(C.byref(r.experts)) == _hip.OK and query(r) == _hip.ERR_BAD_SHAPE
    # the 64-bit strides, the output stride and the shared-row counts of the GPU module are inside the domain
    r = rows_request(16, N=N, K=K, gs=gs)
    r.experts.stride_expert_w = r.experts.stride_expert_meta = r.experts.stride_expert_bias = 1 << 32
    r.experts.n_slots, r.experts.slots_per_x_row, r.experts.stride_out_slot = 3, 1, (1 << 31) - 2
    assert query(r) == _hip.OK
    r.experts.stride_out_slot = 1 << 31
    assert query(r) == _hip.ERR_BAD_SHAPE
    for spx in (8, 65535, 1 << 40):
        r = rows_request(16, N=SMALL["N"], K=SMALL["K"], gs=SMALL["gs"])
        r.experts.n_slots, r.experts.n_experts, r.experts.slots_per_x_row = 65535, 4096, spx
        r.workspace_bytes = lib.gemlite_hip_experts_rows_workspace_bytes(65535, 4096, 16)
        assert query(r) == _hip.OK, spx
    r.experts.stride_x_row = 0
    assert query(r) == _hip.OK
