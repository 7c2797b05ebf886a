"""gemlite_hip_experts_route / gemlite_hip_forward_experts_rows and GemLiteExperts.forward_batched, the parts that need no GPU: symbols, the
struct mirror, the workspace formula, the resolution of rows_per_block, one refusal per rule of the domain with its status, the module's
refusals in words, the fake ops, and a numpy restatement of the routing CONTRACT (check_table) that tests/test_experts_rows_gpu.py holds
the kernel's table against."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gemlite_amd
from gemlite_amd import DType, ExpertsRouting, GemLiteExperts, GemLiteExpertsMLP, _hip, experts as X
from tests.test_experts_cpu import make_layers, request as experts_request, set_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, BAD_ARG, UNSUPPORTED, BAD_SHAPE, WORKSPACE = _hip.OK, _hip.ERR_BAD_ARGUMENT, _hip.ERR_UNSUPPORTED, _hip.ERR_BAD_SHAPE, _hip.ERR_WORKSPACE
SYMBOLS = ("gemlite_hip_experts_rows_workspace_bytes", "gemlite_hip_experts_rows_per_block", "gemlite_hip_experts_route",
           "gemlite_hip_forward_experts_rows", "gemlite_hip_experts_rows_query")
MAX_E, MAX_SLOTS = 4096, 65535  # the documented limits (include/gemlite_hip.h)
HEADER = 4


# ---- the routing contract, restated ---------------------------------------------------------------------------------------------------
def buckets_of(ids, E):
    """Bucket of every slot: its id inside [0, E), else E (negative, too large, an int64 with a high dword)."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    return np.where((ids >= 0) & (ids < E), ids, E)


def blocks_max(n_slots, E, R):
    return -(-n_slots // R) + min(E + 1, n_slots)


def blocks_used(ids, E, R):
    counts = np.bincount(buckets_of(ids, E), minlength=E + 1)
    return int(sum(-(-int(c) // R) for c in counts))


def check_table(table, ids, E, R):
    """The contract of a routed work table, not an order: every slot exactly once, in a block of its own bucket; padding is -1; the
    used count is sum ceil(c_e / R); an expert's slots fill ceil(c_e / R) blocks of at most R.  `table`: the int32 entries."""
    table = np.asarray(table, dtype=np.int64)
    b = buckets_of(ids, E)
    n, bmax = len(b), blocks_max(len(b), E, R)
    used = int(table[0])
    assert used == blocks_used(ids, E, R), (used, blocks_used(ids, E, R))
    assert used <= bmax and list(table[1:HEADER]) == [0, 0, 0]
    block_expert = table[HEADER:HEADER + used]
    rows = table[HEADER + bmax:HEADER + bmax + used * R].reshape(used, R)
    assert ((block_expert >= 0) & (block_expert <= E)).all(), block_expert
    assert ((rows >= -1) & (rows < n)).all()
    seen = rows[rows >= 0]
    assert sorted(seen.tolist()) == list(range(n)), "every slot exactly once"
    for blk in range(used):
        slots = rows[blk][rows[blk] >= 0]
        assert len(slots) >= 1 and (b[slots] == block_expert[blk]).all(), (blk, block_expert[blk], slots)
    counts = np.bincount(b, minlength=E + 1)
    for e in range(E + 1):
        assert int((block_expert == e).sum()) == -(-int(counts[e]) // R), e
    return used


def make_table(ids, E, R, order=None):
    """One table that satisfies the contract (slots of a bucket in ascending order, or in `order`)."""
    b = buckets_of(ids, E)
    n, bmax = len(b), blocks_max(len(b), E, R)
    table = np.full(HEADER + bmax + bmax * R, -7, dtype=np.int64)
    table[:HEADER] = 0
    blk = 0
    for e in range(E + 1):
        slots = [s for s in (order if order is not None else range(n)) if b[s] == e]
        for i in range(0, len(slots), R):
            part = slots[i:i + R]
            table[HEADER + blk] = e
            table[HEADER + bmax + blk * R:HEADER + bmax + (blk + 1) * R] = part + [-1] * (R - len(part))
            blk += 1
    table[0] = blk
    return table


def test_the_restatement_accepts_a_right_table_in_any_order_and_rejects_wrong_ones():
    ids = np.array([3, 3, 0, -1, 8, 3, 1 << 40, 7, 3, 3], dtype=np.int64)
    for R in (2, 16):
        t = make_table(ids, 8, R)
        assert check_table(t, ids, 8, R) == blocks_used(ids, 8, R)
        assert check_table(make_table(ids, 8, R, order=list(range(9, -1, -1))), ids, 8, R)
    t = make_table(ids, 8, 2)
    assert list(buckets_of(ids, 8)) == [3, 3, 0, 8, 8, 3, 8, 7, 3, 3] and t[0] == 1 + 3 + 1 + 2
    bmax = blocks_max(10, 8, 2)
    for change in (lambda t: t.__setitem__(0, t[0] - 1),                      # a block short
                   lambda t: t.__setitem__(HEADER, 1),                        # expert 0's block labelled 1
                   lambda t: t.__setitem__(HEADER + bmax, 3),                 # a slot twice, another missing
                   lambda t: t.__setitem__(HEADER + bmax + 1, 0),             # padding that is not -1
                   lambda t: t.__setitem__(1, 5)):                            # the header's zeros
        bad = t.copy()
        change(bad)
        with pytest.raises(AssertionError):
            check_table(bad, ids, 8, 2)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------------
def rows_request(R=0, ws=0x80000, ws_bytes=None, **kw):
    """A valid request on stand-in addresses: tests/test_experts_cpu.py's experts request (8 experts, 6 slots, 2 per x row), a workspace."""
    r = _hip.ExpertsRowsArgs()
    r.struct_size = C.sizeof(_hip.ExpertsRowsArgs)
    r.rows_per_block = R
    r.experts = experts_request(**kw)
    r.workspace = ws
    e = r.experts
    need = _hip.load().gemlite_hip_experts_rows_workspace_bytes(e.n_slots, e.n_experts, R or 16)
    r.workspace_bytes = need if ws_bytes is None else ws_bytes
    return r


def query(r):
    return _hip.load().gemlite_hip_experts_rows_query(C.byref(r))


def test_symbols_are_declared_exported_and_bound_and_the_abi_version_stays():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in SYMBOLS:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    for sym in SYMBOLS[1:]:
        assert getattr(lib, sym).argtypes[0] == C.POINTER(_hip.ExpertsRowsArgs), sym
    assert lib.gemlite_hip_experts_route.argtypes[1] == C.c_void_p and lib.gemlite_hip_forward_experts_rows.argtypes[1] == C.c_void_p
    assert lib.gemlite_hip_experts_rows_workspace_bytes.restype == C.c_uint64
    assert lib.gemlite_hip_abi_version() == 1 and _hip.ABI_VERSION == 1
    assert gemlite_amd.ExpertsRouting is X.ExpertsRouting
    assert f"#define GEMLITE_EXPERTS_ROWS_MAX_EXPERTS {MAX_E}" in header and _hip.EXPERTS_ROWS_MAX_EXPERTS == MAX_E


def test_the_struct_mirror_matches_the_header_field_for_field():
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    body = re.search(r"typedef struct gemlite_hip_experts_rows_args \{(.*?)\} gemlite_hip_experts_rows_args;", header, re.S).group(1)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "uint64_t": C.c_uint64, "int64_t": C.c_int64, "void*": C.c_void_p,
             "gemlite_hip_experts_args": _hip.ExpertsArgs}
    fields = []
    for decl in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";"):
        decl = decl.strip()
        if decl:
            m = re.fullmatch(r"(?:const )?([\w]+\*?)\s+(\w+)(?:\[(\d+)\])?", decl)
            t = ctype[m.group(1)]
            fields.append((m.group(2), t * int(m.group(3)) if m.group(3) else t))
    assert fields == list(_hip.ExpertsRowsArgs._fields_)
    assert [f[0] for f in fields] == ["struct_size", "rows_per_block", "experts", "workspace", "workspace_bytes", "reserved"]
    assert C.sizeof(_hip.ExpertsRowsArgs) == 8 + C.sizeof(_hip.ExpertsArgs) + 8 + 8 + 16


@pytest.mark.parametrize("R", [16, 32, 48, 64])
def test_workspace_bytes_and_bmax_follow_the_formula(R):
    lib = _hip.load()
    for n in (1, 2, 15, 16, 17, 63, 64, 65, 512, 4097, 65535):
        for E in (1, 2, 8, 128, 1024, 4096):
            bmax = -(-n // R) + min(E + 1, n)
            assert X.rows_blocks_max(n, E, R) == bmax == blocks_max(n, E, R)
            assert lib.gemlite_hip_experts_rows_workspace_bytes(n, E, R) == 4 * (HEADER + bmax + bmax * R) == 4 * X.rows_workspace_ints(n, E, R)
            # the bound holds for every id pattern: all on one expert, spread evenly, all invalid
            for ids in (np.zeros(n), np.arange(n) % E, np.full(n, -1)):
                assert blocks_used(ids, E, R) <= bmax
    for n, E, r in ((0, 8, R), (-1, 8, R), (65536, 8, R), (6, 0, R), (6, 4097, R), (6, 8, R + 1), (6, 8, 0), (6, 8, 80)):
        assert lib.gemlite_hip_experts_rows_workspace_bytes(n, E, r) == 0, (n, E, r)


def test_rows_per_block_resolution_and_refusals():
    lib = _hip.load()
    rpb = lambda r: lib.gemlite_hip_experts_rows_per_block(C.byref(r))  # noqa: E731
    for gs in (32, 64, 128, 256):
        for R in (16, 32):
            assert rpb(rows_request(R, gs=gs)) == R and query(rows_request(R, gs=gs)) == OK
        for R in (48, 64):
            assert rpb(rows_request(R, gs=gs)) == (BAD_SHAPE if gs == 32 else R)
            assert query(rows_request(R, gs=gs)) == (BAD_SHAPE if gs == 32 else OK)
        for R in (8, 17, 24, 40, 80, 128, -16):
            assert rpb(rows_request(R, gs=gs)) == BAD_ARG and query(rows_request(R, gs=gs)) == BAD_ARG, R
    # 0: the default — the smallest block that holds the mean slot count per expert, m = n_slots / min(E, n_slots), plus a quarter
    # (m + m // 4); groups of 32 stop at 32
    for n, E, want in ((6, 8, 16), (1, 8, 16), (96, 8, 16), (104, 8, 16), (112, 8, 32), (128, 8, 32), (136, 8, 32), (208, 8, 32), (216, 8, 48),
                       (256, 8, 48), (312, 8, 48), (320, 8, 64), (384, 8, 64), (65535, 8, 64), (512, 128, 16), (1024, 128, 16),
                       (65535, 4096, 32), (65535, 1024, 64)):
        for gs in (32, 128):
            r = rows_request(0, gs=gs)
            r.experts.n_slots, r.experts.n_experts = n, E
            assert rpb(r) == min(want, 32 if gs == 32 else 64), (n, E, gs)
    # it never reads the workspace fields, and nested refusals come through
    r = rows_request(0)
    r.workspace, r.workspace_bytes = None, 0
    assert rpb(r) == 16 and query(r) == WORKSPACE
    r.experts.layer.N = 776
    assert rpb(r) == BAD_SHAPE
    assert lib.gemlite_hip_experts_rows_per_block(None) == BAD_ARG


REFUSALS = [
    ("struct_size + 4", set_("struct_size", C.sizeof(_hip.ExpertsRowsArgs) + 4), BAD_ARG),
    ("struct_size - 4", set_("struct_size", C.sizeof(_hip.ExpertsRowsArgs) - 4), BAD_ARG),
    ("nested struct_size", set_("experts.struct_size", C.sizeof(_hip.ExpertsArgs) - 4), BAD_ARG),
    ("ids int16", set_("experts.ids_dtype", DType.INT16.value), UNSUPPORTED), ("ids fp32", set_("experts.ids_dtype", DType.FP32.value), UNSUPPORTED),
    ("null ids", set_("experts.ids", None), BAD_ARG),
    ("K % 256", set_("experts.layer.K", 2048 + 128), BAD_SHAPE), ("N % 16", set_("experts.layer.N", 776), BAD_SHAPE),
    ("group 16", set_("experts.layer.group_size", 16), BAD_SHAPE), ("group 96", set_("experts.layer.group_size", 96), BAD_SHAPE),
    ("2 bits", lambda r: (set_("experts.layer.W_nbits", 2)(r), set_("experts.layer.elements_per_sample", 16)(r)), UNSUPPORTED),
    ("x 8-byte aligned", set_("experts.layer.x", 0x10008), BAD_ARG), ("x row stride", set_("experts.stride_x_row", 2052), BAD_ARG),
    ("w_q 8-byte aligned", set_("experts.layer.w_q", 0x20008), BAD_ARG),
    ("out 2-byte aligned", set_("experts.layer.out", 0x50002), BAD_ARG), ("odd out stride", set_("experts.stride_out_slot", 769), BAD_ARG),
    ("workspace null", set_("workspace", None), WORKSPACE), ("workspace misaligned", set_("workspace", 0x80002), WORKSPACE),
    ("workspace one byte short", lambda r: set_("workspace_bytes", r.workspace_bytes - 1)(r), WORKSPACE),
    ("x extent at 2^31", lambda r: (set_("experts.n_slots", 2 * 512 + 1)(r), set_("experts.stride_x_row", 1 << 21)(r),
                                    set_("workspace_bytes", 1 << 20)(r)), BAD_SHAPE),
    ("out stride at 2^31", set_("experts.stride_out_slot", 1 << 31), BAD_SHAPE),
    ("too many slots", lambda r: (set_("experts.n_slots", MAX_SLOTS + 1)(r), set_("workspace_bytes", 1 << 26)(r)), BAD_SHAPE),
    ("too many experts", lambda r: (set_("experts.n_experts", MAX_E + 1)(r), set_("workspace_bytes", 1 << 26)(r)), BAD_SHAPE),
]


@pytest.mark.parametrize("what,change,status", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_one_refusal_per_rule_of_the_domain(what, change, status):
    lib = _hip.load()
    r = rows_request()
    assert query(r) == OK
    change(r)
    assert query(r) == status, what
    # the launches validate first too: a refused request never reaches a device
    assert lib.gemlite_hip_experts_route(C.byref(r), None) == status and lib.gemlite_hip_forward_experts_rows(C.byref(r), None) == status


def test_the_edges_of_the_domain_are_inside():
    """One step inside every limit of the refusal table: the x extent just below 2^31, the documented maxima of slots and experts, a
    workspace of exactly the bytes asked for."""
    r = rows_request()
    r.experts.n_slots, r.experts.stride_x_row, r.workspace_bytes = 2 * 512 + 1, (1 << 21) - 8, 1 << 20
    # 513 x rows: 512 * ((2^21 - 8) * 2) + 2048 * 2 = 2^31 - 8192 + 4096 < 2^31
    assert query(r) == OK
    r.experts.stride_x_row = 1 << 21  # 512 * 2^22 + 4096 >= 2^31
    assert query(r) == BAD_SHAPE
    for gs in (32, 128):
        r = rows_request(gs=gs)
        r.experts.n_slots, r.experts.n_experts = MAX_SLOTS, MAX_E
        R = _hip.load().gemlite_hip_experts_rows_per_block(C.byref(r))
        r.workspace_bytes = _hip.load().gemlite_hip_experts_rows_workspace_bytes(MAX_SLOTS, MAX_E, R)
        assert R == 32 and query(r) == OK
        r.workspace_bytes -= 1
        assert query(r) == WORKSPACE
    assert _hip.load().gemlite_hip_experts_rows_query(None) == BAD_ARG
    # the rows kernel's weight extent counts the row it ends in: 256 rows of (2^22 - 4) words are 2^32 - 4096 bytes, and 2048 columns more
    r = rows_request(N=2048)
    r.experts.layer.stride_wk = (1 << 22) - 4
    assert _hip.load().gemlite_hip_experts_query(C.byref(r.experts)) == OK and query(r) == BAD_SHAPE


@pytest.mark.parametrize("dt", [DType.FP16.value, DType.BF16.value])
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
@pytest.mark.parametrize("gs", [32, 64, 128, 256])
def test_valid_requests_are_accepted(dt, mode, gs):
    for N, K in ((48, 768), (256, 4352), (16, 256), (768, 2048)):
        for R in (0, 16, 32) + ((48, 64) if gs > 32 else ()):
            for bias in (True, False):
                assert query(rows_request(R, N=N, K=K, gs=gs, mode=mode, dt=dt, bias=bias)) == OK, (N, K, R)
    if mode in (1, 3):
        assert query(rows_request(gs=gs, mode=mode, dt=dt, scalar_zero=True)) == OK


# ---- the module -----------------------------------------------------------------------------------------------------------------------
def test_routing_and_forward_batched_refuse_in_words():
    ex = GemLiteExperts.from_layers(make_layers(E=3))
    ex32 = GemLiteExperts.from_layers(make_layers(E=3, gs=32))
    assert ex.rows_per_block(10) == 16 and ex.rows_per_block(10, 64) == 64 and ex.rows_per_block(3 * 40) == 64 and ex.rows_per_block(3 * 30) == 48
    assert ex32.rows_per_block(3 * 40) == 32 and ex32.rows_per_block(10, 32) == 32
    with pytest.raises(ValueError, match="rows_per_block is 24"):
        ex.rows_per_block(10, 24)
    with pytest.raises(NotImplementedError, match="groups of 32 take 16 or 32"):
        ex32.rows_per_block(10, 48)
    ids, x = torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 768, dtype=torch.float16)
    with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
        ex.route(ids)
    with pytest.raises(ValueError, match=r"\[\.\.\., top_k\]"):
        ex.route(torch.tensor(3))
    with pytest.raises(NotImplementedError, match="at most 65535"):
        ex.route(torch.zeros(65536, 1, dtype=torch.int64))
    # a routing is a plain holder: its workspace has to fit what it describes
    ws = torch.zeros(X.rows_workspace_ints(10, 3, 16), dtype=torch.int32)
    routing = ExpertsRouting(ws, 16, 10, 3)
    assert routing.blocks_max == blocks_max(10, 3, 16) and "rows_per_block=16" in repr(routing)
    with pytest.raises(ValueError, match="need 89 int32"):
        ExpertsRouting(ws[:-1], 16, 10, 3)
    with pytest.raises(ValueError, match="rows_per_block is 24"):
        ExpertsRouting(ws, 24, 10, 3)
    with pytest.raises(ValueError, match="need"):
        ExpertsRouting(ws.float(), 16, 10, 3)
    # forward_batched: x shapes as forward takes them, a routing of these ids and experts, the dtype
    with pytest.raises(ValueError, match="asks for"):
        ex.forward_batched(torch.zeros(5, 3, 768, dtype=torch.float16), ids, routing)
    with pytest.raises(NotImplementedError, match="x is torch.bfloat16"):
        ex.forward_batched(x.bfloat16(), ids, routing)
    with pytest.raises(TypeError, match="ExpertsRouting"):
        ex.forward_batched(x, ids, ws)
    with pytest.raises(ValueError, match="holds 10 slots over 3 experts"):
        ex.forward_batched(x[:4], ids[:4], routing)
    with pytest.raises(ValueError, match="holds 10 slots over 4 experts"):
        ex.forward_batched(x, ids, ExpertsRouting(torch.zeros(200, dtype=torch.int32), 16, 10, 4))
    with pytest.raises(NotImplementedError, match="groups of 32 take 16 or 32"):
        ex32.forward_batched(x, ids, ExpertsRouting(torch.zeros(1000, dtype=torch.int32), 48, 10, 3))
    with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):  # and there is no CPU path behind a right call
        ex.forward_batched(x, ids, routing)


def test_the_mlp_picks_a_block_size_both_stacks_take():
    gate = make_layers(E=3, N=256, K=768, gs=128, bias=False)
    up = make_layers(E=3, N=256, K=768, gs=128, bias=False, seed=1)
    for gs_down, want in ((128, 64), (32, 32)):
        mlp = GemLiteExpertsMLP(GemLiteExperts.from_gate_up(gate, up), GemLiteExperts.from_layers(make_layers(E=3, N=768, K=256, gs=gs_down, bias=False)))
        assert mlp.gate_up.rows_per_block(120) == 64 and mlp.down.rows_per_block(120) == want
        assert mlp.rows_per_block(120) == want
        with pytest.raises(ValueError, match="one weight per slot"):
            mlp.forward_batched(torch.zeros(5, 768, dtype=torch.float16), torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 3))
        with pytest.raises(_hip.GemliteHipError, match="no CPU fallback"):
            mlp.forward_batched(torch.zeros(5, 768, dtype=torch.float16), torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, 2))


def test_the_fake_implementations_give_shape_and_dtype():
    from torch._subclasses.fake_tensor import FakeTensorMode
    ex = GemLiteExperts.from_layers(make_layers(E=3))
    route, rows = torch.ops.gemlite.experts_route, torch.ops.gemlite.forward_experts_rows
    assert "gemlite::experts_route" in str(route.default._schema) and "gemlite::forward_experts_rows" in str(rows.default._schema)
    with FakeTensorMode() as mode:
        targs = [mode.from_tensor(t) for t in ex.get_tensor_args()]
        ids = torch.empty((5, 2), dtype=torch.int64)
        for R in (16, 64):
            ws = route(ids, R, None, targs, ex.get_meta_args())
            assert tuple(ws.shape) == (X.rows_workspace_ints(10, 3, R),) and ws.dtype == torch.int32
            y = rows(torch.empty((5, 768), dtype=torch.float16), ids, ws, R, None, targs, ex.get_meta_args())
            assert tuple(y.shape) == (5, 2, 48) and y.dtype == torch.float16
            y = rows(torch.empty((5, 2, 768), dtype=torch.bfloat16), ids, ws, R, None, targs, ex.get_meta_args())
            assert tuple(y.shape) == (5, 2, 48) and y.dtype == torch.bfloat16
            with pytest.raises(Exception):
                rows(torch.empty((5, 3, 768), dtype=torch.float16), ids, ws, R, None, targs, ex.get_meta_args())
        assert tuple(route(torch.empty((0, 2), dtype=torch.int64), 16, None, targs, ex.get_meta_args()).shape) == (X.rows_workspace_ints(1, 3, 16),)
