"""The inventory of kernel forms the forward planner answers with, and everything the two test files that use it share.

A FORM is what `gemlite_hip_kernel_name` answers: a kernel label such as `gemm_w4_mma_kernel<64x128>` (with its pack-width suffix `,b8>` /
`,b16>` where it carries one).  The unit of the inventory is (form, 16-bit type of the layer); per unit one request at the smallest
shape the sweep found, one ragged row count where the tile is taller than that request, and one request with K slices (workspace bytes
> 0) where the form has them.  `python tests/kernel_forms.py --write` regenerates tests/golden/kernel_forms.json — data only.

Three parts:
  * recipes: one per layer family, `recipe(fam, tdt, M, N, K, mt, tuning)` -> the ForwardArgs of that request exactly as the Python layer
    would fill them (tests/test_kernel_forms_cpu.py compares them field by field with the layers `build_layer` packs);
  * the sweep over M x (N, K) x matmul_type x the documented tuning values of the family, and the selection of the rows to freeze;
  * the layers, activations, float64 oracle and checker of tests/test_kernel_forms_gpu.py — written against a `device` argument, so the CPU
    test runs the same code on CPU tensors (to check the recipes and to check that the checker rejects wrong results).
Not collected by pytest (no test_ prefix), like dequant_spec.py and quant_int_spec.py."""
import ctypes as C
import json
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from tests.test_host_cpu import _args  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "kernel_forms.json")
CSRC = os.path.join(os.path.dirname(HERE), "gemlite_amd", "csrc")

FP32, FP16, BF16, FP8E4, INT8, UINT8, INT32, FP8E5, INT16 = 0, 1, 2, 3, 4, 5, 6, 8, 9
MXFP16, MXBF16, MXFP8, MXFP4, NVFP4 = 14, 15, 16, 17, 18
TDT_NAME = {FP16: "fp16", BF16: "bf16"}


# ------------------------------------------------------------------------------------------------ synthetic requests (moved from test_planner_tile_families_cpu.py)
def _mx(in_dt, nbits, M, c_mode, N, K, group=32):
    """A block-scaled request in the K-contiguous layout of pack() (input types: 14 / 15 = fp16 / bf16 over MX weights, 16 = MXFP8, 17 = MXFP4, 18 = NVFP4)."""
    a = _hip.ForwardArgs()
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = -1
    a.x = a.w_q = a.scales = a.out = a.scales_x = 0x1000
    a.M, a.N, a.K = M, N, K
    a.W_nbits, a.group_size, a.unpack_mask = nbits, group, 2 ** nbits - 1
    a.elements_per_sample = 1 if nbits == 8 else 2
    a.w_pack_bits = 0 if nbits == 8 else 8
    a.w_dtype = 3 if nbits == 8 else 5
    a.input_dtype, a.output_dtype, a.meta_dtype = in_dt, (1 if in_dt == 14 else 2), 5
    a.channel_scale_mode, a.W_group_mode = c_mode, 0
    a.stride_xm, a.stride_xk = (K if in_dt in (14, 15, 16) else K // 2), 1
    a.stride_wk, a.stride_wn = 1, (K if nbits == 8 else K // 2)
    a.stride_om, a.stride_on = N, 1
    a.stride_meta_g, a.stride_meta_n = N, 1
    a.stride_sx_m = K // group
    return a


def _a8(in_dt, M, N, K):
    a = _args(M=M, N=N, K=K, nbits=8, e=1, in_dt=in_dt, w_mode=0, c_mode=3, out_dt=1, gs=K)
    a.scales_x = 0x1000
    return a


# ------------------------------------------------------------------------------------------------ the candidate space
MS = (1, 2, 3, 4, 5, 16, 17, 32, 33, 48, 49, 64, 65, 100, 129, 256, 257, 300, 513)
SHAPES = ((128, 256), (256, 512), (192, 384), (512, 1024), (1024, 2048), (1024, 4096 + 128))   # ascending N K; the last one: long-K forms
WIDE = ((128, 256), (256, 512), (192, 384), (512, 1024), (1024, 2048), (8192, 256), (1024, 4096 + 128))   # ... with a wide N for the forms that count tiles or blocks
SMALL_NK = 1024 * 2048
FORCED_MT = (0, 1, 2, 3, 4)   # GEMV, GEMV_REVSPLITK, GEMV_SPLITK, GEMM_SPLITK, GEMM (include/gemlite_hip.h)


def _tunings(t0, t1, t2, flags, flag_t0=None):
    """(t0 x t1 x t2) without flags, and every flag alone over t0 (t1 = t2 = 0): the flags are A/B switches of a family's default plan and of a
    forced kernel, the tile numbers of tuning[1 .. 2] do not interact with them in any planner."""
    out = [(a, b, c, 0) for a in t0 for b in t1 for c in t2]
    out += [(a, 0, 0, f) for f in flags for a in (t0 if flag_t0 is None else flag_t0)]
    return tuple(dict.fromkeys(out))


# the values include/gemlite_hip.h documents per family (enum gemlite_hip_tuning0 / tuning2 / tuning_flags and the comment in the struct)
T_PACKED_X16 = _tunings((0, 1, 2, 3, 4, 9, 21, 22, 24), (0, 1, 2, 4), (0, 1, 2, 4, 8, 16, 20, 24, 32, 33, 34, 35, 48, 82),
                        (1, 2, 16, 32, 128, 512, 1024, 2048, 4096, 16384, 65536, 131072))
# 8- and 16-bit words: the same kernel choices, tile geometries and flags (the planners refuse what they have no word source for); K slices: auto and two
T_PACKED_NARROW_WORDS = _tunings((0, 1, 2, 3, 4, 9, 21, 22, 24), (0, 2), (0, 1, 2, 4, 8, 16, 20, 24, 32, 33, 34, 35, 48, 82),
                                 (1, 2, 16, 32, 128, 512, 1024, 2048, 4096, 16384, 65536, 131072))
T_PACKED_X8 = _tunings((0, 4, 7), (0, 1, 2, 4), (0, 1, 2, 4, 8, 32), (16384,))
T_A8W8 = _tunings((0, 1, 2, 4, 5, 6, 7, 8, 10), (0, 1, 2, 4), (0, 1, 2, 3, 4, 5, 8), (64, 524288, 1048576, 2097152, 4194304))
T_A8W8 += tuple((0, sk, rows, 64) for sk in (0, 2) for rows in (4, 8))   # the 128- / 256-row tiles with the weights straight from memory
T_A16W8 = _tunings((0, 2, 4, 7), (0, 1, 2, 4), (0, 1, 2, 4, 8, 32), (524288, 1048576))
T_MX = _tunings((0, 1, 2, 3, 4, 5, 6), (0, 1, 2, 4), (0, 1, 2, 3, 4, 8, 32), (1, 2, 16, 16384))
T_NONE = ((0, 0, 0, 0),)
T_FUSED = ((0, 0, 0, 0), (7, 0, 0, 0), (8, 0, 0, 0))   # (a forced kernel refuses the in-launch quantiser: only M = 1 of A8W8 reads tuning[0])


class Family:
    def __init__(self, kind, tunings, mts=(-1,), ms=MS, shapes=SHAPES, **params):
        self.kind, self.tunings, self.mts, self.ms, self.shapes, self.params = kind, tunings, mts, ms, shapes, params


def _families():
    f = {}
    for nbits in (4, 2, 1, 8):
        for gs in (128, 64, 32, 96, 0):          # 0: channel-wise (one scale and zero per output column)
            for pb in (32, 16, 8):
                if pb < 32 and pb // nbits < 2:
                    continue                     # (8-bit codes in 8-bit words are not packed)
                name = f"a16w{nbits}_" + (f"g{gs}" if gs else "ch") + (f"_b{pb}" if pb != 32 else "")
                f[name] = Family("a16wn", T_PACKED_X16 if pb == 32 else T_PACKED_NARROW_WORDS, (-1,) + FORCED_MT, nbits=nbits, gs=gs, pb=pb)
    for w, code in (("int8", INT8), ("fp8", FP8E4)):
        for post in (0, 1):
            f[f"a16w8_{w}" + ("_post" if post else "")] = Family("a16w8", T_A16W8, (-1, 4), shapes=WIDE, w_dt=code, post=post)
    for act, code in (("int8", INT8), ("e4m3", FP8E4), ("e5m2", FP8E5)):
        f[f"a8w8_{act}"] = Family("a8w8", T_A8W8, (-1, 0, 3, 4), shapes=WIDE, act=code, fused=0)
        f[f"a8w8_{act}_fq"] = Family("a8w8", T_FUSED, ms=tuple(m for m in MS if m <= 65), act=code, fused=1)
    for nbits in (4, 2):
        for gs in (128, 32, 0):
            tag = f"a8w{nbits}_fp8_" + (f"g{gs}" if gs else "ch")
            f[tag] = Family("a8wn", T_PACKED_X8, (-1, 0, 3, 4), nbits=nbits, gs=gs, act=FP8E4, fused=0)
            if gs != 32:
                f[tag + "_fq"] = Family("a8wn", T_NONE, ms=(1, 2), nbits=nbits, gs=gs, act=FP8E4, fused=1)
    f["a8w158_int8"] = Family("a8wn", T_PACKED_X8, (-1, 0, 3, 4), nbits=2, gs=0, act=INT8, fused=0)
    f["a8w158_int8_fq"] = Family("a8wn", T_NONE, ms=(1, 2), nbits=2, gs=0, act=INT8, fused=1)
    for tag, in_dt, nbits, c_mode in (("mx_a8w8", MXFP8, 8, 4), ("mx_a8w8_post", MXFP8, 8, 2), ("mx_a8w4", MXFP8, 4, 4), ("mx_a8w4_post", MXFP8, 4, 2),
                                      ("mx_a4w4", MXFP4, 4, 4), ("nvfp4", NVFP4, 4, 4)):
        f[tag] = Family("mx", T_MX, in_dt=in_dt, nbits=nbits, c_mode=c_mode, fused=0)
        f[tag + "_fq"] = Family("mx", T_NONE, ms=(1, 2), in_dt=in_dt, nbits=nbits, c_mode=c_mode, fused=1)
    f["a16w8_mxfp"] = Family("mx", T_MX, in_dt=MXFP16, nbits=8, c_mode=0, fused=0)
    f["a16w4_mxfp"] = Family("mx", T_MX, in_dt=MXFP16, nbits=4, c_mode=0, fused=0)
    f["f16"] = Family("f16", T_NONE, (-1, 0, 4))
    return f


FAMILIES = _families()


def shape_ok(fam, N, K):
    p = FAMILIES[fam].params
    gs = p.get("gs", 0)
    return not gs or K % gs == 0


def recipe(fam, tdt, M, N, K, mt=-1, tuning=(0, 0, 0, 0)):
    """The ForwardArgs of one request to a layer of family `fam` whose 16-bit type is `tdt` (FP16 / BF16), as core._call_args fills them for the
    layer build_layer() packs (pointers: a 4 KiB-aligned stand-in, or NULL where the layer holds no such tensor)."""
    F = FAMILIES[fam]
    p = F.params
    if F.kind in ("a16wn", "a8wn"):
        nbits, gs, pb = p["nbits"], p["gs"], p.get("pb", 32)
        x8 = F.kind == "a8wn"
        bitnet = x8 and p["act"] == INT8
        if gs:
            w_mode, c_mode = (3, 2) if x8 else (4, 0)
        else:
            w_mode, c_mode = (1, 3) if x8 else (1, 1)
        in_dt = p["act"] if x8 else tdt
        a = _args(M=M, N=N, K=K, nbits=nbits, gs=gs or K, in_dt=in_dt, w_mode=w_mode, c_mode=c_mode, mt=mt, e=pb // nbits, out_dt=tdt, tuning=tuning,
                  meta_dt=FP32 if bitnet else tdt, zeros_dt=INT32 if bitnet else tdt, zero_scalar=int(bitnet))
        a.w_pack_bits, a.w_dtype = pb, {32: INT32, 16: INT16, 8: UINT8}[pb]
        a.stride_meta_g, a.stride_meta_n = (N if gs else 1), 1   # ([1, N] metadata is the transpose of an [N, 1] view: both strides 1)
        if bitnet:
            a.acc_dtype = INT32
        a.type_id = (in_dt if x8 else FP16) * 100 + nbits
        a.data_contiguous = 1
        if x8:
            a.scales_x, a.stride_sx_m = 0x1000, 1
            if p["fused"]:
                a.input_dtype, a.scales_x, a.stride_sx_m = tdt, None, 0
    elif F.kind == "a16w8":
        a = _args(M=M, N=N, K=K, nbits=8, e=1, gs=K, in_dt=tdt, w_dtype=p["w_dt"], w_mode=0 if p["post"] else 2, c_mode=1 if p["post"] else 0, mt=mt,
                  meta_dt=FP32, zeros_dt=FP32, tuning=tuning)
        a.zeros = None
        a.stride_meta_g = 1
        a.type_id = FP16 * 100 + 8
    elif F.kind == "a8w8":
        a = _args(M=M, N=N, K=K, nbits=8, e=1, gs=K, in_dt=p["act"], w_mode=0, c_mode=3, mt=mt, out_dt=tdt, meta_dt=FP32, zeros_dt=FP32, tuning=tuning)
        a.zeros = None
        a.stride_meta_g = 1
        a.acc_dtype = INT32 if p["act"] == INT8 else FP32
        a.scales_x, a.stride_sx_m = 0x1000, 1
        a.type_id = p["act"] * 100 + 8
        if p["fused"]:
            a.input_dtype, a.scales_x, a.stride_sx_m = tdt, None, 0
    elif F.kind == "mx":
        in_dt, nbits, c_mode = p["in_dt"], p["nbits"], p["c_mode"]
        x16 = in_dt == MXFP16
        if x16 and tdt == BF16:
            in_dt = MXBF16
        nv = in_dt == NVFP4
        a = _mx(in_dt, nbits, M, c_mode, N, K, group=16 if nv else 32)
        a.matmul_type = mt
        a.output_dtype = tdt
        a.meta_dtype = a.zeros_dtype = FP8E4 if nv else UINT8
        a.W_group_mode = 2 if x16 else 0
        a.type_id = (MXFP16 if x16 else in_dt) * 100 + nbits
        if x16:
            a.scales_x, a.stride_sx_m = None, 0
        elif c_mode == 2:
            a.stride_sx_m = 1
        if p["fused"]:
            a.input_dtype, a.scales_x, a.stride_sx_m = tdt, None, 0
            a.stride_xm = K
        for i, t in enumerate(tuning):
            a.tuning[i] = t
    elif F.kind == "f16":
        a = _args(M=M, N=N, K=K, nbits=16, e=1, gs=1, in_dt=tdt, w_mode=0, c_mode=0, mt=mt, tuning=tuning)
        a.scales = a.zeros = None
        a.meta_dtype = a.zeros_dtype = INT32   # (absent metadata travels as empty int32 tensors)
        a.stride_meta_g, a.stride_meta_n = 0, 1
        a.type_id = FP16 * 100 + 16
    else:
        raise KeyError(fam)
    return a


def load_lib():
    lib = _hip.load()
    lib.gemlite_hip_workspace_bytes.restype = C.c_uint64
    lib.gemlite_hip_kernel_name.restype = C.c_char_p
    return lib


def plan(lib, a):
    """(kernel name, workspace bytes) of a request; ("", 0) where the planner refuses it"""
    name = lib.gemlite_hip_kernel_name(C.byref(a))
    if not name:
        return "", 0
    return name.decode(), int(lib.gemlite_hip_workspace_bytes(C.byref(a)))


def sweep(lib=None, families=None):
    """Every candidate's plan: yields (fam, tdt, M, N, K, mt, tuning, name, ws) in ascending N K, then M, per family and type."""
    lib = lib or load_lib()
    ref = C.byref
    kn, wsb = lib.gemlite_hip_kernel_name, lib.gemlite_hip_workspace_bytes
    for fam in (families or FAMILIES):
        F = FAMILIES[fam]
        for tdt in (FP16, BF16):
            for (N, K) in F.shapes:
                if not shape_ok(fam, N, K):
                    continue
                for M in F.ms:
                    a = recipe(fam, tdt, M, N, K)
                    r = ref(a)
                    for mt in F.mts:
                        a.matmul_type = mt
                        for tun in F.tunings:
                            a.tuning[0], a.tuning[1], a.tuning[2], a.tuning[3] = tun
                            name = kn(r)
                            if name:
                                yield fam, tdt, M, N, K, mt, tun, name.decode(), int(wsb(r))


# ------------------------------------------------------------------------------------------------ selection
_TILE = re.compile(r"<(\d+)x(\d+)")


def tile_rows(name):
    """the rows of one tile of a form, or 0 where its label names none (GEMV forms, streaming and coverage kernels)"""
    m = _TILE.search(name)
    return int(m.group(1)) if m else 0


def has_slices(c):
    """the plan of this candidate splits K: it asks for slabs behind the arrival counters.  (Workspace bytes alone do not say so: the NVFP4 tile forms always
    hold the fp16 expansion of x and one factor per row there — plan_forward.hip, K_NV_MMA — and the fused-quantiser rows forms the quantised x.)"""
    fam, tdt, M, N, K, mt, tun, name, ws = c
    if name.startswith("gemm_nvfp4_f16_kernel"):
        a256 = lambda n: (n + 255) & ~255   # noqa: E731
        return ws > COUNTER_BYTES + a256(M * K * 2) + a256(M * 4)
    if "_fq_kernel" in name:
        return False
    return ws > 0


def select(cands):
    """The rows to freeze from the sweep's answers: per (name, tdt) the first candidate (ascending N K, then M, then the order of matmul types and
    tunings); a ragged second row count where the first one does not spill over one tile; and the first candidate with workspace bytes > 0."""
    first, above, below, split, ragged = {}, {}, {}, {}, {}

    def keep(table, key, rank, c):   # the candidates of the lowest rank, one per family (the first in the order of matmul types and tunings)
        if key not in table or rank < table[key][0]:
            table[key] = (rank, {c[0]: c})
        elif rank == table[key][0]:
            table[key][1].setdefault(c[0], c)

    for c in cands:
        fam, tdt, M, N, K, mt, tun, name, ws = c
        key = (name, tdt)
        rank = (N * K, M)
        keep(first, key, rank, c)
        if has_slices(c):
            keep(split, key, rank, c)
        rows = tile_rows(name)
        if rows and M == rows + 1:
            keep(above, key, rank, c)
        elif rows and M == rows - 1:
            keep(below, key, rank, c)
    # Where several families reach a form at the same shape and row count, the rows go to the family that has the fewest so far (then the first in
    # FAMILIES): the inventory spends its launches on as many layer kinds as the forms allow, not all on the first family of the list.
    used = {f: 0 for f in FAMILIES}
    order = {f: i for i, f in enumerate(FAMILIES)}

    def choose(entry):
        fam = min(entry[1], key=lambda f: (used[f], order[f]))
        used[fam] += 1
        return entry[1][fam]

    for key in sorted(first):
        first[key] = (first[key][0], choose(first[key]))
    for key in sorted(first):
        rows, M = tile_rows(key[0]), first[key][1][2]
        # tile rows + 1 — or tile rows - 1 where the form stops at one tile (forms capped at 64 rows)
        if rows and M <= rows:
            pick = above.get(key) or (below.get(key) if M != rows - 1 else None)
            if pick:
                ragged[key] = choose(pick)
        if key in split:
            split[key] = (split[key][0], choose(split[key]) if not has_slices(first[key][1]) and not (key in ragged and has_slices(ragged[key])) else None)
    rows_out = []
    for key in sorted(first):
        picks = [("first", first[key][1])]
        if key in ragged:
            picks.append(("ragged", ragged[key]))
        if key in split and split[key][1] is not None:
            picks.append(("split", split[key][1]))
        for role, (fam, tdt, M, N, K, mt, tun, name, ws) in picks:
            row = dict(family=fam, kind=FAMILIES[fam].kind, params=FAMILIES[fam].params, tdt=TDT_NAME[tdt], M=M, N=N, K=K,
                       group_size=FAMILIES[fam].params.get("gs", 0) or (32 if FAMILIES[fam].kind == "mx" else K),
                       matmul_type=mt, tuning=list(tun), name=name, workspace_bytes=ws, role=role)
            if N * K > SMALL_NK:
                row["why"] = "no candidate at or below 1024 x 2048 plans to this form: it needs a long K (K slices, the long-K rules of the planner)"
            rows_out.append(row)
    return rows_out


def load_rows():
    with open(GOLDEN) as f:
        return json.load(f)["rows"]


def row_id(r):
    return f"{r['name']}|{r['tdt']}|{r['family']}|M{r['M']}|{r['N']}x{r['K']}|mt{r['matmul_type']}|t{'.'.join(map(str, r['tuning']))}"


def row_args(r):
    return recipe(r["family"], FP16 if r["tdt"] == "fp16" else BF16, r["M"], r["N"], r["K"], r["matmul_type"], tuple(r["tuning"]))


_LITERAL = re.compile(r'"([a-z0-9_]+_kernel(?:<[^"]*>)?)"')


def source_names():
    """every string literal in csrc that reads like a kernel label, read as text"""
    out = set()
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(CSRC, fn), errors="replace") as f:
                out.update(_LITERAL.findall(f.read()))
    return out


def pack_width_names():
    """The labels `pw_label` can compose at run time (`name,b8>` / `name,b16>`; api.hip): of every label with a tile suffix in a file that calls pw_label.
    They are no literals, so the completeness test adds them to its universe from here — not from what the sweep happens to reach."""
    out = set()
    for fn in sorted(os.listdir(CSRC)):
        if not fn.endswith((".hip", ".inc")) or fn == "api.hip":
            continue
        with open(os.path.join(CSRC, fn), errors="replace") as f:
            text = f.read()
        if "pw_label(" in text:
            out.update(n[:-1] + sfx for n in _LITERAL.findall(text) if n.endswith(">") for sfx in (",b8>", ",b16>"))
    return out


def write():
    rows = select(c for c in sweep() if c[7].endswith(("_kernel", ">")))   # (not the status words the query answers for a refused request)
    with open(GOLDEN, "w") as f:
        f.write('{"_note": "one request per kernel form the forward planner answers and 16-bit type (first: the smallest shape of the sweep in tests/kernel_forms.py; ragged: a row count '
                'that does not fill its tiles; split: K slices, workspace bytes > 0); regenerate with python tests/kernel_forms.py --write", "rows": [\n')
        f.write(",\n".join(" " + json.dumps(r) for r in rows))
        f.write("\n]}\n")
    names = {r["name"] for r in rows}
    print(len(rows), "rows,", len(names), "names,", sum(1 for r in rows if r["N"] * r["K"] > SMALL_NK), "above the small cap")
    return rows


# ------------------------------------------------------------------------------------------------ layers, activations, oracle, checker
# (torch, numpy and the family tests' helpers are imported inside the functions: `--write` needs none of them)
COUNTER_BYTES = 65536 * 4   # the arrival counters at the head of a workspace (gl_common.h)
_LAYERS = {}


def torch_dtype(tdt):
    import torch
    return torch.float16 if tdt in (FP16, "fp16") else torch.bfloat16


def _seed(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode())


def build_layer(fam, tdt, N, K, device):
    """The layer of family `fam` through the public path (GemLiteLinear.pack or the helper processor), on `device`.  Codes, scales and zeros are
    random per element / per (group, column), so any two groups and any two columns differ; weight rows differ in magnitude."""
    import numpy as np
    import torch
    from gemlite_amd import DType, GemLiteLinear, helper as H
    key = (fam, tdt, N, K, str(device))
    if key in _LAYERS:
        return _LAYERS[key]
    F = FAMILIES[fam]
    p = F.params
    tt = torch_dtype(tdt)
    rng = np.random.default_rng(_seed(fam, N, K))
    code = DType(tdt)

    def float_weight(div):
        W = rng.standard_normal((N, K), dtype=np.float32) / div
        W *= (1.7 ** (np.arange(N) % 5))[:, None]           # neighbouring columns of the output differ in magnitude, and so in every scale they carry
        W[:, :32] *= 4.0                                      # ... and so do the blocks of a column
        return torch.from_numpy(W).to(tt)

    if F.kind in ("a16wn", "a8wn") and not (F.kind == "a8wn" and p["act"] == INT8):
        nbits, g = p["nbits"], p["gs"] or K
        W_q = rng.integers(0, 2 ** nbits, size=(N, K), dtype=np.uint8)
        ng = N * K // g
        # (code steps worth the same at every bit width: outputs stay around 0.1, where the absolute gate of the family tests is not the bf16 rounding of the output)
        s = torch.from_numpy((rng.random((ng, 1), dtype=np.float32) * 0.01 + 0.002) * (16.0 / 2 ** nbits)).to(tt)
        z = rng.random((ng, 1), dtype=np.float32) * (2 ** nbits - 1)
        if nbits == 8:   # codes within a few steps of their group's zero point, as quantised weights lie: one code step stays visible next to the column's sum
            W_q = np.clip(np.rint(np.repeat(z.reshape(N, K // g), g, axis=1) + rng.normal(0.0, 5.0, size=(N, K))), 0, 255).astype(np.uint8)
        W_q, z = torch.from_numpy(W_q), torch.from_numpy(z).to(tt)
        if F.kind == "a16wn":
            lin = GemLiteLinear(nbits, g, K, N, code, code)
            lin.pack(W_q.to(device), s.to(device), z.to(device), packing_bitwidth=p["pb"])
        else:
            lin = H.A8Wn_HQQ_INT_dynamic(device=device, dtype=tt, post_scale=not p["gs"], W_nbits=nbits).from_weights(W_q, s, z)
    elif F.kind == "a8wn":   # BitNet, int8 activations: ternary codes, one scale for the matrix
        lin = H.A8W158_INT_dynamic(device=device, dtype=tt).from_weights(torch.from_numpy(rng.integers(-1, 2, size=(N, K)).astype(np.float32)).to(tt), torch.tensor(0.02))
    elif F.kind == "a16w8":
        lin = H.A16W8(device=device, dtype=tt, fp8=torch.float8_e4m3fn if p["w_dt"] == FP8E4 else None, post_scale=bool(p["post"])).from_weights(float_weight(30).to(device))
    elif F.kind == "a8w8":
        fp8 = {INT8: False, FP8E4: torch.float8_e4m3fn, FP8E5: torch.float8_e5m2}[p["act"]]
        lin = H.A8W8_dynamic(device=device, dtype=tt, fp8=fp8).from_weights(float_weight(30).to(device))
    elif F.kind == "mx":
        lin_f = torch.nn.Linear(K, N, bias=False, dtype=tt)
        with torch.no_grad():
            lin_f.weight.copy_(float_weight(10))
        lin_f = lin_f.to(device)
        in_dt, nbits, c_mode = p["in_dt"], p["nbits"], p["c_mode"]
        if in_dt == MXFP16:
            proc = (H.A16W8_MXFP if nbits == 8 else H.A16W4_MXFP)(device=device, dtype=tt)
        elif in_dt == MXFP8:
            proc = (H.A8W8_MXFP_dynamic if nbits == 8 else H.A8W4_MXFP_dynamic)(device=device, dtype=tt, post_scale=c_mode == 2)
        else:
            proc = (H.A4W4_MXFP_dynamic if in_dt == MXFP4 else H.A4W4_NVFP_dynamic)(device=device, dtype=tt)
        lin = proc.from_linear(lin_f, del_orig=False)
    elif F.kind == "f16":
        lin = GemLiteLinear(16, None, K, N, code, code)
        lin.pack(float_weight(30).to(device), None, None, None)
    else:
        raise KeyError(fam)
    if len(_LAYERS) >= 24:
        _LAYERS.pop(next(iter(_LAYERS)))
    _LAYERS[key] = lin
    return lin


def make_x(tdt, M, K, device):
    """[M, K] activations of the 16-bit type: rows pairwise distinct (random), each with a mean of its own that is not zero, so a row, column or group mix-up
    moves the result by far more than rounding"""
    import numpy as np
    import torch
    rng = np.random.default_rng(_seed("x", M, K))
    x = rng.standard_normal((M, K), dtype=np.float32) / 8 + (0.05 + 0.01 * (np.arange(M) % 7))[:, None].astype(np.float32)
    x *= np.float32(0.5 * (256.0 / K) ** 0.5)   # (the same output magnitude at every K)
    return torch.from_numpy(x).to(torch_dtype(tdt)).to(device)


def quantise_x(fam, x):
    """(x as the matmul reads it, scales_x or None) for a request that brings quantised activations: the project's quantisers on the GPU, the oracle's on
    CPU tensors (the two are bit-identical: tests/test_gpu_parity.py, tests/test_mx_gpu.py)."""
    import numpy as np
    import torch
    from oracle import gemlite_oracle as O, mx_oracle as MX
    F = FAMILIES[fam]
    p = F.params
    gpu = x.is_cuda
    if F.kind == "mx":
        in_dt, c_mode = p["in_dt"], p["c_mode"]
        if in_dt == MXFP16:
            return x, None
        if gpu:
            from gemlite_amd.quant_utils import scale_activations_mxfp4, scale_activations_mxfp8, scale_activations_nvfp4, scale_activations_per_token
            if in_dt == MXFP8:
                return scale_activations_per_token(x, w_dtype=torch.float8_e4m3fn) if c_mode == 2 else scale_activations_mxfp8(x)
            return (scale_activations_mxfp4 if in_dt == MXFP4 else scale_activations_nvfp4)(x)
        xf = x.float().numpy()
        if in_dt == MXFP8 and c_mode == 2:
            v, s = O.scale_activations_per_token(x, O.FP8E4)
            return torch.from_numpy(v).to(torch.float8_e4m3fn), torch.from_numpy(s)
        if in_dt == MXFP8:
            y, s = MX.scale_activations_mxfp8(xf)
            return torch.from_numpy(y).view(torch.float8_e4m3fn), torch.from_numpy(s)
        y, s = (MX.scale_activations_mxfp4 if in_dt == MXFP4 else MX.scale_activations_nvfp4)(xf)
        s = torch.from_numpy(s)
        return torch.from_numpy(y), (s.view(torch.float8_e4m3fn) if in_dt == NVFP4 else s)
    if F.kind in ("a8w8", "a8wn"):
        qdt = {INT8: torch.int8, FP8E4: torch.float8_e4m3fn, FP8E5: torch.float8_e5m2}[p["act"]]
        if gpu:
            from gemlite_amd.quant_utils import scale_activations_per_token
            return scale_activations_per_token(x, w_dtype=qdt)
        v, s = O.scale_activations_per_token(x, {INT8: O.INT8, FP8E4: O.FP8E4, FP8E5: O.FP8E5}[p["act"]])
        return torch.from_numpy(v).to(qdt), torch.from_numpy(np.asarray(s, np.float32))
    return x, None


def _bytes(t):
    import torch
    return t.contiguous().view(torch.uint8).cpu().numpy()


def oracle_parts(fam, lin, xq, sx, name=""):
    """The float64 oracle (oracle/gemlite_oracle.py, oracle/mx_oracle.py) on the tensors the layer holds and the activations the matmul reads, in parts:
    X [M, K] and W [K, N] dequantised, U [K, N] = what one code step of every weight is worth (its scale), the per-row and per-column factors of the
    epilogue and the layer's constant factor.  The result is ((X @ W) * row[:, None] * col[None, :]) * post.
    `name`: the form that runs — fp8 activations over packed words multiply weights rounded to e4m3 (the reference's `b.to(a.dtype)`), in the GEMV family
    at one row weights rounded to the layer's 16-bit type (tests/test_gpu_parity.py, test_a8wn_fp8_activations_on_the_mfma_kernel)."""
    import numpy as np
    from oracle import gemlite_oracle as O, mx_oracle as MX
    F = FAMILIES[fam]
    p = F.params
    M = xq.shape[0]
    if F.kind == "mx":
        from tests.test_mx_gpu import _weights_nk
        in_dt, c_mode = p["in_dt"], p["c_mode"]
        nv = in_dt == NVFP4
        g = lin.group_size
        wv, ws = _weights_nk(lin)
        W = MX.dequant_blocks(wv, ws, g, nv).T
        U = MX.dequant_blocks(np.ones_like(wv), ws, g, nv).T
        row = np.ones(M)
        if in_dt == MXFP16:
            X = xq.float().cpu().numpy().astype(np.float64)
        elif in_dt == MXFP8 and c_mode == 2:
            X = MX.fp8_e4m3_decode(_bytes(xq)).astype(np.float64)
            row = sx.float().cpu().numpy().astype(np.float64).reshape(-1)
        elif in_dt == MXFP8:
            X = MX.dequant_blocks(MX.fp8_e4m3_decode(_bytes(xq)), _bytes(sx), g)[:M]
        else:
            X = MX.dequant_blocks(MX.fp4_unpack(_bytes(xq)), _bytes(sx), g, nv)[:M]
        return dict(X=X, W=W, U=U, row=row, col=np.ones(W.shape[1]), post=0.05 ** 2 if nv else 1.0)
    meta = lin.get_meta_args()
    e, wgm, csm = meta[4], meta[10], meta[9]
    s = O.to_f64(lin.scales.data) if lin.scales.numel() else None
    z = O.to_f64(lin.zeros.data).reshape(-1) if lin.zeros.numel() == 1 else (O.to_f64(lin.zeros.data) if lin.zeros.numel() else None)
    if e > 1:
        q = O.unpack_over_cols(lin.W_q.data.cpu().numpy(), lin.W_nbits, lin.W_q.element_size() * 8).T.astype(np.float64)
    else:
        q = O.to_f64(lin.W_q.data)
    one = lin.zeros.numel() == 1
    W = O.dequantize(q, s if wgm >= 2 else None, z if wgm in (1, 3, 4) else None, lin.group_size, wgm, one)
    U = O.dequantize(np.ones_like(q), s, None, lin.group_size, 2) if wgm >= 2 else np.ones_like(q)
    if F.kind == "a8wn" and p["act"] == FP8E4:
        W = O.round_to_dtype(W, meta[6] if (name.startswith("gemv_a8w") and M == 1) else O.FP8E4)
    N = W.shape[1]
    col = s.reshape(-1) if csm in (1, 3) else np.ones(N)
    row = sx.float().cpu().numpy().astype(np.float64).reshape(-1) if csm in (2, 3) else np.ones(M)
    return dict(X=O.to_f64(xq).reshape(M, -1), W=W, U=U, row=row, col=col, post=1.0)


def oracle_out(parts, X=None, W=None):
    X = parts["X"] if X is None else X
    W = parts["W"] if W is None else W
    return (X @ W) * parts["row"][:, None] * parts["col"][None, :] * parts["post"]


def is_exact(fam):
    """int8 activations on int8 / ternary weights: exact integer accumulation, compared bit for bit"""
    F = FAMILIES[fam]
    return F.kind in ("a8w8", "a8wn") and F.params["act"] == INT8


def exact_out(parts, tdt):
    """fp16 / bf16 ((integer dot) * (s_x * s_w)) in fp32 — the epilogue's operation order (tests/test_gpu_parity.py, the BitNet int8 test)"""
    import numpy as np
    import torch
    dot = parts["X"] @ parts["W"]
    assert float(np.abs(dot).max()) < (1 << 24) and np.array_equal(dot, np.round(dot)), "not an exact integer dot in fp32"
    sc = torch.from_numpy(parts["row"]).float()[:, None] * torch.from_numpy(parts["col"]).float()[None, :]
    return (torch.from_numpy(dot).float() * sc).to(torch_dtype(tdt))


def gate(fam, ref, tdt):
    """the element-wise gate of the family's checker at `ref`: atol + rtol |ref| with the family tests' constants"""
    import numpy as np
    if FAMILIES[fam].kind == "mx":
        from tests.test_mx_gpu import REL_TOL as REL_MX
        tol = REL_MX[torch_dtype(tdt)]
    else:
        from tests.test_gpu_parity import REL_TOL as REL_INT
        tol = REL_INT[tdt]
    return 10 * tol * max(float(np.abs(ref).mean()), 1e-12) + 4 * tol * np.abs(ref)


def check(fam, tdt, tag, y, ref, parts=None):
    """The comparison of tests/test_kernel_forms_gpu.py: the family's own gates, unchanged — `_compare` of tests/test_gpu_parity.py (REL_TOL, the
    element-wise gate; mean |err| < 1e-3, or 5e-3 with fp8 operands, like there), `_check` of tests/test_mx_gpu.py for the block-scaled families,
    bit for bit for int8 x int8.  y: a torch tensor [M, N] of the layer's 16-bit type.  Raises AssertionError."""
    import torch
    F = FAMILIES[fam]
    assert tuple(y.shape) == tuple(ref.shape) and y.dtype == torch_dtype(tdt), (tag, tuple(y.shape), y.dtype)
    assert bool(torch.isfinite(y).all()), tag
    if F.kind == "mx":
        from tests.test_mx_gpu import _check
        return _check(tag, y, ref, torch_dtype(tdt))
    from tests.test_gpu_parity import _compare
    if is_exact(fam):
        want = exact_out(parts, tdt)
        assert torch.equal(y.cpu(), want), (tag, float((y.cpu().float() - want.float()).abs().max()))
    if F.kind == "a8wn":
        abs_gate = None      # (as the family's tests have it)
    else:
        abs_gate = 5e-3 if (F.kind == "a16w8" or F.params.get("act") in (FP8E4, FP8E5)) else 1e-3
    from tests.test_gpu_parity import REPORT
    n = len(REPORT)
    try:
        return _compare(tag, y, ref, tdt, abs_gate=abs_gate)
    finally:
        del REPORT[n:]   # (the records of that module's own report file stay its own)


def build_case(row, device):
    """Everything one frozen row needs: the layer, the 16-bit activations, what the matmul reads (x, scales_x; the quantiser's output unless the row is a
    fused-quantiser one) and the quantised pair the oracle is evaluated on."""
    fam, tdt = row["family"], (FP16 if row["tdt"] == "fp16" else BF16)
    lin = build_layer(fam, tdt, row["N"], row["K"], device)
    x = make_x(tdt, row["M"], row["K"], device)
    xq, sx = quantise_x(fam, x)
    fused = bool(FAMILIES[fam].params.get("fused"))
    return dict(fam=fam, tdt=tdt, lin=lin, x=x, xq=xq, sx=sx, fused=fused, x_in=x if fused else xq, sx_in=None if fused else sx)


def call_args(row, case, out_ptr=0x1000):
    """the request of the row on the case's real tensors, as core._hip_matmul builds it"""
    from gemlite_amd.core import _call_args
    lin = case["lin"]
    return _call_args(case["x_in"], lin.W_q, lin.scales, lin.zeros, case["sx_in"], lin.get_meta_args(), row["matmul_type"], tuple(row["tuning"]), case["fused"],
                      out_ptr, (row["N"], 1))


def wrong_results(fam, tdt, parts):
    """{what: y} — the oracle's result as the layer's 16-bit type, and copies a subtly wrong kernel would give: one element off by twice the element-wise
    gate (one unit in the last place where the comparison is bit for bit), two rows swapped, one column computed with zero point + 1 (every weight
    of the column one code step lower; formats without a zero point: the column under its neighbour's scales, or, without any metadata, holding its
    neighbour's result), the last K group dropped."""
    import numpy as np
    import torch
    tt = torch_dtype(tdt)
    exact = is_exact(fam)

    def as_y(ref, p=parts):
        return exact_out(p, tdt) if exact and p is not None else torch.from_numpy(ref).to(tt)

    ref = oracle_out(parts)
    M, N = ref.shape
    K = parts["X"].shape[1]
    out = {"clean": as_y(ref)}
    # the column: the largest of those whose right-hand neighbour has float weights 1.7^4 times smaller (build_layer), so that no near-zero output hides the change
    i, j = M // 2, max(range(4, N - 1, 5), key=lambda c: float(np.abs(ref[:, c]).min()))
    one = out["clean"].clone()
    if exact:
        one.view(torch.int16)[i, j] += 1
    else:
        one[i, j] = float(ref[i, j] + 2 * gate(fam, ref, tdt)[i, j])
    out["one element"] = one
    if M >= 2:
        sw = out["clean"].clone()
        sw[[0, M - 1]] = sw[[M - 1, 0]]
        out["rows swapped"] = sw
    W2 = parts["W"].copy()
    if FAMILIES[fam].kind in ("a16wn", "a8wn"):
        W2[:, j] -= parts["U"][:, j]
        out["zero point + 1"] = as_y(oracle_out(parts, W=W2), dict(parts, W=W2))
    elif FAMILIES[fam].kind == "f16":   # no metadata at all: the column holds its neighbour's result
        nb = out["clean"].clone()
        nb[:, j] = nb[:, j + 1]
        out["neighbour's column"] = nb
    else:   # no zero point in the format: the column's codes under the scales of the column next to it — block scales, or the channel scale of the epilogue
        jn = j + 1
        W2[:, j] = W2[:, j] / parts["U"][:, j] * parts["U"][:, jn]
        col2 = parts["col"].copy()
        col2[j] = col2[jn]
        p2 = dict(parts, W=W2, col=col2)
        out["neighbour's scales"] = as_y(oracle_out(p2), p2)
    g = FAMILIES[fam].params.get("gs") or 32
    X2 = parts["X"].copy()
    X2[:, K - g:] = 0
    out["last group dropped"] = as_y(oracle_out(parts, X=X2), dict(parts, X=X2))
    return ref, out


if __name__ == "__main__" and "--write" in sys.argv:
    write()
