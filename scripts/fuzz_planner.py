"""CPU-only fuzz of the planner through the C ABI (gemlite_hip_query / kernel_name / workspace_bytes never launch): random layer
families x M x (N, K) x tuning.  Checks: no crash, a kernel name and a sane workspace for every accepted request, and — on
"realistic" shapes (N % 128 == 0, K % 256 == 0, both >= 1024) with default tuning — which requests still reach a coverage kernel.
    python scripts/fuzz_planner.py [seed] [iterations]
    python scripts/fuzz_planner.py --dump FILE [--lib OTHER_BUILD.so] [--seed S] [--iters N]     (see below: comparing two builds)"""
import collections, ctypes as C, os, random, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from gemlite_amd import _hip  # noqa: E402
import test_host_cpu as T  # noqa: E402

FAMS = {"a16w4": dict(), "a16w2": dict(nbits=2), "a16w1": dict(nbits=1), "a16w8p": dict(nbits=8), "a16w4bf": dict(in_dt=2),
        "a16w8i": dict(nbits=8, e=1, in_dt=1, w_dtype=4, w_mode=2, gsK=1), "a16w8f": dict(nbits=8, e=1, in_dt=2, w_dtype=3, w_mode=0, c_mode=1, gsK=1),
        "a8w8i": dict(nbits=8, e=1, in_dt=4, w_mode=0, c_mode=3, out_dt=1, gsK=1), "a8w8f": dict(nbits=8, e=1, in_dt=3, w_mode=0, c_mode=3, out_dt=2, gsK=1),
        "a8w4": dict(in_dt=3, out_dt=2, meta_dt=2, zeros_dt=2, w_mode=4, c_mode=2), "a8w2": dict(nbits=2, in_dt=3, out_dt=1, meta_dt=1, zeros_dt=1, w_mode=3, c_mode=2),
        "bitnet8": dict(nbits=2, in_dt=4, out_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=3, gsK=1),
        "bitnet16": dict(nbits=2, in_dt=1, meta_dt=0, zeros_dt=6, zero_scalar=1, w_mode=1, c_mode=1, gsK=1)}
MXF = {"mx88": (16, 8, 4, 32), "mx84": (16, 4, 2, 32), "mx84b": (16, 4, 4, 32), "mx44": (17, 4, 4, 32), "mx16w8": (15, 8, 0, 32), "mx16w4": (14, 4, 0, 32),
       "nv": (18, 4, 4, 16), "mx88pt": (16, 8, 2, 32)}
DIMS = [1, 2, 3, 4, 5, 8, 16, 17, 22, 23, 32, 33, 40, 48, 64, 65, 96, 128, 200, 256, 300, 384, 385, 512, 513, 700, 1024, 2048, 4096]
NK = [64, 128, 192, 256, 512, 1024, 1280, 1536, 2048, 2560, 3072, 4096, 4224, 5120, 8192, 8960, 11008, 13824, 14336, 16384, 28672]
TUN = [0, 1, 2, 3, 4, 5, 6, 7, 8, 32, 34]


def run(seed=0, iters=100000, lib=None):
    """-> (kernels chosen, {family: [(M, N, K) realistic default-tuning requests on a coverage kernel]})"""
    lib = lib or _hip.load()
    rnd = random.Random(seed)
    buf = (C.c_uint8 * 64)()
    ptr = C.addressof(buf) // 16 * 16 + 16
    cnt, cov = collections.Counter(), collections.defaultdict(list)
    for _ in range(iters):
        M, N, K = rnd.choice(DIMS), rnd.choice(NK), rnd.choice(NK)
        tun = tuple(rnd.choice(TUN) if rnd.random() < 0.15 else 0 for _ in range(3)) + (rnd.choice([0, 0, 0, 16, 64, 128, 1024, 2048, 4096, 16384]),)
        if rnd.random() < 0.5:
            tun = (0, 0, 0, 0)
        if rnd.random() < 0.6:
            f = rnd.choice(list(FAMS))
            kw = dict(FAMS[f])
            gsk = kw.pop("gsK", 0)
            gs = K if gsk else rnd.choice([32, 64, 128, 128, 256])
            if K % gs:
                continue
            a = T._args(M=M, N=N, K=K, gs=gs, tuning=tun, mt=rnd.choice([-1, -1, -1, 0, 1, 2, 3, 4]) if any(tun) else -1, **kw)
            if kw.get("c_mode", 0) in (2, 3):
                a.scales_x = 0x1000
            f += "" if gsk else "/g%d" % gs
        else:
            f = rnd.choice(list(MXF))
            in_dt, nbits, c_mode, group = MXF[f]
            if K % group:
                continue
            a = _hip.ForwardArgs()
            a.struct_size = C.sizeof(_hip.ForwardArgs)
            a.matmul_type = -1
            a.x = a.w_q = a.scales = a.out = a.scales_x = ptr
            a.M, a.N, a.K = M, N, K
            a.W_nbits, a.group_size, a.unpack_mask = nbits, group, 2 ** nbits - 1
            a.elements_per_sample = 1 if nbits == 8 else 2
            a.w_pack_bits = 0 if nbits == 8 else 8
            a.w_dtype = 3 if nbits == 8 else 5
            a.input_dtype, a.output_dtype, a.meta_dtype = in_dt, (1 if in_dt in (14, 18) else 2), 5
            a.channel_scale_mode, a.W_group_mode = c_mode, 0
            a.stride_xm, a.stride_xk = (K // 2 if in_dt in (17, 18) else K), 1
            a.stride_wk, a.stride_wn = 1, (K if nbits == 8 else K // 2)
            a.stride_om, a.stride_on = N, 1
            a.stride_meta_g, a.stride_meta_n = N, 1
            a.stride_sx_m = K // group if c_mode == 4 else 1
            for i in range(4):
                a.tuning[i] = tun[i]
        st = lib.gemlite_hip_query(C.byref(a))
        cnt["status %d" % st] += 1
        if st != 0:
            continue
        name = lib.gemlite_hip_kernel_name(C.byref(a)).decode()
        ws = lib.gemlite_hip_workspace_bytes(C.byref(a))
        assert name and ws < (1 << 36), (f, M, N, K, tun, name, ws)
        cnt[name.split("<")[0]] += 1
        if "generic" in name and not any(tun) and N % 128 == 0 and K % 256 == 0 and N >= 1024 and K >= 1024:
            cov[f].append((M, N, K))
    return cnt, cov


# ---- --dump FILE: one line per request with everything the host queries say about it.  Two builds of the library plan alike exactly
# when their dumps are byte-identical (a refactor of the planner is checked this way: same script, `--lib` names the other build).
# Part 1 is the full product FAMS / MXF x DIMS x NK x NK x group sizes at default tuning; part 2 is `iters` seeded random requests that
# also vary what the resolver branches on and run() leaves alone (see _random_request).
FLAG_BITS = [1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 16384, 32768, 65536, 131072, 262144, 524288, 1048576, 2097152, 4194304]
ODD_NK = [896, 1000, 4100, 4112, 4160, 4352, 4608, 4864, 9728]
GROUPS = [32, 64, 128, 256]
ALL_TUN = TUN + [9, 10, 16, 20]
_FIELDS = [n for n, _ in _hip.ForwardArgs._fields_ if n not in ("struct_size", "workspace", "workspace_bytes", "tuning")]


def _fam_args(f, M, N, K, gs, tun=(0, 0, 0, 0), mt=-1):
    kw = dict(FAMS[f])
    kw.pop("gsK", 0)
    a = T._args(M=M, N=N, K=K, gs=gs, tuning=tun, mt=mt, **kw)
    if kw.get("c_mode", 0) in (2, 3):
        a.scales_x = 0x1000
    return a


def _mx_args(f, M, N, K, tun=(0, 0, 0, 0), mt=-1):
    in_dt, nbits, c_mode, group = MXF[f]
    a = _hip.ForwardArgs()
    a.struct_size = C.sizeof(_hip.ForwardArgs)
    a.matmul_type = mt
    a.x = a.w_q = a.scales = a.out = a.scales_x = 0x1000
    a.M, a.N, a.K = M, N, K
    a.W_nbits, a.group_size, a.unpack_mask = nbits, group, 2 ** nbits - 1
    a.elements_per_sample = 1 if nbits == 8 else 2
    a.w_pack_bits = 0 if nbits == 8 else 8
    a.w_dtype = 3 if nbits == 8 else 5
    a.input_dtype, a.output_dtype, a.meta_dtype = in_dt, (1 if in_dt in (14, 18) else 2), 5
    a.channel_scale_mode, a.W_group_mode = c_mode, 0
    a.stride_xm, a.stride_xk = (K // 2 if in_dt in (17, 18) else K), 1
    a.stride_wk, a.stride_wn = 1, (K if nbits == 8 else K // 2)
    a.stride_om, a.stride_on = N, 1
    a.stride_meta_g, a.stride_meta_n = N, 1
    a.stride_sx_m = K // group if c_mode == 4 else 1
    for i in range(4):
        a.tuning[i] = tun[i]
    return a


def _random_request(rnd):
    """A request of the random part: TUN and more in tuning[0 .. 2], every matmul type, the named tuning[3] bits, and — each with a small
    probability — pointers off 16-byte alignment, odd / non-unit strides, 8- and 16-bit packed words, group sizes 96 / 160, the
    fused-quant requests (16-bit x, the layer's type in type_id, scales_x NULL) and M above 65535."""
    M = rnd.choice(DIMS) if rnd.random() < 0.97 else rnd.choice([65536, 70000, 100000])
    N = rnd.choice(NK) if rnd.random() < 0.9 else rnd.choice(ODD_NK)
    K = rnd.choice(NK) if rnd.random() < 0.9 else rnd.choice(ODD_NK)
    tun = [rnd.choice(ALL_TUN) if rnd.random() < 0.15 else 0 for _ in range(3)] + [0]
    for _ in range(rnd.choice([0, 0, 1, 1, 2, 3])):
        tun[3] |= rnd.choice(FLAG_BITS)
    if rnd.random() < 0.1:
        tun[3] |= rnd.randrange(1, 16) << 24
    if rnd.random() < 0.4:
        tun = [0, 0, 0, 0]
    mt = rnd.choice([-1, -1, -1, 0, 1, 2, 3, 4])
    if rnd.random() < 0.7:
        f = rnd.choice(list(FAMS))
        gs = K if "gsK" in FAMS[f] else rnd.choice(GROUPS + [128, 96, 160])
        a = _fam_args(f, M, N, K, gs, tun, mt)
        if a.elements_per_sample > 1 and rnd.random() < 0.1:  # 8- / 16-bit packed words
            a.w_pack_bits = rnd.choice([8, 16])
            a.elements_per_sample = a.w_pack_bits // a.W_nbits
        if a.channel_scale_mode in (2, 3) and rnd.random() < 0.3:  # the quantiser inside the launch: raw 16-bit x
            a.type_id = a.input_dtype * 100 + a.W_nbits
            if a.elements_per_sample == 1:
                a.w_dtype = a.input_dtype
            a.input_dtype = rnd.choice([1, 2])
            if rnd.random() < 0.8:
                a.output_dtype = a.input_dtype
            a.scales_x = None
    else:
        f = rnd.choice(list(MXF))
        a = _mx_args(f, M, N, K, tun, mt)
        if a.channel_scale_mode in (2, 4) and rnd.random() < 0.3:
            a.type_id = a.input_dtype * 100 + a.W_nbits
            a.input_dtype = rnd.choice([1, 2])
            a.stride_xm = K
            a.scales_x = None
    if rnd.random() < 0.05:
        a.x += rnd.choice([2, 8])
    if rnd.random() < 0.05:
        a.w_q += rnd.choice([2, 8])
    if rnd.random() < 0.05:
        a.out += rnd.choice([2, 8])
    if rnd.random() < 0.05:
        a.stride_xm += rnd.choice([1, 4, 8, 16])
    if rnd.random() < 0.03:
        a.stride_xk = 2
    if rnd.random() < 0.03:
        a.stride_on = 2
    if rnd.random() < 0.03:
        a.stride_wn += rnd.choice([1, 8, 16])
    if rnd.random() < 0.03:
        a.stride_meta_n = 2
    return f, a


def _requests(seed, iters):
    for f in FAMS:
        for gs in ([0] if "gsK" in FAMS[f] else GROUPS):
            for M in DIMS:
                for N in NK:
                    for K in NK:
                        if gs and K % gs:
                            continue
                        yield f, _fam_args(f, M, N, K, gs or K)
    for f in MXF:
        for M in DIMS:
            for N in NK:
                for K in NK:
                    if K % MXF[f][3] == 0:
                        yield f, _mx_args(f, M, N, K)
    rnd = random.Random(seed)
    for _ in range(iters):
        yield _random_request(rnd)


def load_lib(path):
    """Another build of the library, with the prototypes of the host queries the dump uses."""
    lib = C.CDLL(path)
    p, e = C.POINTER(_hip.ForwardArgs), C.POINTER(_hip.ForwardExt)
    for name, res, args in (("gemlite_hip_query", C.c_int, [p]), ("gemlite_hip_kernel_name", C.c_char_p, [p]),
                            ("gemlite_hip_workspace_bytes", C.c_uint64, [p]), ("gemlite_hip_bias_fused", C.c_int, [p, e]),
                            ("gemlite_hip_kernel_name_ex", C.c_char_p, [p, e]), ("gemlite_hip_k_order_mode", C.c_int, [p])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def dump(path, seed=0, iters=1000000, lib=None):
    """-> (lines, kernel labels seen, statuses seen)"""
    lib = lib or _hip.load()
    ext = _hip.ForwardExt()
    ext.struct_size = C.sizeof(_hip.ForwardExt)
    ext.bias = 0x2000  # 16-bit aligned, never dereferenced
    names, statuses, n = set(), set(), 0
    with open(path, "w") as out:
        for f, a in _requests(seed, iters):
            ext.bias_dtype = a.output_dtype
            ra, re_ = C.byref(a), C.byref(ext)
            st = lib.gemlite_hip_query(ra)
            name = lib.gemlite_hip_kernel_name(ra).decode()
            name_ex = lib.gemlite_hip_kernel_name_ex(ra, re_).decode()
            out.write("%s %s %s | %d %s %d %d %s %d\n" % (
                f, " ".join("%d" % (getattr(a, k) or 0) for k in _FIELDS), " ".join("%d" % t for t in a.tuning),
                st, name, lib.gemlite_hip_workspace_bytes(ra), lib.gemlite_hip_bias_fused(ra, re_), name_ex, lib.gemlite_hip_k_order_mode(ra)))
            names.update((name, name_ex))
            statuses.add(st)
            n += 1
    return n, names, statuses


def pinned_labels():
    """Every kernel label tests/test_host_cpu.py pins (the '|ab' ones exist in A/B builds only)."""
    import re
    src = open(T.__file__).read()
    return {m for m in re.findall(r'"([a-z][a-z0-9_]*_kernel(?:<[^"|]*>)?)"', src)}


if __name__ == "__main__":
    if "--dump" in sys.argv:
        import hashlib
        argv = sys.argv[1:]
        path = argv[argv.index("--dump") + 1]
        lib = load_lib(argv[argv.index("--lib") + 1]) if "--lib" in argv else None
        seed = int(argv[argv.index("--seed") + 1]) if "--seed" in argv else 0
        iters = int(argv[argv.index("--iters") + 1]) if "--iters" in argv else 1000000
        n, names, statuses = dump(path, seed, iters, lib)
        h = hashlib.sha256()
        with open(path, "rb") as fh:
            for blk in iter(lambda: fh.read(1 << 20), b""):
                h.update(blk)
        print("lines", n, "sha256", h.hexdigest())
        print("statuses", sorted(statuses), "| pinned labels missing from the dump:", sorted(pinned_labels() - names))
        sys.exit(0)
    cnt, cov = run(int(sys.argv[1]) if len(sys.argv) > 1 else 0, int(sys.argv[2]) if len(sys.argv) > 2 else 100000)
    print(dict(cnt.most_common()))
    for f in sorted(cov):
        print("coverage kernel on realistic shapes:", f, len(cov[f]), sorted(set(m for m, _, _ in cov[f]))[:12])
