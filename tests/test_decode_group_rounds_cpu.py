"""Host-only side of the ROUNDS of a grouped decode node (gl_common.h: decode3_round_member; capture_group.hip, ROUNDS): a node of R
rounds of m members each runs as grid (grid.x, Y * R), and block row yy holds, as its block-local layer li, member
m * (yy // Y) + yy % Y + li * Y of the node's table.  The exported rule is the function the kernel calls.  No GPU."""
import ctypes as C
import os
import subprocess
import sys

from gemlite_amd import _hip
from tests.test_decode_group_tiles_cpu import ROOT

NEW = ("gemlite_hip_capture_group_merge_stats", "gemlite_hip_capture_group_rounds_max", "gemlite_hip_capture_group_last_rounds",
       "gemlite_hip_capture_group_round_member")
SWITCH = "GEMLITE_HIP_CAPTURE_GROUP_ROUNDS"
NODE_MAX, GMAX, RESIDENT = 64, 16, 256
TILES = (4, 64, 256, 688)


def member(m, Y, block_y, li):
    return _hip.load().gemlite_hip_capture_group_round_member(m, Y, block_y, li)


def grid_ys(m):
    """Every grid.y per round that decode3_group_geometry gives m members: the four tile counts, every TB asked for and the default"""
    lib, out, ys = _hip.load(), (C.c_int32 * 4)(), set()
    for tiles in TILES:
        for tb_want in (0, 1, 2, 4):
            assert lib.gemlite_hip_capture_group_geometry(tiles, m, RESIDENT, tb_want, 0, C.byref(out)) == 0
            ys.add(out[2])
    return sorted(ys)


def test_the_new_symbols_are_exported_and_declared():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in NEW:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    for doc in ("include/gemlite_hip.h", "README.md", "DESIGN.md", "INTEGRATION.md", "scripts/README.md"):
        assert SWITCH in open(os.path.join(ROOT, doc)).read(), doc
    assert 0 <= lib.gemlite_hip_capture_group_last_rounds() <= lib.gemlite_hip_capture_group_rounds_max()
    merged = C.c_uint64(1 << 63)
    lib.gemlite_hip_capture_group_merge_stats(C.byref(merged))
    assert merged.value < 1 << 63  # (written: a count of this process)
    lib.gemlite_hip_capture_group_merge_stats(None)


def test_every_member_of_a_node_is_visited_exactly_once():
    cells = 0
    for m in range(1, GMAX + 1):
        ys = grid_ys(m)
        assert ys and all(1 <= Y <= m for Y in ys), (m, ys)
        for Y in ys:
            for R in range(1, NODE_MAX // m + 1):
                seen = []
                for block_y in range(Y * R):
                    y = block_y % Y
                    for li in range((m - y + Y - 1) // Y):  # the layers the kernel gives this block: ceil((m - y) / Y)
                        got = member(m, Y, block_y, li)
                        assert got == m * (block_y // Y) + y + li * Y, (m, Y, R, block_y, li, got)
                        seen.append(got)
                assert sorted(seen) == list(range(m * R)), (m, Y, R)
                cells += 1
    assert cells > 16 * 4  # (every m had its rounds, several Y among them)


def test_a_node_of_one_round_is_the_index_it_always_was():
    for m in range(1, GMAX + 1):
        for Y in grid_ys(m):
            for y in range(Y):
                for li in range((m - y + Y - 1) // Y):
                    assert member(m, Y, y, li) == y + li * Y


def test_bad_arguments():
    for bad in ((0, 1, 0, 0), (17, 1, 0, 0), (-1, 1, 0, 0), (4, 0, 0, 0), (4, 5, 0, 0), (4, -1, 0, 0), (4, 2, -1, 0), (4, 2, 0, -1),
                (4, 2, 0, 2),     # block row 0 of Y = 2 holds the layers 0 and 2: local layers 0 and 1
                (4, 2, 1, 2),
                (5, 2, 1, 2),     # row 1 of five members: 1 and 3
                (16, 4, 16, 0),   # the fifth round of 16: past 64 members
                (16, 16, 64, 0),
                (1, 1, 64, 0),
                (3, 1, 21, 0),    # 21 rounds of 3 fit, the 22nd does not
                (4, 2, 2 ** 31 - 1, 0), (4, 2, 0, 2 ** 31 - 1)):
        assert member(*bad) == -1, bad
    assert member(5, 2, 0, 2) == 4 and member(16, 4, 15, 3) == 63 and member(1, 1, 63, 0) == 63 and member(3, 1, 20, 2) == 62
    assert member(16, 16, 63, 0) == 63


def _child(env_extra):
    env = dict(os.environ)
    for k in (SWITCH, "GEMLITE_HIP_CAPTURE_GROUP_MAX", "GEMLITE_HIP_NO_CAPTURE_GROUPS"):
        env.pop(k, None)
    env.update(env_extra)
    # (the library alone: the child does not need the package, and the switches are the library's)
    code = ("import ctypes, sys; lib = ctypes.CDLL(sys.argv[1]); "
            "print('LIMITS', lib.gemlite_hip_capture_group_rounds_max(), lib.gemlite_hip_capture_group_max())")
    _hip.load()
    out = subprocess.run([sys.executable, "-c", code, _hip.LIB_PATH], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("LIMITS ")][-1].split()
    return int(line[1]), int(line[2])


def test_the_limits_fit_the_table():
    lib = _hip.load()
    rounds, gmax = lib.gemlite_hip_capture_group_rounds_max(), lib.gemlite_hip_capture_group_max()
    assert rounds >= 1 and rounds * gmax <= NODE_MAX and gmax <= GMAX


def test_the_switches():
    """Read once per process: every setting in a child of its own."""
    assert _child({SWITCH: "1"}) == (1, GMAX)  # merging off, grouping as before
    assert _child({"GEMLITE_HIP_NO_CAPTURE_GROUPS": "1"}) == (1, 1)
    for asked, got in (("2", 2), ("3", 3), ("4", 4), ("9", 4), ("0", 1)):
        assert _child({SWITCH: asked})[0] == got, asked
    rounds, gmax = _child({"GEMLITE_HIP_CAPTURE_GROUP_MAX": "3"})
    assert gmax == 3 and 1 <= rounds <= 4
