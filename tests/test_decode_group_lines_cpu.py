"""Host-only side of the lines of the grouped decode kernel (gl_common.h: decode3_group_lines, decode3_group_lines_default): a wave of a
grouped block works on H in {1, 2, 4} adjacent tiles of the block's tile group at once — its lanes are H sub-waves of 64 / H lanes — in H
passes over each virtual wave, and the block's LB * TB / H wave-slots take the place its slots had in gemlite_hip_capture_group_wave_split.
Against a restatement in Python.  No GPU."""
import ctypes as C
import os

import pytest

from gemlite_amd import _hip
from tests.test_decode_group_tiles_cpu import RESIDENT, ROOT, TILES, default_py, geometry_py, wave_split

NEW = ("gemlite_hip_capture_group_lines", "gemlite_hip_capture_group_last_lines")
FORCED = os.environ.get("GEMLITE_HIP_CAPTURE_GROUP_LINES", "")


def lines_py(tb, h_want):
    """H divides TB: a wanted H falls back 4 -> 2 -> 1."""
    h = 4 if h_want >= 4 else (2 if h_want >= 2 else 1)
    while h > tb:
        h //= 2
    return h


def default_lines_py(tiles, members, resident, tb):
    """The default rule (profiles/r18/decode_group_lines.log): whole lines wherever the block holds them — H = 2 for every TB >= 2 — and H = 4
    where TB = 4 and the fullest block holds four layers."""
    if tb < 2:
        return 1
    t, _, gy, _ = geometry_py(tiles, members, resident, tb, 0)
    return 4 if t == 4 and -(-members // gy) >= 4 else 2


def lines(tiles, members, resident, tb, h_want):
    return _hip.load().gemlite_hip_capture_group_lines(tiles, members, resident, tb, h_want)


def test_the_new_symbols_are_exported_and_declared():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in NEW:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    for doc in ("include/gemlite_hip.h", "README.md", "DESIGN.md"):
        assert "GEMLITE_HIP_CAPTURE_GROUP_LINES" in open(os.path.join(ROOT, doc)).read(), doc
    assert lib.gemlite_hip_capture_group_last_lines() == 0  # no grouped node in this process


def test_a_wanted_h_falls_back_to_what_tb_admits():
    for tiles in TILES:
        for members in (1, 2, 3, 5, 8, 16):
            for tb in (1, 2, 4):
                if tiles % tb:
                    assert lines(tiles, members, 256, tb, 4) == -1
                    continue
                for h_want in (1, 2, 4):
                    h = lines(tiles, members, 256, tb, h_want)
                    assert h == lines_py(tb, h_want) and h in (1, 2, 4) and h <= h_want and tb % h == 0
                assert [lines(tiles, members, 256, tb, w) for w in (1, 2, 4)] == {1: [1, 1, 1], 2: [1, 2, 2], 4: [1, 2, 4]}[tb]


def test_one_tile_per_block_is_one_tile_per_wave():
    for tiles in TILES:
        for members in range(1, 17):
            for resident in RESIDENT:
                assert [lines(tiles, members, resident, 1, w) for w in (0, 1, 2, 4)] == [1, 1, 1, 1]


def test_bad_arguments():
    for bad in ((0, 4, 256, 1, 1), (64, 0, 256, 1, 1), (64, 17, 256, 1, 1), (64, 4, 0, 1, 1), (64, 4, 256, 3, 1), (64, 4, 256, 8, 1),
                (64, 4, 256, 4, 3), (64, 4, 256, 4, 5), (64, 4, 256, 4, -1), (66, 4, 256, 4, 1)):
        assert lines(*bad) == -1, bad


def lane_of(h_count, lane, p):
    """(sub-wave h, c, row pair g, 16-lane DPP row of the whole wave) of `lane` in pass p under H = h_count"""
    per = 64 // h_count
    h, lq = lane // per, lane % per
    return h, lq & 3, p * (16 // h_count) + (lq >> 2), lane >> 4


def test_the_wave_slot_split_covers_every_slot_virtual_wave_and_pass_exactly_once():
    """What the kernel does with (wave, lane, pass): wave-slot ws = wave_split(slots / H, wave), sub-wave h fills slot ws * H + h; in pass p
    of virtual wave v the lane (h, c, gl) takes the row pair g = p * 16 / H + gl, and the four row pairs of a 16-lane DPP row are summed
    into partial row v * 4 + r of the slot's region, r = p * 4 / H + (DPP row inside the sub-wave).  Every (slot, v, g, c) is computed once,
    every row 4 r .. 4 r + 3 of row pairs meets in ONE DPP row with g ascending across its quads, and every partial row (slot, v * 4 + r)
    is written exactly once — also by the wave-slots of a short K, whose empty (v, p) write zeros."""
    for tb in (1, 2, 4):
        for lb in range(1, 16 // tb + 1):
            slots = lb * tb
            for h_count in (1, 2, 4):
                if h_count > tb:
                    continue
                assert slots % h_count == 0
                work, rows = {}, {}
                for wave in range(16):
                    ws, v0, v1 = wave_split(slots // h_count, wave)
                    if ws < 0:
                        continue
                    assert (ws * h_count) // tb == (ws * h_count + h_count - 1) // tb  # a run of H tiles stays inside one layer
                    for v in range(v0, v1):
                        for p in range(h_count):
                            dpp = {}
                            for lane in range(64):
                                h, c, g, row = lane_of(h_count, lane, p)
                                slot = ws * h_count + h
                                assert 0 <= g < 16 and slot < slots
                                assert (slot, v, g, c) not in work
                                work[(slot, v, g, c)] = 1
                                dpp.setdefault((row, c), []).append((slot, g))
                            for (row, c), members in dpp.items():
                                slot = members[0][0]
                                gs = [g for s, g in members]
                                assert all(s == slot for s, _ in members) and gs == list(range(gs[0], gs[0] + 4)) and gs[0] % 4 == 0
                                r = p * (4 // h_count) + row % (4 // h_count)
                                assert r == gs[0] // 4
                                if c == 0:
                                    assert (slot, v * 4 + r) not in rows
                                    rows[(slot, v * 4 + r)] = 1
                assert set(work) == {(s, v, g, c) for s in range(slots) for v in range(16) for g in range(16) for c in range(4)}, (tb, lb, h_count)
                assert set(rows) == {(s, q) for s in range(slots) for q in range(64)}, (tb, lb, h_count)


def test_the_metadata_row_of_a_pass_splits_exactly():
    """Row pair g = p * 16 / H + gl of chunk gc starts at K index 256 gc + 16 g; its group is (256 gc + 16 g) >> log2(group).  The kernel adds
    three parts: the chunk's (scalar), the pass's (scalar: (256 / H p) >> s) and the lane's (vector, fixed: 16 gl >> s)."""
    for s in range(4, 13):
        for h_count in (1, 2, 4):
            for gc in range(5):
                for p in range(h_count):
                    for gl in range(16 // h_count):
                        g = p * (16 // h_count) + gl
                        chunk = (gc << 8) >> s if s <= 8 else gc >> (s - 8)
                        lane = (16 * gl) >> s if s < 8 else 0
                        ps = ((p << 8) // h_count) >> (s if s < 8 else 31)
                        assert chunk + ps + lane == (256 * gc + 16 * g) >> s, (s, h_count, gc, p, gl)


def test_what_a_capture_picks():
    """h_want = 0: the default rule, or what GEMLITE_HIP_CAPTURE_GROUP_LINES forces (read once per process), after the fallback."""
    for tiles in TILES:
        for members in range(1, 17):
            for resident in RESIDENT:
                for tb in (1, 2, 4):
                    if tiles % tb:
                        continue
                    h = lines(tiles, members, resident, tb, 0)
                    if FORCED:
                        assert h == lines_py(tb, int(FORCED))
                    else:
                        assert h == lines_py(tb, default_lines_py(tiles, members, resident, tb)), (tiles, members, resident, tb)


def test_the_default_rule_at_the_measured_shapes():
    """256 tiles on 256 CUs (profiles/r18/decode_group_lines.log §4 - §6), under the TB the tile rule takes for each member count: H = 1 for 3
    members (TB = 1); H = 2 for 2, 5, 6 (TB = 2) and for 4, 7, 8, 10, 12 (TB = 4, one to three layers in the fullest block: H = 4 was slower
    than H = 2 there); H = 4 for 15 and 16 (four layers per block).  Twelve layers of 256 tiles x K = 11008 share the geometry of 12 members."""
    measured = {2: (2, 2), 3: (1, 1), 4: (4, 2), 5: (2, 2), 6: (2, 2), 7: (4, 2), 8: (4, 2), 10: (4, 2), 12: (4, 2), 15: (4, 4), 16: (4, 4)}
    for members, (tb, h) in measured.items():
        assert default_py(256, members, 256)[0] == tb
        assert lines_py(tb, default_lines_py(256, members, 256, tb)) == h, members
        if not FORCED:
            assert lines(256, members, 256, tb, 0) == h, members
    assert [default_lines_py(256, m, 256, 4) for m in (13, 14)] == [4, 4]  # (not measured: four layers in the fullest block, as 15 and 16)
    # 64 tiles, 16 members (one layer x 4 tiles per block): one wave-slot per block under H = 4, so H = 2
    assert default_py(64, 16, 256)[:3] == (4, 16, 16) and default_lines_py(64, 16, 256, 4) == 2
    assert all(default_lines_py(t, m, r, 1) == 1 for t in TILES for m in range(1, 17) for r in RESIDENT)
