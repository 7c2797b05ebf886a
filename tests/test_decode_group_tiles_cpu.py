"""Host-only side of the tile groups of the grouped decode kernel (gl_common.h: decode3_group_geometry, decode3_group_first_tile): a
block holds TB in {1, 2, 4} adjacent 16-column tiles x LB layers, grid (tiles / TB, Y), and its LB * TB (layer, tile) slots take the place
the layers have in gemlite_hip_capture_group_wave_split.  Against a restatement in Python.  No GPU."""
import ctypes as C
import functools
import os

import pytest

from gemlite_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gemlite_hip_capture_group_geometry", "gemlite_hip_capture_group_tile_of")
TILES = list(range(1, 65)) + [256, 688, 1024]
RESIDENT = [8, 64, 256, 304]
FORCED = os.environ.get("GEMLITE_HIP_CAPTURE_GROUP_TILES", "")


def grid_y(groups, members, resident):
    return max(1, min(resident // groups, members))


def geometry_py(tiles, members, resident, tb_want, span):
    """The largest TB <= tb_want with tiles % TB == 0 and ceil(members / Y) * TB <= 16, Y from the tile GROUPS."""
    for tb in (4, 2):
        if tb > tb_want or tiles % tb:
            continue
        y = grid_y(tiles // tb, members, resident)
        if -(-members // y) * tb <= 16:
            return tb, tiles // tb, y, span
    return 1, tiles, grid_y(tiles, members, resident), span


def geometry(tiles, members, resident, tb_want, span):
    out = (C.c_int32 * 4)()
    assert _hip.load().gemlite_hip_capture_group_geometry(tiles, members, resident, tb_want, span, C.byref(out)) == 0
    return tuple(out)


def tile_of(tiles, tb, span, block):
    return _hip.load().gemlite_hip_capture_group_tile_of(tiles, tb, span, block)


@functools.lru_cache(maxsize=None)
def wave_split(slots, wave):
    out = (C.c_int32 * 3)()
    _hip.load().gemlite_hip_capture_group_wave_split(slots, wave, C.byref(out))
    return tuple(out)


def test_the_new_symbols_are_exported_and_declared():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in NEW:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    assert "GEMLITE_HIP_CAPTURE_GROUP_TILES" in header
    assert "GEMLITE_HIP_CAPTURE_GROUP_TILES" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


@pytest.mark.parametrize("resident", RESIDENT, ids=lambda r: f"cu{r}")
def test_geometry_obeys_the_constraints(resident):
    for tiles in TILES:
        for members in range(1, 17):
            for tb_want in (1, 2, 4):
                for span in (0, 1):
                    tb, gx, gy, sp = got = geometry(tiles, members, resident, tb_want, span)
                    assert got == geometry_py(tiles, members, resident, tb_want, span), (tiles, members, resident, tb_want, span)
                    assert tb in (1, 2, 4) and tb <= tb_want and tiles % tb == 0 and gx * tb == tiles and sp == span
                    assert gy == grid_y(gx, members, resident) and 1 <= gy <= members
                    assert -(-members // gy) * tb <= 16  # the slots of the fullest block (y = 0)
                    if tb < tb_want:  # the TB asked for, and every one between, was refused for a reason
                        for t in (4, 2):
                            if tb < t <= tb_want:
                                assert tiles % t or -(-members // grid_y(tiles // t, members, resident)) * t > 16


@pytest.mark.parametrize("resident", RESIDENT, ids=lambda r: f"cu{r}")
def test_blocks_and_slots_cover_every_layer_and_tile_exactly_once(resident):
    """What the kernel does with (blockIdx, wave): slot = wave_split(LB * TB, wave), layer y + (slot / TB) * Y on tile tile_of(block) + slot % TB;
    waves 0 .. slots - 1 finish slot `wave`.  Both the items (virtual waves 0 .. 15 of every (layer, tile)) and the epilogues cover the
    launch exactly once."""
    for tiles in TILES:
        if tiles > 64 and resident not in (256, 304):
            continue  # (the wide ones on the two real CU counts: the enumeration is 16 waves x every block)
        for members in (1, 2, 3, 5, 7, 8, 11, 16) if tiles > 16 else range(1, 17):
            for tb_want in (1, 2, 4):
                for span in (0, 1):
                    tb, gx, gy, _ = geometry(tiles, members, resident, tb_want, span)
                    work, fin = {}, set()
                    for b in range(gx):
                        t0 = tile_of(tiles, tb, span, b)
                        assert t0 >= 0 and t0 % tb == 0
                        for y in range(gy):
                            slots = -(-(members - y) // gy) * tb
                            assert 1 <= slots <= 16
                            for wave in range(16):
                                s, v0, v1 = wave_split(slots, wave)
                                if s >= 0:
                                    key = (y + (s // tb) * gy, t0 + s % tb)
                                    for v in range(v0, v1):
                                        assert (key, v) not in work
                                        work[(key, v)] = 1
                                if wave < slots:
                                    key = (y + (wave // tb) * gy, t0 + wave % tb)
                                    assert key not in fin
                                    fin.add(key)
                    want = {(l, t) for l in range(members) for t in range(tiles)}
                    assert fin == want, (tiles, members, resident, tb_want, span)
                    assert set(work) == {(k, v) for k in want for v in range(16)}, (tiles, members, resident, tb_want, span)


def test_tile_of_is_a_permutation_under_both_placements():
    for tiles in TILES + [8, 16, 24, 40, 48, 80, 96, 136, 2048]:
        for tb in (1, 2, 4):
            if tiles % tb:
                assert tile_of(tiles, tb, 0, 0) == -1
                continue
            groups = tiles // tb
            for span in (0, 1):
                firsts = [tile_of(tiles, tb, span, b) for b in range(groups)]
                assert sorted(firsts) == [g * tb for g in range(groups)], (tiles, tb, span)
                if span and groups % 8 == 0:  # XCD x = block % 8 takes the contiguous groups [x G / 8, (x + 1) G / 8)
                    for b, f in enumerate(firsts):
                        assert f // tb == (b % 8) * (groups // 8) + b // 8
                elif span or tb > 1 or tiles % 16:  # the identity
                    assert firsts == [g * tb for g in range(groups)]
                else:  # the pair map: XCD x takes both halves of the lines 8 m + x
                    for b, f in enumerate(firsts):
                        assert f == ((b // 16) * 8 + b % 8) * 2 + (b // 8) % 2
            assert tile_of(tiles, tb, 0, groups) == -1 and tile_of(tiles, tb, 0, -1) == -1
    assert tile_of(0, 1, 0, 0) == -1 and tile_of(64, 3, 0, 0) == -1


def test_one_tile_per_block_with_the_pair_map_is_the_grid_there_was():
    """TB = 1: grid (tiles, gemlite_hip_capture_group_grid_y) and, for tiles % 16 == 0, the pair map of the single-layer kernel."""
    lib = _hip.load()
    for tiles in TILES:
        for members in range(1, 17):
            assert geometry(tiles, members, 256, 1, 0) == (1, tiles, lib.gemlite_hip_capture_group_grid_y(tiles, members), 0)
        for b in range(tiles):
            xcd, idx = b & 7, b >> 3
            assert tile_of(tiles, 1, 0, b) == ((((idx >> 1) << 3) + xcd) * 2 + (idx & 1) if tiles % 16 == 0 else b)


def test_the_benchmark_shape():
    """256 tiles, 16 members, 256 CUs: every candidate fills the 256 CUs with blocks of 16 slots, one wave each."""
    assert geometry(256, 16, 256, 1, 0) == (1, 256, 1, 0)
    assert geometry(256, 16, 256, 2, 1) == (2, 128, 2, 1)
    assert geometry(256, 16, 256, 4, 0) == (4, 64, 4, 0)
    assert geometry(256, 16, 8, 4, 0) == (1, 256, 1, 0)  # a small part: one block holds all 16 layers, no room for a second tile
    assert geometry(250, 5, 256, 4, 0) == (2, 125, 2, 0) and geometry(255, 5, 256, 4, 0) == (1, 255, 1, 0)


def test_bad_arguments():
    lib = _hip.load()
    out = (C.c_int32 * 4)()
    for bad in ((0, 4, 256, 1, 0), (64, 0, 256, 1, 0), (64, 17, 256, 1, 0), (64, 4, 0, 1, 0), (64, 4, 256, 3, 0), (64, 4, 256, 5, 0), (64, 4, 256, -1, 0)):
        assert lib.gemlite_hip_capture_group_geometry(*bad, C.byref(out)) == -1, bad
    assert lib.gemlite_hip_capture_group_geometry(64, 4, 256, 1, 0, None) == -1


def busiest_cu(tiles, members, resident, tb):
    """(layer, tile) slots on the busiest CU: rounds of blocks over the CUs x layers of the fullest block x TB; None: TB not admitted."""
    t, gx, gy, _ = geometry_py(tiles, members, resident, tb, 0)
    return None if t != tb else -(-(gx * gy) // resident) * -(-members // gy) * tb


def default_py(tiles, members, resident):
    """The default rule: interleaved, the largest TB whose busiest CU has at most 5/4 of the work of the busiest CU under TB = 1."""
    for tb in (4, 2):
        c = busiest_cu(tiles, members, resident, tb)
        if c is not None and c * 4 <= busiest_cu(tiles, members, resident, 1) * 5:
            return geometry_py(tiles, members, resident, tb, 0)
    return geometry_py(tiles, members, resident, 1, 0)


def test_what_a_capture_picks():
    """tb_want = 0: the default rule, or what GEMLITE_HIP_CAPTURE_GROUP_TILES forces (read once per process)."""
    for tiles in TILES:
        for members in range(1, 17):
            for resident in RESIDENT:
                tb, gx, gy, span = geometry(tiles, members, resident, 0, 0)
                assert (tb, gx, gy, span) == geometry_py(tiles, members, resident, tb, span)
                if FORCED:
                    want_tb = 4 if int(FORCED.rstrip("si")) >= 4 else (2 if int(FORCED.rstrip("si")) >= 2 else 1)
                    assert (tb, gx, gy, span) == geometry_py(tiles, members, resident, want_tb, int("s" in FORCED))
                else:
                    assert (tb, gx, gy, span) == default_py(tiles, members, resident), (tiles, members, resident)


def test_the_default_rule_at_the_measured_shapes():
    """256 tiles on 256 CUs (profiles/r16/decode_group_tiles.log): every measured member count gets the TB that was fastest for it — 1 for 3;
    2 for 2, 5 and 6; 4 for 4, 7, 8, 10, 12, 15 and 16 — and never the span placement."""
    assert [default_py(256, m, 256)[0] for m in range(1, 17)] == [1, 2, 1, 4, 2, 2, 4, 4, 2, 4, 4, 4, 4, 4, 4, 4]
    assert default_py(256, 16, 256) == (4, 64, 4, 0) and default_py(256, 12, 256) == (4, 64, 4, 0) and default_py(256, 2, 256) == (2, 128, 2, 0)
    assert default_py(688, 12, 256) == (1, 688, 1, 0)  # 24 slots per block do not fit: one tile per block
    assert all(default_py(t, m, r)[3] == 0 for t in TILES for m in range(1, 17) for r in RESIDENT)
