"""grid.y of a grouped M = 1 decode launch (gemlite_hip_capture_group_grid_y, host only): clamp(resident blocks / tiles, 1, members),
answered for a full part of 256 CUs (a launch puts its own device's CU count in place of 256)."""
from gemlite_amd import _hip


def _y(tiles, members):
    return _hip.load().gemlite_hip_capture_group_grid_y(tiles, members)


def test_wide_layers_get_one_block_per_tile():
    assert _y(256, 16) == 1 and _y(688, 16) == 1 and _y(257, 2) == 1


def test_narrow_layers_spread_their_members_over_idle_cus():
    assert _y(64, 7) == 4 and _y(128, 16) == 2 and _y(136, 16) == 1 and _y(16, 16) == 16


def test_never_more_blocks_in_y_than_members():
    assert _y(64, 3) == 3 and _y(16, 2) == 2 and _y(64, 1) == 1


def test_non_positive_arguments_answer_zero():
    assert _y(0, 4) == 0 and _y(64, 0) == 0 and _y(-1, -1) == 0
