"""How the 16 waves of a grouped M = 1 decode block share its layers (gemlite_hip_capture_group_wave_split, host only: the rule the
kernel itself compiles, decode3_wave_split of gl_common.h): 16 / LB waves per layer, each in place of a contiguous run of the
single-layer kernel's 16 waves ("virtual waves")."""
import ctypes as C

import pytest

from gemlite_amd import _hip

NW = 16


def _split(lb, wave):
    out = (C.c_int32 * 3)(7, 7, 7)
    _hip.load().gemlite_hip_capture_group_wave_split(lb, wave, C.byref(out))
    return tuple(out)


@pytest.mark.parametrize("lb", range(1, 17))
def test_every_layer_and_virtual_wave_has_exactly_one_owner(lb):
    owners = {}
    for wave in range(NW):
        layer, v0, v1 = _split(lb, wave)
        if layer < 0:
            continue
        assert 0 <= layer < lb and 0 <= v0 < v1 <= NW, (wave, layer, v0, v1)
        for v in range(v0, v1):
            assert (layer, v) not in owners, f"({layer}, {v}) owned by waves {owners[(layer, v)]} and {wave}"
            owners[(layer, v)] = wave
    assert set(owners) == {(layer, v) for layer in range(lb) for v in range(NW)}


@pytest.mark.parametrize("lb", range(1, 17))
def test_waves_past_the_last_layer_own_nothing(lb):
    p = NW // lb
    for wave in range(NW):
        layer, v0, v1 = _split(lb, wave)
        if wave >= lb * p:
            assert (layer, v0, v1) == (-1, 0, 0), (wave, layer, v0, v1)
        else:
            assert layer == wave // p


@pytest.mark.parametrize("lb", range(1, 17))
def test_ranges_are_contiguous_and_ascending(lb):
    p = NW // lb
    for layer in range(lb):
        end = 0
        for wave in range(layer * p, (layer + 1) * p):  # a layer's waves are neighbours
            got, v0, v1 = _split(lb, wave)
            assert got == layer and v0 == end and v1 > v0, (wave, got, v0, v1)
            end = v1
        assert end == NW


def test_the_benchmark_group_and_a_pair():
    """16 members at 4096 columns: one wave per layer walks all 16 virtual waves.  Two members: eight waves per layer, two each."""
    assert [_split(16, w) for w in range(NW)] == [(w, 0, NW) for w in range(NW)]
    assert [_split(2, w) for w in range(NW)] == [(w // 8, 2 * (w % 8), 2 * (w % 8) + 2) for w in range(NW)]
    assert [_split(5, w)[1:] for w in range(3)] == [(0, 5), (5, 10), (10, 16)] and _split(5, 15) == (-1, 0, 0)


def test_arguments_out_of_range():
    for lb, wave in [(0, 0), (17, 0), (-1, 3), (4, -1), (4, 16)]:
        assert _split(lb, wave) == (-1, 0, 0), (lb, wave)
