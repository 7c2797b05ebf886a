"""Tile groups of the grouped M = 1 decode kernel (gemv_decode.hip; gl_common.h: decode3_group_geometry): a block holds TB in {1, 2, 4}
adjacent 16-column tiles x its layers, and the tile groups are placed on the XCDs interleaved or in contiguous spans.  Neither changes what
a wave computes for its (layer, tile, virtual wave), so every output is BIT-EXACT (torch.equal) against the eager layer on the same
inputs under every (TB, placement).  GEMLITE_HIP_CAPTURE_GROUP_TILES is read once per process: every case forces its pair in a fresh
child (tests/decode_group_tiles_child.py, which also describes the groups of each scenario), where every group is captured through the
C ABI with its outputs between guard bytes and replayed twice."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.decode_group_tiles_child import KERNEL, SCENARIOS
from tests.test_capture_groups_gpu import ROOT
from tests.test_decode_group_tiles_cpu import geometry_py

pytestmark = pytest.mark.gpu
PER_WAVE_X, SHARED_X = 1, 2

CASES = [("n4096", f) for f in ("1i", "2i", "4i", "1s", "2s", "4s", "")] + \
        [("n1024", f) for f in ("2i", "4i", "1s", "2s", "4s")] + \
        [("widths", f) for f in ("2i", "4i", "2s", "4s")] + \
        [("ks", f) for f in ("2i", "4i", "1s", "4s")] + \
        [("forms", f) for f in ("2i", "4i", "2s", "4s")]


def _child(scenario, forced):
    env = dict(os.environ)
    env.pop("GEMLITE_HIP_CAPTURE_GROUP_TILES", None)
    if forced:
        env["GEMLITE_HIP_CAPTURE_GROUP_TILES"] = forced
    out = subprocess.run([sys.executable, "-m", "tests.decode_group_tiles_child", scenario], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(l[len("RESULT "):]) for l in out.stdout.splitlines() if l.startswith("RESULT ")]


@pytest.mark.parametrize("scenario,forced", CASES, ids=[f"{s}-{f or 'default'}" for s, f in CASES])
def test_every_layer_is_bit_exact_under_the_forced_geometry(scenario, forced):
    results = _child(scenario, forced)
    specs = SCENARIOS[scenario]
    assert len(results) == len(specs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for r, spec in zip(results, specs):
        N, K, members, dt, gs, zeros_kind, biased, own = spec
        what = f"{spec} forced {forced!r}: {r}"
        assert all(k.startswith(KERNEL) for k in r["kernels"]) and len(r["kernels"]) == 1, what
        assert r["seen"] == members and r["joined"] == members - 1, what
        assert r["form"] == (SHARED_X if members >= 3 and own is None else PER_WAVE_X), what
        tb, gx, gy, span = r["geometry"]
        if forced:
            assert (tb, gx, gy, span) == geometry_py(N // 16, members, cus, int(forced[0]), int(forced[1] == "s")), what
        else:  # the default rule: some admissible geometry
            assert (tb, gx, gy, span) == geometry_py(N // 16, members, cus, tb, span), what
        assert r["guards"], "a store outside every member's out: " + what
        assert all(r["equal"]) and len(r["equal"]) == members, what


def test_the_cases_reach_the_geometries_they_are_meant_for():
    """On a 256-CU part (the arithmetic is host-only; tests/test_decode_group_tiles_cpu.py has the rule): what each scenario exercises."""
    assert geometry_py(256, 16, 256, 2, 0)[:3] == (2, 128, 2) and geometry_py(256, 16, 256, 4, 1)[:3] == (4, 64, 4)  # 16 slots, one round
    assert geometry_py(64, 7, 256, 4, 0)[:3] == (4, 16, 7) and geometry_py(64, 16, 256, 2, 0)[:3] == (2, 32, 8)  # grid.y > 1
    assert geometry_py(70, 3, 256, 4, 0)[0] == 2 and geometry_py(67, 5, 256, 4, 0)[0] == 1  # 4 -> 2 (70 tiles), -> 1 (67 tiles)
    assert (70 // 2) % 8 != 0 and 67 % 8 != 0  # span = the identity map there
    assert geometry_py(256, 5, 256, 4, 0)[:3] == (4, 64, 4)  # blocks of 2, 1, 1, 1 layers x 4 tiles
