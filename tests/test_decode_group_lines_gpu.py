"""Lines of the grouped M = 1 decode kernel (gemv_decode.hip; gl_common.h: decode3_group_lines): a wave works on H in {1, 2, 4} adjacent
tiles of its block's tile group in H passes over each virtual wave, so that one request instruction asks for whole 128- or 256-byte runs
of a weight row.  What a lane computes for its (layer, tile, virtual wave, row pair) and the order in which partial sums are added do
not change, so every output is BIT-EXACT (torch.equal) against the eager layer on the same inputs under every (TB, H).  The two overrides
are read once per process: every case forces its pair in a fresh child (tests/decode_group_lines_child.py, which describes the groups),
where every group is captured through the C ABI with its outputs between guard bytes and replayed twice.  A child that dies on a signal
ends the file: the cases behind it fail without starting anything on the GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.decode_group_lines_child import GROUPS, KERNEL
from tests.test_capture_groups_gpu import ROOT
from tests.test_decode_group_lines_cpu import default_lines_py, lines_py
from tests.test_decode_group_tiles_cpu import default_py, geometry_py

pytestmark = pytest.mark.gpu
PER_WAVE_X, SHARED_X = 1, 2
FORCED = [(2, 2), (4, 2), (4, 4), None]  # (TB, H) asked for; None: the default rule
CASES = [(s, f) for s in ("n1024", "widths", "ks", "forms", "lines") for f in FORCED] + [("n4096", (4, 4)), ("n4096", None)]
_signalled = []


def _child(scenario, forced):
    if _signalled:
        pytest.fail(f"not started: an earlier child died on a signal ({_signalled[0]})")
    env = dict(os.environ)
    env.pop("GEMLITE_HIP_CAPTURE_GROUP_TILES", None)
    env.pop("GEMLITE_HIP_CAPTURE_GROUP_LINES", None)
    if forced:
        env["GEMLITE_HIP_CAPTURE_GROUP_TILES"] = f"{forced[0]}i"
        env["GEMLITE_HIP_CAPTURE_GROUP_LINES"] = str(forced[1])
    out = subprocess.run([sys.executable, "-m", "tests.decode_group_lines_child", scenario], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=180)
    if out.returncode < 0:
        _signalled.append(f"{scenario} {forced}: signal {-out.returncode}")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(l[len("RESULT "):]) for l in out.stdout.splitlines() if l.startswith("RESULT ")]


@pytest.mark.parametrize("scenario,forced", CASES, ids=[f"{s}-{'tb%dh%d' % f if f else 'default'}" for s, f in CASES])
def test_every_layer_is_bit_exact_under_the_forced_lines(scenario, forced):
    results = _child(scenario, forced)
    specs = GROUPS[scenario]
    assert len(results) == len(specs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for r, spec in zip(results, specs):
        N, K, members, dt, gs, zeros_kind, biased, own = spec
        what = f"{spec} forced {forced!r}: {r}"
        # (a group the planner routes elsewhere is a mistake in the child's list, not a reason to skip)
        assert all(k.startswith(KERNEL) for k in r["kernels"]) and len(r["kernels"]) == 1, what
        assert r["seen"] == members and r["joined"] == members - 1, what
        assert r["form"] == (SHARED_X if members >= 3 and own is None else PER_WAVE_X), what
        tb, gx, gy, span = r["geometry"]
        if forced:
            assert (tb, gx, gy, span) == geometry_py(N // 16, members, cus, forced[0], 0), what
            assert r["lines"] == r["last_lines"] == lines_py(tb, forced[1]), what
        else:
            assert (tb, gx, gy, span) == default_py(N // 16, members, cus), what
            assert r["lines"] == r["last_lines"] == default_lines_py(N // 16, members, cus, tb), what
        assert r["guards"], "a store outside every member's out: " + what
        assert all(r["equal"]) and len(r["equal"]) == members, what


def test_the_cases_reach_the_lines_they_are_meant_for():
    """On a 256-CU part (host-only arithmetic): what each scenario exercises."""
    assert geometry_py(70, 3, 256, 4, 0)[0] == 2 and lines_py(2, 4) == 2  # 70 tiles: H = 4 arrives as H = 2
    assert geometry_py(67, 5, 256, 4, 0)[0] == 1 and lines_py(1, 4) == 1  # 67 tiles: H = 1
    assert geometry_py(4, 4, 256, 4, 0)[:3] == (4, 1, 4)                  # N = 64: one run of four tiles, one block per member
    assert geometry_py(64, 7, 256, 4, 0)[:3] == (4, 16, 7) and geometry_py(64, 16, 256, 4, 0)[:3] == (4, 16, 16)  # grid.y > 1
    assert geometry_py(256, 16, 256, 4, 0)[:3] == (4, 64, 4)              # the benchmark's launch: four wave-slots of four waves under H = 4
