"""ROUNDS on the GPU (capture_group.hip: a full grouped decode node directly behind another full one of the same capture is merged into it;
gemv_decode.hip: block row yy of a node is row yy % Y of round yy / Y).  The member limit and the round limit are read once per process,
so every case runs in a fresh child (tests/decode_group_rounds_child.py, which describes the cases): the layers are captured through the
C ABI with their outputs between guard elements, replayed three times, and every output must be torch.equal to the eager layer's.  The
counters must show the merges the case is about.  A child that dies on a signal ends the file: the cases behind it fail without starting
anything on the GPU."""
import json
import os
import subprocess
import sys

import pytest

from tests.decode_group_rounds_child import CASES, KERNEL, SWITCH
from tests.test_capture_groups_gpu import ROOT

pytestmark = pytest.mark.gpu
PER_WAVE_X, SHARED_X = 1, 2
_signalled = []
_results = {}


def _child(name):
    if name in _results:
        return _results[name]
    if _signalled:
        pytest.fail(f"not started: an earlier child died on a signal ({_signalled[0]})")
    env = dict(os.environ)
    for k in ("GEMLITE_HIP_CAPTURE_GROUP_MAX", SWITCH, "GEMLITE_HIP_NO_CAPTURE_GROUPS", "GEMLITE_HIP_CAPTURE_GROUP_TILES",
              "GEMLITE_HIP_CAPTURE_GROUP_LINES", "GEMLITE_HIP_CAPTURE_GROUP_NT", "GEMLITE_HIP_CAPTURE_GROUP_SHARED_X"):
        env.pop(k, None)
    env.update(CASES[name]["env"])
    out = subprocess.run([sys.executable, "-m", "tests.decode_group_rounds_child", name], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=180)
    if out.returncode < 0:
        _signalled.append(f"{name}: signal {-out.returncode}")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    res = [json.loads(l[len("RESULT "):]) for l in out.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(res) == 1
    _results[name] = res[0]
    return res[0]


def rounds_trail_py(L, n, rounds_max):
    """What gemlite_hip_capture_group_last_rounds() says after each of n independent launches on one x, and the merges: a launch that
    opens a group 0, one that joins 1, one that fills a group behind a full predecessor with room for a round: the predecessor's new count."""
    trail, merges, g, prev = [], 0, None, None
    for _ in range(n):
        if g and g[0] < L:
            g[0] += 1
            last = 1
            if g[0] == L and prev:
                prev[0] += L
                prev[1] += 1
                g, prev, merges = prev, None, merges + 1
                last = g[1]
        else:
            prev = g if g and g[1] < rounds_max else None
            g, last = [1, 1], 0
        trail.append(last)
    return trail, merges


def test_the_restatement_of_the_rule():
    assert rounds_trail_py(2, 9, 4) == ([0, 1, 0, 2, 0, 3, 0, 4, 0], 3)
    assert rounds_trail_py(3, 8, 4) == ([0, 1, 1, 0, 1, 2, 0, 1], 1)
    assert rounds_trail_py(2, 10, 4) == ([0, 1, 0, 2, 0, 3, 0, 4, 0, 1], 3)
    assert rounds_trail_py(2, 9, 2) == ([0, 1, 0, 2, 0, 1, 0, 2, 0], 2)
    assert rounds_trail_py(2, 9, 1) == ([0, 1] * 4 + [0], 0)
    assert rounds_trail_py(16, 33, 4)[1] == 1 and rounds_trail_py(16, 64, 4)[1] == 3


def _common(name):
    c, r = CASES[name], _child(name)
    assert all(k.startswith(KERNEL) for k in r["kernels"]), r["kernels"]
    assert r["guards"], name
    assert all(r["equal"]) and len(r["equal"]) == c["n"], (name, r["equal"])
    groups = (c["n"] + c["L"] - 1) // c["L"]
    assert r["seen"] == c["n"] and r["joined"] == c["n"] - groups, (name, r["seen"], r["joined"])  # joins: what they were without merging
    return c, r


PLAIN = ["basic-fp16", "basic-fp16-bias", "basic-bf16", "basic-bf16-bias", "partial-1", "partial-2", "limit", "new-x", "off", "two-rounds",
         "headline"]
MERGES = {"basic-fp16": 3, "basic-fp16-bias": 3, "basic-bf16": 3, "basic-bf16-bias": 3, "partial-1": 1, "partial-2": 1, "limit": 3, "new-x": 1,
          "off": 0, "two-rounds": 2, "headline": 1}


@pytest.mark.parametrize("name", PLAIN)
def test_full_groups_of_independent_layers_become_one_node_of_rounds(name):
    c, r = _common(name)
    want_max = int(c["env"].get(SWITCH, min(4, 64 // c["L"])))
    assert r["rounds_max"] == want_max
    trail, merges = rounds_trail_py(c["L"], c["n"], want_max)
    assert merges == MERGES[name]  # (the issue's figure for the case)
    assert r["merged"] == merges, (name, r["merged"], r["trail"])
    assert [t[3] for t in r["trail"]] == trail, (name, r["trail"])


def test_a_second_group_on_another_x_puts_the_merged_node_on_the_per_wave_x_form():
    c, r = _common("different-x")
    L = c["L"]
    assert r["merged"] == 1
    assert r["trail"][L - 1][0] == SHARED_X and r["trail"][L - 1][3] == 1  # the first group alone: one x
    assert r["trail"][2 * L - 1][0] == PER_WAVE_X and r["trail"][2 * L - 1][3] == 2


def test_one_member_off_the_line_puts_the_merged_node_on_the_default_policy():
    c, r = _common("unaligned")
    L = c["L"]
    assert r["w_mod_128"] == [0, 64]
    assert r["trail"][L - 1][1:] == [2, 1, 1]  # the first group: H = 2, non-temporal, one round
    assert r["merged"] == 1 and r["trail"][2 * L - 1][1:] == [2, 0, 2]


@pytest.mark.parametrize("name", ["dependent", "foreign", "fork"])
def test_what_rules_a_merge_out(name):
    c, r = _common(name)
    assert r["merged"] == 0 and max(t[3] for t in r["trail"]) == 1, r["trail"]
    if name != "dependent":
        assert r["scratch"] == 3.0  # the foreign kernel ran once per replay
