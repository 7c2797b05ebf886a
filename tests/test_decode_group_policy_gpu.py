"""Weight-load policy of the grouped M = 1 decode kernel (gemv_decode.hip; gl_common.h: decode3_group_nt): a grouped node asks for its weights
non-temporally when its waves ask for whole lines (H >= 2), its members' own launches are non-temporal and every member's weight base and
the row pitch are multiples of 128 bytes.  The policy changes how a line is asked for, never which bytes arrive, so every output is
BIT-EXACT (torch.equal) against the eager layer on the same inputs under every (TB, H, policy).  The overrides are read once per process:
every case forces its set in a fresh child (tests/decode_group_policy_child.py, which describes the groups), where every group is captured
through the C ABI with its outputs between guard bytes and replayed twice.  A child that dies on a signal ends the file: the cases behind
it fail without starting anything on the GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.decode_group_policy_child import GROUPS, KERNEL
from tests.test_capture_groups_gpu import ROOT
from tests.test_decode_group_lines_cpu import default_lines_py, lines_py
from tests.test_decode_group_policy_cpu import RULE, policy_py
from tests.test_decode_group_tiles_cpu import default_py, geometry_py

pytestmark = pytest.mark.gpu
PER_WAVE_X, SHARED_X = 1, 2
# (TB, H, policy) asked for; None: the default rules.  (4, 4) and (4, 2) on 4 and 32 tiles need the force: the default rule takes TB = 4 only
# where the layers fill the part
FORCED = [(2, 2, None), (4, 2, None), (4, 4, None), (4, 4, 0), (1, 1, 1), None]
CASES = [("shapes", f) for f in FORCED] + [("policy", None), ("policy", (4, 4, None)), ("policy", (4, 2, 1))]
_signalled = []


def _child(scenario, forced):
    if _signalled:
        pytest.fail(f"not started: an earlier child died on a signal ({_signalled[0]})")
    env = dict(os.environ)
    for k in ("GEMLITE_HIP_CAPTURE_GROUP_TILES", "GEMLITE_HIP_CAPTURE_GROUP_LINES", "GEMLITE_HIP_CAPTURE_GROUP_NT"):
        env.pop(k, None)
    if forced:
        env["GEMLITE_HIP_CAPTURE_GROUP_TILES"] = f"{forced[0]}i"
        env["GEMLITE_HIP_CAPTURE_GROUP_LINES"] = str(forced[1])
        if forced[2] is not None:
            env["GEMLITE_HIP_CAPTURE_GROUP_NT"] = str(forced[2])
    out = subprocess.run([sys.executable, "-m", "tests.decode_group_policy_child", scenario], env=env, cwd=ROOT, capture_output=True, text=True,
                         timeout=180)
    if out.returncode < 0:
        _signalled.append(f"{scenario} {forced}: signal {-out.returncode}")
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    return [json.loads(l[len("RESULT "):]) for l in out.stdout.splitlines() if l.startswith("RESULT ")]


def _nodes(flags, members):
    """Runs of members whose launches share a kernel function: [(first member, count, flagged)]"""
    flags = flags or [0] * members
    runs = []
    for i, f in enumerate(flags):
        if runs and runs[-1][2] == f:
            runs[-1][1] += 1
        else:
            runs.append([i, 1, f])
    return runs


def _id(case):
    s, f = case
    return f"{s}-" + ("default" if f is None else "tb%dh%d%s" % (f[0], f[1], "" if f[2] is None else "nt%d" % f[2]))


@pytest.mark.parametrize("scenario,forced", CASES, ids=[_id(c) for c in CASES])
def test_every_layer_is_bit_exact_and_the_node_carries_the_policy_of_the_rule(scenario, forced):
    results = _child(scenario, forced)
    specs = GROUPS[scenario]
    assert len(results) == len(specs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for r, spec in zip(results, specs):
        N, K, members, dt, gs, zeros_kind, biased, own, w_off, flags = spec
        what = f"{spec} forced {forced!r}: {r}"
        assert all(k.startswith(KERNEL) for k in r["kernels"]) and len(r["kernels"]) == 1, what
        assert r["w_mod_128"] == [w_off % 128], what
        runs = _nodes(flags, members)
        assert r["seen"] == members and r["joined"] == members - len(runs), what
        assert len(r["trail"]) == members, what
        for first, count, flagged in runs:
            # the call that opens a node: no grouped node yet; every later member: the node as it is after that join
            assert r["trail"][first] == [0, 0, -1], what
            for j in range(1, count):
                n = j + 1  # members of the node after this join
                form, lines, policy = r["trail"][first + j]
                same_x = own is None or not (first <= own <= first + j)
                assert form == (SHARED_X if n >= 3 and same_x else PER_WAVE_X), what
                if forced:
                    tb = geometry_py(N // 16, n, cus, forced[0], 0)[0]
                    h = lines_py(tb, forced[1])
                else:
                    tb = default_py(N // 16, n, cus)[0]
                    h = lines_py(tb, default_lines_py(N // 16, n, cus, tb))
                assert lines == h, what
                pitch = N * 4  # bytes of a packed weight row
                f = RULE if not forced or forced[2] is None else forced[2]
                assert policy == policy_py(h, flagged, w_off, pitch, f), what
        assert r["guards"], "a store outside every member's out: " + what
        assert all(r["equal"]) and len(r["equal"]) == members, what


def test_the_cases_reach_the_forms_they_are_meant_for():
    """On a 256-CU part (host-only arithmetic): what the scenarios exercise."""
    # forced TB = 4: N = 64 is ONE tile group, every member a block of its own; N = 512: eight groups
    assert geometry_py(4, 16, 256, 4, 0)[:3] == (4, 1, 16) and geometry_py(32, 5, 256, 4, 0)[:3] == (4, 8, 5)
    assert geometry_py(4, 2, 256, 2, 0)[:3] == (2, 2, 2) and geometry_py(32, 16, 256, 2, 0)[:3] == (2, 16, 16)
    assert [lines_py(tb, h) for tb, h in ((2, 2), (4, 2), (4, 4), (1, 1))] == [2, 2, 4, 1]
    # the rule at the forms the cases reach: non-temporal for aligned members without the flag under H = 2 and 4, never under H = 1
    assert [policy_py(h, 0, 0, 2048) for h in (1, 2, 4)] == [0, 1, 1]
    assert [policy_py(h, 0, 64, 2048) for h in (2, 4)] == [0, 0] and [policy_py(h, 1, 0, 2048) for h in (2, 4)] == [0, 0]
    assert policy_py(4, 0, 128, 2048) == 1 and policy_py(1, 0, 0, 2048, 1) == 0 and policy_py(2, 1, 64, 2048, 1) == 1
    assert _nodes([1, 1, 1, 0, 0, 0, 1, 1, 1], 9) == [[0, 3, 1], [3, 3, 0], [6, 3, 1]]
