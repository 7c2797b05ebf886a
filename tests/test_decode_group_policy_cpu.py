"""Host-only side of the weight-load policy of the grouped decode kernel (gl_common.h: decode3_group_nt): a grouped launch asks for its
weights non-temporally only when its waves ask for whole 128-byte lines (H >= 2), its members' own launches are non-temporal (their
tuning carries no GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS) and every member's weight base and the row pitch are multiples of 128 bytes.
Against a restatement in Python.  No GPU."""
import os

from gemlite_amd import _hip
from tests.test_decode_group_tiles_cpu import ROOT

NEW = ("gemlite_hip_capture_group_policy", "gemlite_hip_capture_group_last_policy")
SWITCH = "GEMLITE_HIP_CAPTURE_GROUP_NT"
FORCED = os.environ.get(SWITCH, "")
RULE, CAPTURE = -1, -2  # `forced`: the rule alone / what a capture of this process picks (the switch, read once, or the rule)
BASE = 0x7F0000000000   # an allocation's address: a multiple of 128
OFFSETS = (0, 64, 128)
PITCHES = tuple(128 * k for k in (1, 2, 3, 16, 43)) + tuple(128 * k + 64 for k in (0, 1, 2, 16, 43))


def policy_py(h, default_policy_loads, w_bases_or, pitch, forced=RULE):
    if h < 2 or forced == 0:
        return 0
    if forced == 1:
        return 1
    return int(not default_policy_loads and (w_bases_or | pitch) % 128 == 0)


def policy(h, default_policy_loads, w_bases_or, pitch, forced=RULE):
    return _hip.load().gemlite_hip_capture_group_policy(h, default_policy_loads, w_bases_or, pitch, forced)


def test_the_new_symbols_are_exported_and_declared():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in NEW:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    for doc in ("include/gemlite_hip.h", "README.md", "DESIGN.md", "INTEGRATION.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "GEMLITE_TF_GEMV_DEFAULT_POLICY_LOADS" in text, doc
    for doc in ("README.md", "DESIGN.md"):
        assert SWITCH in open(os.path.join(ROOT, doc)).read(), doc
    assert lib.gemlite_hip_capture_group_last_policy() == -1  # no grouped decode node in this process


def test_the_rule_over_h_flag_base_and_pitch():
    seen = set()
    for h in (1, 2, 4):
        for flag in (0, 1):
            for off in OFFSETS:
                for pitch in PITCHES:
                    got = policy(h, flag, BASE + off, pitch)
                    assert got == policy_py(h, flag, BASE + off, pitch), (h, flag, off, pitch)
                    assert got == int(h >= 2 and not flag and off % 128 == 0 and pitch % 128 == 0)
                    seen.add(got)
    assert seen == {0, 1}


def test_one_member_off_the_line_puts_the_group_on_the_default_policy():
    """The bases travel OR-ed together: one member 64 bytes into a line is enough, wherever it stands in the group."""
    bases = [BASE + 8192 * i for i in range(5)]
    for h in (2, 4):
        acc = 0
        for b in bases:
            acc |= b
        assert policy(h, 0, acc, 2048) == 1
        for odd in range(5):
            acc = 0
            for i, b in enumerate(bases):
                acc |= b + (64 if i == odd else 0)
            assert policy(h, 0, acc, 2048) == 0, odd


def test_a_forced_value():
    for h in (1, 2, 4):
        for flag in (0, 1):
            for off in OFFSETS:
                for pitch in PITCHES:
                    assert policy(h, flag, BASE + off, pitch, 0) == 0
                    # a forced 1 overrides the flag and the alignment (speed only), and still falls back where H = 1
                    assert policy(h, flag, BASE + off, pitch, 1) == (1 if h >= 2 else 0)
                    for forced in (0, 1):
                        assert policy(h, flag, BASE + off, pitch, forced) == policy_py(h, flag, BASE + off, pitch, forced)


def test_what_a_capture_picks():
    forced = (1 if int(FORCED) else 0) if FORCED else RULE
    for h in (1, 2, 4):
        for flag in (0, 1):
            for off in OFFSETS:
                for pitch in PITCHES:
                    assert policy(h, flag, BASE + off, pitch, CAPTURE) == policy_py(h, flag, BASE + off, pitch, forced)


def test_bad_arguments():
    for bad in ((0, 0, BASE, 2048, RULE), (3, 0, BASE, 2048, RULE), (8, 0, BASE, 2048, RULE), (2, 0, BASE, 2048, 2), (2, 0, BASE, 2048, -3)):
        assert policy(*bad) == -1, bad
