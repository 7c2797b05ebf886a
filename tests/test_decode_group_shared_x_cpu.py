"""Host-only side of the shared-x grouped decode form (capture_group.hip, gl_common.h): which form a grouped node takes and how much
dynamic LDS a shared-x block asks for, against a restatement in Python.  No GPU."""
import os

import pytest

from gemlite_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gemlite_hip_capture_group_last_form", "gemlite_hip_capture_group_form", "gemlite_hip_capture_group_shared_x_lds_bytes")
RED_BYTES = 16 * 4096      # 16 layers x (16 waves x 4 DPP rows x 16 columns) floats of partial rows
MIN_MEMBERS = 3            # two members: staging costs more than it saves (profiles/r15/decode_group_shared_x.log)
LDS_LIMIT = 160 * 1024     # LDS of one CU of gfx950
SWITCH_ON = os.environ.get("GEMLITE_HIP_CAPTURE_GROUP_SHARED_X", "1") not in ("0",)


def lds_bytes(K):
    """64 KiB of partial rows, then per 16 elements of x eight pair dwords and one fp32 sum: 36 bytes per unit = 2.25 K bytes."""
    if K <= 0 or K % 256:
        return 0
    b = RED_BYTES + (K // 16) * 36
    return b if b <= LDS_LIMIT else 0


def form(members, same_x, K):
    if members < 2:
        return 0
    return 2 if (SWITCH_ON and same_x and members >= MIN_MEMBERS and lds_bytes(K) > 0) else 1


def test_the_new_symbols_are_exported_and_declared():
    lib = _hip.load()
    header = open(os.path.join(ROOT, "include", "gemlite_hip.h")).read()
    for sym in NEW:
        assert sym in _hip.EXPORTED_SYMBOLS and hasattr(lib, sym) and sym + "(" in header, sym
    assert "GEMLITE_HIP_CAPTURE_GROUP_SHARED_X" in header


KS = [256, 512, 768, 4096, 4352, 11008, 16384, 16640, 32768, 43520, 43776, 65536]


@pytest.mark.parametrize("K", KS, ids=lambda k: f"K{k}")
def test_lds_size(K):
    lib = _hip.load()
    assert lib.gemlite_hip_capture_group_shared_x_lds_bytes(K) == lds_bytes(K)


def test_lds_size_at_the_benchmark_shape_and_at_the_budget_edge():
    assert lds_bytes(4096) == 65536 + 9216
    assert lds_bytes(16384) == 65536 + 36864 and lds_bytes(16640) == 65536 + 37440
    assert lds_bytes(43520) == 65536 + 97920 and lds_bytes(43776) == 0  # 2.25 K <= 96 KiB: K <= 43690
    lib = _hip.load()
    for K in (0, -256, 100, 4095):
        assert lib.gemlite_hip_capture_group_shared_x_lds_bytes(K) == 0


def test_form_decision():
    lib = _hip.load()
    for K in KS:
        for members in range(1, 17):
            for same_x in (0, 1):
                assert lib.gemlite_hip_capture_group_form(members, same_x, K) == form(members, same_x, K), (members, same_x, K)
    if SWITCH_ON:
        assert form(2, 1, 4096) == 1 and form(3, 1, 4096) == 2 and form(16, 1, 4096) == 2 and form(16, 0, 4096) == 1 and form(5, 1, 16640) == 2 and form(5, 1, 43520) == 2 and form(5, 1, 43776) == 1
    for bad in ((0, 1, 4096), (17, 1, 4096), (4, 1, 0), (4, 1, 1000)):
        assert lib.gemlite_hip_capture_group_form(*bad) == -1


def test_last_form_answers_without_a_device():
    assert _hip.load().gemlite_hip_capture_group_last_form() in (0, 1, 2)
