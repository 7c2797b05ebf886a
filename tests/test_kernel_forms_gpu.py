"""Every kernel form the forward planner answers, launched once against the float64 oracle (`pytest -m gpu`).

One case per row of tests/golden/kernel_forms.json (tests/kernel_forms.py): (form, fp16 | bf16) at the smallest shape the planner's
sweep reaches it, a ragged row count, and K slices where the form has them.  A case
  1. builds the layer through the public path (GemLiteLinear.pack or the helper processor) with metadata that differs per group and column and activation
     rows that differ pairwise and have a mean that is not zero;
  2. asks the planner on the real tensors and FAILS unless the answer is the frozen form and workspace size — it never tests another kernel instead;
  3. launches through core._hip_matmul with the row's matmul_type and tuning (raw_x for the forms that quantise the activations themselves);
  4. compares with the oracle on the tensors the layer holds and the activations the project's quantiser produced — the family's own gates, unchanged
     (`_compare` of test_gpu_parity, `_check` of test_mx_gpu, bit for bit for int8 x int8: KF.check); a fused-quantiser form is also bit-identical to
     quantiser + matmul under the same tuning;
  5. checks shape, finiteness, and that a launch with K slices leaves the arrival counters of the workspace at zero.
tests/test_kernel_forms_cpu.py checks on the CPU that this comparison rejects wrong results at these shapes with this data."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemlite_amd import _hip  # noqa: E402
from gemlite_amd.core import _hip_matmul  # noqa: E402
from tests import kernel_forms as KF  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (rows of one layer next to each other: the layer is packed once)
ROWS = sorted(KF.load_rows(), key=lambda r: (r["family"], r["tdt"], r["N"], r["K"], r["M"]))


@pytest.mark.parametrize("row", ROWS, ids=[KF.row_id(r) for r in ROWS])
def test_form_against_the_oracle(row):
    lib = KF.load_lib()
    case = KF.build_case(row, DEV)
    fam, tdt, lin = case["fam"], case["tdt"], case["lin"]
    M, N = row["M"], row["N"]
    got = KF.plan(lib, KF.call_args(row, case))
    assert got == (row["name"], row["workspace_bytes"]), (got, "the planner answers another form for this row on the real tensors")
    tuning, meta = tuple(row["tuning"]), lin.get_meta_args()
    y = _hip_matmul(case["x_in"], lin.W_q, lin.scales, lin.zeros, case["sx_in"], meta, row["matmul_type"], tuning, raw_x=case["fused"])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device error: the context is gone, every later case would only launch onto a faulted GPU
        pytest.exit(f"{KF.row_id(row)}: {e!r} — nothing more is launched after a device error", returncode=3)
    assert tuple(y.shape) == (M, N) and y.dtype == KF.torch_dtype(tdt)
    if row["workspace_bytes"] > 0:
        dev = torch.device(DEV)
        ws = _hip.workspace(dev, _hip.current_stream_handle(dev), 0)
        assert ws.numel() >= row["workspace_bytes"]
        assert bool((ws[:KF.COUNTER_BYTES] == 0).all()), "arrival counters not left at zero"
    parts = KF.oracle_parts(fam, lin, case["xq"], case["sx"], row["name"])
    KF.check(fam, tdt, KF.row_id(row), y, KF.oracle_out(parts), parts)
    if case["fused"]:
        y_two = _hip_matmul(case["xq"], lin.W_q, lin.scales, lin.zeros, case["sx"], meta, row["matmul_type"], tuning)
        torch.cuda.synchronize()
        assert torch.equal(y, y_two), ("not bit-identical to quantiser + matmul", float((y.float() - y_two.float()).abs().max()))
