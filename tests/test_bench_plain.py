"""bench.py: a plain run measures the headline only; everything that takes runs of its own is behind --full."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")

# keys of the line / of `roofline` that only --full measures
FULL_ONLY_LINE = ("cpu_baseline",)
FULL_ONLY_ROOFLINE = ("event_us", "event_clock_floor_us", "empty_launch_us", "kernel_us_minus_empty_launch", "schema", "m256", "fewrows",
                      "m1_bf16", "cfg4", "cfg5", "mx_fewrows", "mx_m256", "prefill_m2048", "trend_m1", "rotation_ab", "eager", "sustained")


def test_full_is_an_option_and_off_by_default():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full " in out.stdout


def test_full_out_needs_full(tmp_path):
    out = subprocess.run([sys.executable, BENCH, "--full-out", str(tmp_path / "full.json")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--full" in out.stderr
    assert not (tmp_path / "full.json").exists()


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_nothing_that_takes_runs_of_its_own(tmp_path):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "fp16"
    assert line["steps"] == 5 and line["warmup"] == 2 and line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step are two views of the same timed region: 64 layers x 8 929 280 algorithmic bytes per step
    assert line["value"] == pytest.approx(64 * 8929280 / 1e9 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    roof = line["roofline"]
    assert roof["kernel"] and roof["kernel_us"] == pytest.approx(line["ms_per_step"] * 1e3 / 64, rel=1e-3)
    assert not [k for k in FULL_ONLY_LINE if k in line]
    assert not [k for k in FULL_ONLY_ROOFLINE if k in roof]
    assert sorted(os.listdir(tmp_path)) == ["out.npy"]
