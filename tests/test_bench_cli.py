"""bench.py's two kinds of run: a plain run builds, settles, warms up, times --steps steps, writes --dump-outputs and prints its
line; whatever takes runs of its own (the 300-step distribution, the lazy read-back, the small-island sample, the other
configurations, the CPU baselines) is behind --full. Both time the same steps from the same state."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
CONTRACT_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY_KEYS = ("per_step_distribution_300", "ms_per_step_lazy_readback", "roofline_small_islands", "extra_configs", "cpu_baseline")


def _bench(*args):
    """One bench.py run in a process of its own: its parsed JSON line"""
    res = subprocess.run([sys.executable, BENCH] + [str(a) for a in args], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, "one JSON line expected, got %d" % len(lines)
    return json.loads(lines[0])


def test_full_is_an_option_and_off_by_default():
    res = subprocess.run([sys.executable, BENCH, "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "--full" in res.stdout
    for opt in ("--gpus", "--steps", "--warmup", "--dump-outputs"):
        assert opt in res.stdout


@pytest.mark.gpu
def test_plain_run_is_lean_and_full_run_times_the_same_steps(tmp_path):
    """A small Tumbler (40 x 40 boxes) through both kinds of run: the plain line carries the contract's keys and none of the
    figures that take runs of their own, the --full line carries them, and what the last timed step handed its caller is the
    same array for array - the extra measurements come behind the timed steps and the dump."""
    common = ["--gpus", 1, "--steps", 10, "--warmup", 5, "--tumbler", 40]
    plain = _bench(*common, "--dump-outputs", tmp_path / "plain")
    full = _bench(*common, "--full", "--no-extras", "--no-secondary", "--no-cpu-baseline", "--dump-outputs", tmp_path / "full")
    for line in (plain, full):
        for key in CONTRACT_KEYS:
            assert key in line, key
        assert line["unit"] == "steps/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
        assert line["steps"] == 10 and line["warmup"] == 5
        assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1000.0) < 1e-6 * 1000.0
    assert plain["full"] is False and full["full"] is True
    for key in FULL_ONLY_KEYS:
        assert key not in plain, key
    assert "per_step_distribution_300" in full and "error" not in full["per_step_distribution_300"]
    assert "ms_per_step_lazy_readback" in full
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "bodies.npy" in names
    for name in names:
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.shape == b.shape and np.array_equal(a, b), name
