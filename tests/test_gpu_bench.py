"""bench.py end to end on a small workload: a plain run prints the headline line and measures nothing
else; --full adds the figures measured after the timed region."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "sustained", "step_incl_launch_ms", "strong_scaling_shard_ms", "end_to_end", "cpu_baseline")


def _bench(*extra, timeout):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--workload", "c1", "--steps", "3",
                        "--warmup", "1"] + list(extra), cwd=REPO, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only():
    out = _bench(timeout=300)
    for k in HEADLINE:
        assert k in out, k
    assert out["metric"] == "resolved propagation paths/sec" and out["unit"] == "paths/s"
    assert out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["steps"] == 3
    for k in FULL_ONLY:
        assert k not in out, k


@pytest.mark.gpu
def test_full_run_adds_the_other_figures():
    out = _bench("--full", "--sustain-s", "0.2", "--cpu-budget-s", "1", timeout=600)
    for k in HEADLINE + FULL_ONLY:
        assert k in out, k
    assert "end_to_end_error" not in out, out.get("end_to_end_error")
    assert out["roofline"]["steps_with_kernel_events"] == 10
