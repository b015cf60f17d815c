"""The host acts on the launch plan (csrc/hrt_launch_plan.h) before it launches: the LoS pass rides in launch 0's fused
kernel only where the plan says that launch 0 fuses.  Two tunes on the street canyon (234 triangles, 20 000 rays per
TX, 4 bounces), each a process of its own (tests/launch_plan_child.py):

  fine_off_lds   accel_fine_min=0,lds_tri_bytes=0: the fine walk, launch 0 cannot fuse, the LoS pass is its own kernel
                 and has a time of its own; no records kernel
  default        launch 0 fused with the LoS pass in its tail; patch tables, the records kernel

In both the dense result equals the oracle's bit for bit, and with the timer every phase is finite and not negative."""
import json
import math
import os
import subprocess
import sys

import pytest

from tests.tune import tuned

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120

TUNES = {"fine_off_lds": dict(accel_fine_min="0", lds_tri_bytes="0"), "default": {}}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(TUNES))
def test_dense_is_bit_identical_and_the_timer_phases_are_sound(name):
    records_kernel = name == "default"
    p = subprocess.run([sys.executable, "-m", "tests.launch_plan_child", "1" if records_kernel else "0"], cwd=REPO,
                       env=tuned(**TUNES[name]), capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    assert p.returncode == 0 and "PLAN_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    times = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("PLAN_TIMES ")][0][len("PLAN_TIMES "):])
    print(name, times)
    phases = [times["los_ms"]] + [t for k in ("trace_ms", "shade_ms", "records_ms") for t in times[k]]
    assert len(phases) == 1 + 3 * 5
    assert all(math.isfinite(t) and t >= 0.0 for t in phases), times
    if name == "fine_off_lds":
        assert times["los_ms"] > 0.0, times   # its own kernel between the timer's first two events
