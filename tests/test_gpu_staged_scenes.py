"""The staged triangle test with its certain-hit shortcut (HRT_STAGED_TEST, csrc/hrt_kernels.hip: no u, v division
where the hit is certain) inside the kernels that walk with it, on whole scenes: the product against the CPU port
(oracle.compute_paths), every output array bit for bit.

  canyon       the street canyon (234 triangles: launch 0's cell masks, the patch-table walks of the trace, image and
               records kernels) at 20 000 rays and 4 bounces
  gen65        a generated scene of 65 triangles, tilted: the smallest table with patch tables
  gen256       a generated scene of 256 triangles: the largest
  cars         2cars.hrt (at most 64 triangles: the fused bodies and the chain kernel, the per-cell masks) at 20 000
               rays and 6 bounces

Each case is a process of its own (tests/staged_scenes_child.py) under a time limit."""
import os
import subprocess
import sys

import pytest

from tests import configs as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120
CASES = ["canyon", "gen65", "gen256", "cars"]


def case_config(name, tmp):
    if name == "canyon":
        return K.small(K.C3, 20000)
    if name == "cars":
        return K.small(K.C4, 20000)
    from tests import scenes_gen as G
    from tests.candidates_util import GEN_TX, GENERATED, generated_scene
    key = {"gen65": "gen65_tilt", "gen256": "gen256"}[name]
    p = os.path.join(str(tmp), name + ".hrt")
    rx, _, _ = generated_scene(p, **GENERATED[key])
    return G.cfg(p, rx, GEN_TX[:1], 20000, 4)


def test_the_cases_are_what_they_are_named_for(tmp_path):
    """No GPU: the tables' sizes (which walk a problem gets is decided by them), the depths, and that more than a
    chunk of rays is alive behind the first three launches (2cars is open: its rays leave within a few bounces), so the
    primary walks of launch 0 and of later launches and the shadow walks all run on full and on partial waves."""
    from oracle import oracle
    from oracle.oracle import read_hrt
    want = dict(canyon=(65, 256, 4), gen65=(65, 65, 4), gen256=(256, 256, 4), cars=(1, 64, 6))
    for name in CASES:
        c = case_config(name, tmp_path)
        n_tri = sum(len(m["idx"]) for m in read_hrt(c["scene_path"]))
        lo, hi, nb = want[name]
        assert lo <= n_tri <= hi and c["num_bounces"] == nb and c["num_paths"] == 20000, (name, n_tri)
        live = [int(x) for x in oracle.compute_paths(*K.args(c))["extras"]["live"]]
        assert len(live) == nb + 1 and live[1] > 256 and live[2] > 64, (name, live)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_scene_is_bit_identical_to_the_oracle(name, tmp_path):
    p = subprocess.run([sys.executable, "-m", "tests.staged_scenes_child", name, str(tmp_path)], cwd=REPO,
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    assert p.returncode == 0 and "STAGED_OK " + name in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
