"""The primary rays of launches >= 2 on patch tables as their own instantiation of hrt_trace_kernel (PATCH: no launch-0
ray generation, no shadow units, no per-cell masks, an LDS image of rows, mask words and counters) on
whole scenes: the product through the C ABI against the CPU port (oracle.compute_paths), every output array, the
live-list lengths and the LoS block bit for bit.

Scenes: the street canyon (234 triangles), gen65 and gen256 (the largest patch table: seven workgroups per CU, the
others eight).  One RX unless the case says otherwise.  Per scene:

  r1000     1 000 rays, 3 bounces: launch 2 walks a list of a few hundred entries -- a partial wave, a partial chunk
  r65537    65 537 rays, 3 bounces: many chunks at launch 2, the last one partial
  tx2       2 TXs at 1 000 rays, 4 bounces: launches 2 and 3
  tx65      65 TXs at 300 rays, 4 bounces

and the canyon with 4 RXs and 4 bounces at 20 000 rays (`deep`: launches 2 and 3, four records streams beside them);
`tie` at 65 537 rays and 3 bounces: the room of tests/test_gpu_launch0_patch.py whose walls are given twice, so that every
wall hit is an exact tie which the reference-order words decide; and the canyon at 20 000 rays and 3 bounces with fused
launches switched off (`nofuse`, HRT_FUSE=0): launch 0 is then the shared instantiation of the same kernel and launch 1
the image kernel, as the plan says (hrt_plan_trace_patch is 0 at launches 0 and 1), and the results are the same bits.
Each case is a process of its own (tests/trace_patch_child.py) under a time limit; it asserts that the plan sends
launches >= 2 to the instantiation under test, that the tables which make it so are built at this size (HRT_TUNE
rxt_min_rays=0, as tests/conftest.py sets it for the suite), that those launches had entries to walk and that no kernel was
switched off (hrt_fallback_state() == 0; an error word that is not clean fails the call itself)."""
import os
import subprocess
import sys

import pytest

from tests import scenes_gen as G
from tests import test_gpu_launch0_patch as L0

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120
SCENES = {"canyon": 234, "gen65": 65, "gen256": 256}
SHAPES = {"r1000": (1, 1000, 3), "r65537": (1, 65537, 3), "tx2": (2, 1000, 4), "tx65": (65, 300, 4)}   # TXs, rays, bounces
CASES = ["%s-%s" % (s, k) for s in SCENES for k in SHAPES] + ["canyon-deep", "tie-r65537", "canyon-nofuse"]


def case_config(name, tmp):
    """(config, environment of the child beyond the caller's)"""
    scene, shape = name.split("-")
    base = L0.case_config(scene + "-r65537" if scene == "tie" else scene + "-r1000", tmp)   # scene file, one RX, one TX
    path, rx, tx0, f = base["scene_path"], [list(p) for p in base["rx_pos"]], list(base["tx_pos"][0]), base["f_ghz"]
    if shape == "deep":
        rx4 = [[rx[0][0] + 0.5 * i, rx[0][1], rx[0][2]] for i in range(4)]
        return G.cfg(path, rx4, [tx0], 20000, 4, f=f), {}
    if shape == "nofuse":
        return G.cfg(path, rx, [tx0], 20000, 3, f=f), {"HRT_FUSE": "0"}
    ntx, rays, nb = SHAPES[shape]
    return G.cfg(path, rx, L0.tx_positions(tx0, ntx), rays, nb, f=f), {}


def test_the_cases_are_what_they_are_named_for(tmp_path):
    """No GPU: the tables' sizes, and that the lists which launches 2 (and 3) walk are of the lengths the cases are for."""
    from oracle import oracle
    from oracle.oracle import read_hrt
    from tests import configs as K
    assert len(CASES) == 15
    for scene, n_tri in SCENES.items():
        c, env = case_config(scene + "-r1000", tmp_path)
        assert env == {} and c["num_bounces"] == 3 and len(c["rx_pos"]) == 1
        assert sum(len(m["idx"]) for m in read_hrt(c["scene_path"])) == n_tri, scene
        live = [int(x) for x in oracle.compute_paths(*K.args(c))["extras"]["live"]]
        # launch 2's list: more than one wave, and either a partial last wave or a partial last chunk
        # (the generated rooms are closed: every ray is still alive there)
        assert live[0] == 1000 and 64 < live[2] <= 1000 and live[2] % 64 != 0 and live[2] % 256 != 0, (scene, live)
    c, _ = case_config("canyon-tx2", tmp_path)
    assert (len(c["tx_pos"]), c["num_paths"], c["num_bounces"]) == (2, 1000, 4)
    c, _ = case_config("gen65-tx65", tmp_path)
    assert (len(c["tx_pos"]), c["num_paths"], c["num_bounces"]) == (65, 300, 4)
    c, _ = case_config("canyon-deep", tmp_path)
    assert (len(c["rx_pos"]), c["num_bounces"], c["num_paths"]) == (4, 4, 20000)
    c, env = case_config("canyon-nofuse", tmp_path)
    assert env == {"HRT_FUSE": "0"} and c["num_bounces"] == 3
    c, _ = case_config("tie-r65537", tmp_path)
    assert sum(len(m["idx"]) for m in read_hrt(c["scene_path"])) == L0.TIE_TRI and c["num_bounces"] == 3
    assert -(-65537 // 256) == 257 and 65537 % 256 == 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_later_launches_are_bit_identical_to_the_oracle(name, tmp_path):
    _, extra = case_config(name, tmp_path)
    # (HRT_TUNE stays as tests/conftest.py set it: rxt_min_rays=0, without which a problem of this few rays gets no tables)
    env = {k: v for k, v in os.environ.items() if k != "HRT_FUSE"}
    env.update(extra)
    p = subprocess.run([sys.executable, "-m", "tests.trace_patch_child", name, str(tmp_path)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    print(p.stdout[-1500:])
    assert p.returncode == 0 and "TRACE_PATCH_OK " + name in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
