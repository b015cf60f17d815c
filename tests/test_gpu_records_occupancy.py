"""hrt_records_kernel (csrc/hrt_kernels.hip) on the shapes where its per-receiver loop can go wrong: the masks of RX
r + 1 are requested in front of the walk of RX r and consumed behind it, in front of the record stores, and expf's table
comes from the kernel's LDS image.  Every case is the product against the CPU port (oracle.compute_paths), every
output array bit for bit, on the street canyon (234 triangles: patch tables, the records kernel) at about 20 000
rays per TX and 4 bounces:

  rx1, rx3, rx5     1, 3 and 5 receivers (with one there is no next receiver to request for)
  tail1, tail65     ray counts whose first live list ends in a chunk of 1 and of 65 entries: a wave with one lane,
                    a partial wave, and waves entirely past the end (the oracle's live counts are asserted)
  doppler           the c3_doppler velocities: the ray's direction and the mesh velocities reach freq_shift
  in_plane          a receiver inside a triangle's plane
  no_overlap        HRT_OVERLAP=0: one stream
  timer             HIP events around every kernel (Tracer.trace_with_timer)
  gen256            a generated scene of 256 triangles (the largest table with patch tables: the LDS image's bound)

Each case is a process of its own (tests/records_occupancy_child.py)."""
import os
import subprocess
import sys

import pytest

from tests import configs as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 120

RX5 = K.C3_RX + [[20, 4.0, 2.0]]
TAIL = {"tail1": (20096, 1), "tail65": (20178, 65)}   # ray count -> entries in the last chunk of launch 1's list


def case_config(name, tmp):
    """-> (config, "dense" | "timer")"""
    base = K.small(K.C3, 20000)
    if name in ("rx1", "rx3", "rx5"):
        rx = {"rx1": K.C3_RX[:1], "rx3": K.C3_RX[:3], "rx5": RX5}[name]
        return K.cfg("simple_street_canyon_with_cars.hrt", rx, base["tx_pos"], 3.5, 20000, 4), "dense"
    if name in TAIL:
        return K.small(K.C3, TAIL[name][0]), "dense"
    if name == "doppler":
        return K.small(K.C3_DOPPLER, 20000), "dense"
    if name == "in_plane":   # z = 0: the plane of the street's triangles
        return K.cfg("simple_street_canyon_with_cars.hrt", K.C3_RX[:3] + [[-10, 1.5, 0]], base["tx_pos"], 3.5, 20000, 4), "dense"
    if name == "no_overlap":
        return base, "dense"
    if name == "timer":
        return base, "timer"
    if name == "gen256":
        from tests import scenes_gen as G
        from tests.candidates_util import GEN_TX, GENERATED, generated_scene
        p = os.path.join(str(tmp), "gen256.hrt")
        rx, _, _ = generated_scene(p, **GENERATED["gen256"])
        return G.cfg(p, rx + [[-3, 9, 4.0]], GEN_TX[:1], 20000, 4), "dense"
    raise KeyError(name)


CASES = ["rx1", "rx3", "rx5", "tail1", "tail65", "doppler", "in_plane", "no_overlap", "timer", "gen256"]


def test_the_tail_cases_end_in_chunks_of_1_and_65(tmp_path):
    """No GPU: the oracle's live counts of the two tail cases (256 entries per chunk), and rays survive to every launch
    of every case."""
    from oracle import oracle
    for name in CASES:
        c, _ = case_config(name, tmp_path)
        live = [int(x) for x in oracle.compute_paths(*K.args(c))["extras"]["live"]]
        assert len(live) == 5 and all(n > 256 for n in live), (name, live)
        if name in TAIL:
            assert live[1] % 256 == TAIL[name][1], (name, live)
    c, _ = case_config("gen256", tmp_path)
    assert len(c["rx_pos"]) == 4


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_records_are_bit_identical_to_the_oracle(name, tmp_path):
    env = dict(os.environ)
    if name == "no_overlap":
        env["HRT_OVERLAP"] = "0"
    p = subprocess.run([sys.executable, "-m", "tests.records_occupancy_child", name, str(tmp_path)], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    assert p.returncode == 0 and "RECORDS_OK " + name in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
