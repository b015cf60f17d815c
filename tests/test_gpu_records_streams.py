"""The records streams of a trace on the GPU (csrc/host/problem.c: trace_impl): launch b >= 1 runs its
records kernel on stream (b - 1) mod A, at the lowest priority, beside the bounce kernels and beside its neighbours'
records kernels, and the caller's stream joins every stream used.  Every case is the product against the CPU port
(oracle.compute_paths), every output array bit for bit, on the street canyon (234 triangles: patch tables, the records
kernel), one process per case (tests/records_streams_child.py):

  nb1               20 000 rays, 1 bounce: one records launch, one stream used
  nb2               2 bounces: both streams, none twice
  nb5               5 bounces: stream 0 takes launches 1, 3 and 5; the late lists are short (2 345 and 1 173 entries)
  tiny              300 rays, 4 bounces: every list inside one chunk of 256 entries (246, 152, 76, 35)
  empty             100 rays, 12 bounces: lists of a few entries, of one entry, and three EMPTY ones at the end (300
                    rays at 4 bounces do not reach an empty list)
  rx5               5 receivers, 20 000 rays, 4 bounces: theta carried across an odd count of receivers
  a1, a3            HRT_TUNE aux_streams=1 / 3 on the nb5 shape
  noprio            aux_prio=0 on the nb5 shape: the streams at the default priority
  parent            HRT_OVERLAP=1 on the nb5 shape: one stream at the default priority
  back_to_back      the device-resident Tracer on the nb5 shape: blocks poisoned, a trace, then five (poison, trace) with
                    no synchronisation, only the caller's stream synchronised: every word as after the first trace"""
import os
import subprocess
import sys

import pytest

from tests import configs as K
from tests.test_gpu_records_occupancy import REPO, RX5, STEP_TIMEOUT_S

CANYON = "simple_street_canyon_with_cars.hrt"
SHAPES = {"nb1": (20000, 1), "nb2": (20000, 2), "nb5": (20000, 5), "tiny": (300, 4), "empty": (100, 12)}
SWITCHES = {"a1": {"HRT_TUNE": "aux_streams=1"}, "a3": {"HRT_TUNE": "aux_streams=3"}, "noprio": {"HRT_TUNE": "aux_prio=0"},
            "parent": {"HRT_OVERLAP": "1"}}
CASES = ["nb1", "nb2", "nb5", "tiny", "empty", "rx5", "a1", "a3", "noprio", "parent", "back_to_back"]


def case_config(name):
    """-> (config, "dense" | "back_to_back")"""
    base = K.small(K.C3, 20000)
    if name == "rx5":
        return K.cfg(CANYON, RX5, base["tx_pos"], 3.5, 20000, 4), "dense"
    n, nb = SHAPES.get(name, SHAPES["nb5"])
    c = K.cfg(CANYON, base["rx_pos"], base["tx_pos"], 3.5, n, nb)
    return c, ("back_to_back" if name == "back_to_back" else "dense")


def test_the_shapes_reach_what_they_are_for():
    """No GPU: the oracle's live lists of the cases."""
    from oracle import oracle
    live = {}
    for name in ("nb1", "nb2", "nb5", "tiny", "empty", "rx5"):
        c, _ = case_config(name)
        live[name] = [int(x) for x in oracle.compute_paths(*K.args(c))["extras"]["live"]]
    assert live["nb1"] == [20000, 16312] and live["nb2"] == [20000, 16312, 10109]
    assert live["nb5"] == [20000, 16312, 10109, 5037, 2345, 1173]      # 64, 40, 20, 10 and 5 chunks: records launches 1 .. 5
    assert live["tiny"] == [300, 246, 152, 76, 35]                       # every records launch: one partial chunk
    assert live["empty"] == [100, 81, 52, 24, 13, 6, 4, 3, 1, 1, 0, 0, 0]
    assert live["rx5"] == live["nb5"][:5] and len(case_config("rx5")[0]["rx_pos"]) == 5
    for name in ("a1", "a3", "noprio", "parent", "back_to_back"):
        assert case_config(name)[0] == case_config("nb5")[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_records_on_their_streams_are_bit_identical_to_the_oracle(name):
    env = {k: v for k, v in os.environ.items() if k not in ("HRT_TUNE", "HRT_OVERLAP")}
    env.update(SWITCHES.get(name, {}))
    p = subprocess.run([sys.executable, "-m", "tests.records_streams_child", name], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=STEP_TIMEOUT_S)
    assert p.returncode == 0 and "STREAMS_OK " + name in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
