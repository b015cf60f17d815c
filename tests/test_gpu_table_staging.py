"""The staging of the per-problem tables into LDS (stage_load / stage_store / stage_rest in
csrc/hrt_kernels.hip): every kernel requests a batch of every table -- and its first entry's state -- before its
first wait, predicated on the tables' lengths.  A wrong bound there drops or invents a table row, so the
scenes put the lengths on the batches' edges, and every case is the product against the oracle, every
output array bit for bit.

The triangle table is HRT_ROW * T = 5 T float4, copied 5 * 256 float4 (256 triangles) per batch and 256 per
instruction; guard pairs, reference-order indices and the shade kernel's normals are T items, copied 256
(512: guard pairs, normals) per batch.  5 T is one below / one above a multiple of 256 for T = 51, 563 /
205, 717 and a multiple of the batch for T = 256, 512; T itself is one below, at and one above 256 and 512.
Each kernel family gets such tables:
  * at most 64 triangles (fused bounces): 51, 52, 64;
  * 65 .. 256 (records, image, trace and shade kernels): 204, 205, 255, 256;
  * 257 .. 1 024 (the trace and shade pair): 257, 511, 512 staged; 513, 563, 717 staged when `lds_tri_bytes` allows;
  * the table read from global memory (`lds_tri_bytes=0`): all of them.
1, 4 and 8 RXs, two TXs in one case.  The staging is latched per process: subprocesses."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import scenes_gen as G
from tests.tune import tuned

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RXS = [[5, 3, 1.5], [-8, -4, 2.0], [12, 9, 8.0], [-15, 10, 3.0], [3, -11, 6.5], [16, -9, 1.0], [-2, 1, 10.5],
       [9, -2, 4.0]]
RXV = [[1, 2, 0], [0, -3, 1], [2, 0, 0], [0, 0, 2], [-1, 1, 0], [3, 0, -1], [0, 2, 2], [1, -1, 1]]
TXS = [[-10, 5, 6.0], [11, -7, 9.0]]

# name: (triangles, RXs, TXs, rays per TX, bounces)
CASES = {
    "t51_rx1": (51, 1, 1, 4000, 3), "t52_rx4": (52, 4, 1, 4000, 3), "t64_rx8": (64, 8, 1, 3000, 3),
    "t204_rx4": (204, 4, 1, 4000, 3), "t205_rx1": (205, 1, 1, 4000, 3), "t255_rx8": (255, 8, 1, 3000, 3),
    "t256_rx4_tx2": (256, 4, 2, 3000, 3),
    "t257_rx4": (257, 4, 1, 3000, 3), "t511_rx1": (511, 1, 1, 3000, 2), "t512_rx8": (512, 8, 1, 2000, 2),
    "t513_rx4": (513, 4, 1, 3000, 2), "t563_rx4_tx2": (563, 4, 2, 2000, 2), "t717_rx1": (717, 1, 1, 3000, 2),
}


def scene(path, num_tri, seed):
    """A 40 x 30 x 12 m room with tilted boxes in it (tests/scenes_gen.room_with_clutter's) and a padding mesh of
    small free-standing triangles that brings the table to exactly `num_tri` rows.  Materials cycle, odd meshes move."""
    rng = np.random.default_rng(seed)
    n_boxes = num_tri // 12 - 1
    v, f = G._box([0, 0, 6], [40, 30, 12])
    meshes = [dict(vs=v, idx=f, material_index=1, velocity=[0, 0, 0])]
    for i in range(n_boxes):
        c = rng.uniform([-18, -13, 0.5], [18, 13, 10])
        v, f = G._box(c, rng.uniform(0.3, 2.5, 3))
        a, b = rng.uniform(0, np.pi, 2)
        Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        v = ((v - c) @ (Rz @ Rx).T + c).astype(np.float32)
        meshes.append(dict(vs=v, idx=f, material_index=(i + 1) % 17, velocity=rng.uniform(-30, 30, 3) if i % 2 else np.zeros(3)))
    pad = num_tri - 12 * (n_boxes + 1)
    if pad:
        vs, idx = [], []
        for k in range(pad):   # shards of 1.5 m, each with a normal of its own
            c = rng.uniform([-15, -10, 1.0], [15, 10, 9.0])
            e = rng.normal(size=(2, 3))
            vs += [c, c + 1.5 * e[0] / np.linalg.norm(e[0]), c + 1.5 * e[1] / np.linalg.norm(e[1])]
            idx.append([3 * k, 3 * k + 1, 3 * k + 2])
        meshes.append(dict(vs=np.array(vs, np.float32), idx=np.array(idx, np.uint32), material_index=7, velocity=[2, -1, 0.5]))
    assert sum(len(m["idx"]) for m in meshes) == num_tri
    G.write_hrt(path, meshes)


def make(tmp, name):
    num_tri, n_rx, n_tx, rays, bounces = CASES[name]
    p = os.path.join(str(tmp), name + ".hrt")
    scene(p, num_tri, seed=num_tri)
    return G.cfg(p, RXS[:n_rx], TXS[:n_tx], rays, bounces, rx_vel=RXV[:n_rx], tx_vel=[[10, 0, 0], [0, -4, 1]][:n_tx])


def test_the_oracle_runs_the_cases(tmp_path):
    """No GPU: the scenes have the intended tables, and rays survive to every launch, so that every kernel of
    a case's family has entries to work on."""
    from oracle import oracle
    from tests import configs as K
    for name in CASES:
        c = make(tmp_path, name)
        ref = oracle.compute_paths(*K.args(c))
        live = [int(x) for x in ref["extras"]["live"]]
        assert len(live) == CASES[name][4] + 1 and all(n > 100 for n in live), (name, live)


CODE = r"""
import sys, tempfile
sys.path.insert(0, %(repo)r)
from hermespy_rt_amd import abi, lib
from oracle import oracle
from tests import configs as K
from tests.parity import compare_dense
from tests.test_gpu_table_staging import make, CASES
tmp = tempfile.mkdtemp()
for name in CASES:
    c = make(tmp, name)
    got = abi.run_compute_paths(lib.load(), *K.args(c))
    ref = oracle.compute_paths(*K.args(c))
    st = compare_dense(got, ref)
    print(name, st, [int(x) for x in ref["extras"]["live"]], flush=True)
    assert all(v == 0 for v in st.values()), (name, st)
print("STAGING_OK", len(CASES))
"""


@pytest.mark.gpu
@pytest.mark.parametrize("env", [
    dict(),                              # tables of up to 512 triangles staged, the larger ones read from global memory
    dict(lds_tri_bytes="147456"),        # every table staged (717 triangles: three batches)
    dict(lds_tri_bytes="0"),             # every table read from global memory
    dict(lds_tri_bytes="147456", variant="4"),   # ... staged with guard pairs and leaf records
], ids=["default", "all_staged", "global_table", "all_staged_leaves"])
def test_tables_on_batch_edges_are_bit_identical_to_the_oracle(env):
    p = subprocess.run([sys.executable, "-c", CODE % dict(repo=REPO)], env=tuned(**env),
                       capture_output=True, text=True)
    assert p.returncode == 0 and "STAGING_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
