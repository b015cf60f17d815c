"""The pencil filter of the patch masks as the design study restates it on the host (profiles/study/cand.c:
product_patch, pencil_culls -- the arithmetic of csrc/hrt_kernels.hip's Pencil / pencil_culls, DESIGN_ACCEL.md A.5 items 4-6).

A NECESSARY condition of soundness, not a proof (the proof is the argument in A.5): on the canyon, for every (patch, RX),
every triangle that any of 9 x 9 origins sampled over the patch's prism -- the cell enlarged by HRT_PATCH_MARGIN on every
side, heights cycling through -hball, 0, +hball, the four (u, v) corners at all three -- hits on its line to the RX, at any distance in front of the origin, is in the restated
mask.  Hits are decided in double with 1e-9 slack (strictly inside the triangle, strictly in front).  All patches at
patch_size 2.0 (43 k patches x 4 RX); at the default 0.5 (692 k patches) a SAMPLE: every 47th patch, which keeps the
test at seconds (47 is prime to every grid width, so the sample runs through all columns and rows of the big grids, rim
cells included).  No GPU."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

from . import configs as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def study(tmp_path_factory):
    spec = importlib.util.spec_from_file_location("hrt_study", os.path.join(REPO, "profiles", "study", "study.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.load_lib(str(tmp_path_factory.mktemp("study")))
    return m


@pytest.mark.parametrize("size,stride", [(2.0, 1), (0.5, 47)])
def test_sampled_hits_are_in_the_restated_mask(study, size, stride):
    S, c = study, K.IN_PLANE["canyon"]
    rows, _ = S.rows_of(c["scene_path"])
    T = len(rows)
    W = (T + 63) // 64
    rx = np.asarray(c["rx_pos"], np.float32)
    k = S.product_consts(rows, rx, c["tx_pos"])
    pd, npatch = S.product_grid(rows, size)
    u64p = C.POINTER(C.c_uint64)
    total = 0
    for a in range(len(rx)):
        mask, cone, hits = (np.zeros((npatch, W), np.uint64) for _ in range(3))
        S.L.build_patch_table_product(S.P(rows), T, pd, S.P(rx[a]), 0, C.c_float(k["ro_rx"]), 1, C.c_float(k["hball"]), 1, stride, S.P(mask, u64p))
        S.L.build_patch_table_product(S.P(rows), T, pd, S.P(rx[a]), 0, C.c_float(k["ro_rx"]), 1, C.c_float(k["hball"]), 0, stride, S.P(cone, u64p))
        S.L.sample_patch_table(S.P(rows), T, pd, S.P(rx[a]), 0, 1, 9, C.c_double(0.0625), C.c_double(float(k["hball"])), C.c_double(1e-9),
                               stride, S.P(hits, u64p))
        assert not (mask & ~cone).any(), "the pencil mask has a bit the cone mask lacks"
        lost = np.flatnonzero((hits & ~mask).any(axis=1))
        assert lost.size == 0, "rx %d, patch size %g: %d patches lack a triangle a sampled origin hits, first patch %d" % (a, size, lost.size, lost[0])
        total += int(S.popc_rows(hits).sum())
        assert S.popc_rows(mask).sum() < S.popc_rows(cone).sum(), "the pencil removes nothing"
    assert total > 0, "no sampled origin hits anything: the check is empty"
