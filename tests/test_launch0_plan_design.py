"""The launch plan's image of launch 0 on patch tables (csrc/hrt_launch_plan.h: fused0_txcell, fused0_words, lds_fused0;
DESIGN.md 5.1 and 5.6), built for the HOST like tests/test_launch_plan_design.py: the sum of its named terms, the seventh
of a CU it has to stay within, where the two word tables are in, and that nothing the plan answered before depends on
the new inputs.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB = 1024
SEVENTH = 160 * KIB // 7   # 23 405

IN = ["variant", "T", "num_leaf", "big", "fine_built", "mask", "num_img", "lds_max", "staged_max", "num_rx", "num_mesh", "nb",
      "num_tx", "txcell", "cell_mask"]
OLD = ["tri_bytes", "in_lds", "one_block", "trees", "fine", "trace_v", "fused_v", "chain_v", "own_records", "image",
       "shade_lds_normals", "cnt_per_wave", "t_rows", "t_table", "t_rx", "t_masks", "t_scratch", "t_mat_exp", "t_tx", "t_orig",
       "t_normals", "lds_trace", "lds_fused", "lds_chain", "lds_records", "lds_image", "lds_shade"]
NEW = ["fused0_txcell", "fused0_words", "t_mat0", "t_tx0", "t_words0", "lds_fused0"]
PER_LAUNCH = ["own@1", "image@1", "fuses@0", "fuses@1", "chains@1"]
COLS = OLD + NEW + PER_LAUNCH

_SRC = r"""
#include "hrt_launch_plan.h"
void probe_plan0(const long long *in, long long *out, long n)
{
    static const float built = 0.f;
    static const unsigned long long masks = 0u;
    for (long i = 0; i < n; ++i, in += %d, out += %d) {
        hrt_kparams K;
        memset(&K, 0, sizeof K);
        K.tune.variant = (int32_t)in[0];
        K.num_tri = (uint32_t)in[1];
        K.acc.num_leaf = (uint32_t)in[2];
        K.acc.big = (uint32_t)in[3];
        K.acc.fine = in[4] ? &built : NULL;
        K.patch.mask = in[5] ? &masks : NULL;
        K.patch.num_img = (uint32_t)in[6];
        K.tune.lds_tri_bytes_max = (uint64_t)in[7];
        K.tune.fuse_staged_max_tri = (uint32_t)in[8];
        K.num_rx = (uint32_t)in[9];
        K.num_mesh = (uint32_t)in[10];
        K.num_bounces = (uint32_t)in[11];
        K.num_tx = (uint32_t)in[12];
        K.patch.txcell = in[13] ? &masks : NULL;
        K.rxt.cell_mask = in[14] ? &masks : NULL;
        const hrt_launch_plan p = hrt_plan(&K);
        const long long v[] = {(long long)p.tri_bytes, p.in_lds, p.one_block, p.trees, p.fine, p.trace_v, p.fused_v, p.chain_v,
            p.own_records, p.image, p.shade_lds_normals, p.cnt_per_wave, (long long)p.t_rows, (long long)p.t_table,
            (long long)p.t_rx, (long long)p.t_masks, (long long)p.t_scratch, (long long)p.t_mat_exp, (long long)p.t_tx,
            (long long)p.t_orig, (long long)p.t_normals, (long long)p.lds_trace, (long long)p.lds_fused, (long long)p.lds_chain,
            (long long)p.lds_records, (long long)p.lds_image, (long long)p.lds_shade,
            p.fused0_txcell, p.fused0_words, (long long)p.t_mat0, (long long)p.t_tx0, (long long)p.t_words0,
            (long long)p.lds_fused0,
            hrt_plan_own_records(&p, 1u), hrt_plan_image(&p, 1u), hrt_plan_fuses(&p, 0u), hrt_plan_fuses(&p, 1u),
            hrt_plan_chains(&p, 1u, K.num_bounces)};
        for (unsigned k = 0; k < sizeof v / sizeof v[0]; ++k) out[k] = v[k];
    }
}
""" % (len(IN), len(COLS))


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plan0")
    src, so = os.path.join(str(tmp), "plan0_probe.c"), os.path.join(str(tmp), "libplan0_probe.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["cc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"), src, "-o", so, "-lm"])
    return C.CDLL(so)


def plans(H, rows):
    a = np.ascontiguousarray(rows, np.int64).reshape(-1, len(IN))
    out = np.zeros((a.shape[0], len(COLS)), np.int64)
    p64 = C.POINTER(C.c_longlong)
    H.probe_plan0(a.ctypes.data_as(p64), out.ctypes.data_as(p64), C.c_long(a.shape[0]))
    return {c: out[:, k] for k, c in enumerate(COLS)}


def plan(H, **kw):
    """one plan of a patch-table problem under the default tune unless overridden"""
    d = dict(variant=7, T=234, num_leaf=None, big=0, fine_built=0, mask=1, num_img=1, lds_max=40 * KIB, staged_max=6,
             num_rx=1, num_mesh=10, nb=4, num_tx=1, txcell=1, cell_mask=0)
    d.update(kw)
    if d["num_leaf"] is None:
        d["num_leaf"] = (d["T"] + 63) // 64
    return {k: int(v[0]) for k, v in plans(H, [[d[k] for k in IN]]).items()}


def pad16(n):
    return (n + 15) // 16 * 16


def test_the_canyon_with_one_tx_holds_both_word_tables_within_a_seventh(H):
    a = plan(H, T=234, num_tx=1)
    assert (a["fused0_txcell"], a["fused0_words"]) == (1, 1)
    assert (a["t_rows"], a["t_mat0"], a["t_tx0"], a["t_words0"]) == (18720, 1088, 16, 944)
    assert a["lds_fused0"] == 18720 + 256 + 1088 + 16 + 2 * 944 == 21968 <= SEVENTH
    assert a["lds_fused"] == 25920 and 160 * KIB // a["lds_fused"] == 6 and 160 * KIB // a["lds_fused0"] == 7
    b = plan(H, T=234, num_tx=64)   # every TX slot of the shared image: still within a seventh
    assert (b["fused0_words"], b["t_tx0"], b["lds_fused0"]) == (1, 1024, 22976) and b["lds_fused0"] <= SEVENTH
    c = plan(H, T=234, num_tx=65)   # the slots end at HRT_LDS_TX
    assert (c["t_tx0"], c["lds_fused0"]) == (1024, 22976)


def test_the_largest_patch_table_leaves_the_words_out(H):
    a = plan(H, T=256, num_tx=1)
    assert (a["fused0_txcell"], a["fused0_words"], a["t_words0"]) == (1, 0, 0)
    assert a["lds_fused0"] == 256 * 80 + 256 + 1088 + 16 == 21840 <= SEVENTH
    assert a["lds_fused0"] + 2 * 1024 > SEVENTH
    b = plan(H, T=65, num_tx=2)
    assert (b["fused0_words"], b["t_words0"], b["lds_fused0"]) == (1, 272, 65 * 80 + 256 + 1088 + 32 + 544)


def test_the_instantiation_is_launch_0_of_the_staged_flat_walk_with_a_tx_cell_table_and_no_cell_masks(H):
    assert plan(H)["fused0_txcell"] == 1
    for kw in (dict(txcell=0), dict(cell_mask=1), dict(lds_max=0), dict(big=1), dict(variant=4), dict(variant=1),
               dict(T=1025, lds_max=144 * KIB), dict(T=234, lds_max=0, fine_built=1)):
        p = plan(H, **kw)
        assert [p[k] for k in NEW] == [0] * len(NEW), kw
    for v in (2, 3, 7):
        assert plan(H, variant=v)["fused0_txcell"] == 1, v


T_GRID = [1, 6, 7, 64, 65, 128, 234, 249, 250, 251, 256, 257, 512, 513, 1024, 1025, 100002]


@pytest.fixture(scope="module")
def grid(H):
    rows = []
    for v, T, big, fine, mask, lds_max, ntx, txcell, cmask in itertools.product(
            range(10), T_GRID, (0, 1), (0, 1), (0, 1), (0, 40 * KIB, 144 * KIB), (1, 2, 63, 64, 65, 200), (0, 1), (0, 1)):
        rows.append((v, T, (T + 63) // 64, big, fine, mask, mask, lds_max, 6, 3, 10, 3, ntx, txcell, cmask))
    a = np.array(rows, np.int64)
    g = plans(H, a)
    g.update({k: a[:, i] for i, k in enumerate(IN)})
    return g


def test_lds_fused0_is_the_sum_of_its_named_terms_and_never_above_lds_fused(grid):
    g = grid
    on = g["fused0_txcell"] == 1
    assert on.any() and (~on).any()
    assert np.array_equal(on, (g["fused_v"] == 2) & (g["in_lds"] == 1) & (g["txcell"] == 1) & (g["cell_mask"] == 0))
    for k in NEW:
        assert np.all(g[k][~on] == 0), k
    assert np.all(g["t_mat0"][on] == 17 * 16 * 4)
    assert np.array_equal(g["t_tx0"][on], np.minimum(g["num_tx"], 64)[on] * 16)
    assert np.array_equal(g["t_words0"][on], np.where(g["fused0_words"] == 1, (g["T"] * 4 + 15) // 16 * 16, 0)[on])
    assert np.array_equal(g["lds_fused0"], np.where(on, g["t_rows"] + 256 + g["t_mat0"] + g["t_tx0"] + 2 * g["t_words0"], 0))
    assert np.all(g["lds_fused0"] <= g["lds_fused"])
    assert np.all(g["fuses@0"][on] == 1)   # the launch the image is for runs fused


def test_the_words_are_out_exactly_where_they_would_push_the_image_above_a_seventh(grid):
    g = grid
    on = g["fused0_txcell"] == 1
    base = g["t_rows"] + 256 + 1088 + np.minimum(g["num_tx"], 64) * 16
    with_words = base + 2 * ((g["T"] * 4 + 15) // 16 * 16)
    assert np.array_equal(g["fused0_words"][on], (with_words <= SEVENTH)[on].astype(np.int64))
    w = on & (g["fused0_words"] == 1)
    assert w.any() and g["lds_fused0"][w].max() <= SEVENTH
    # a table with the words in has at most 250 rows: a word per thread at staging (fused0_stage)
    assert g["T"][w].max() == 250
    assert plan_row(g, T=250, num_tx=1)["fused0_words"] == 1 and plan_row(g, T=251, num_tx=1)["fused0_words"] == 0


def plan_row(g, **kw):
    sel = (g["variant"] == 7) & (g["big"] == 0) & (g["fine_built"] == 0) & (g["mask"] == 1) & (g["lds_max"] == 40 * KIB) & \
          (g["txcell"] == 1) & (g["cell_mask"] == 0)
    for k, v in kw.items():
        sel &= g[k] == v
    i = np.flatnonzero(sel)
    assert i.size == 1, kw
    return {k: int(v[i[0]]) for k, v in g.items()}


def test_nothing_the_plan_answered_before_depends_on_the_new_inputs(H, grid):
    """Every earlier field over the grid: the same whatever num_tx, the TX cell table and the per-cell masks are (the
    parent's plan read none of them), and the parent's written-out answers of tests/test_launch_plan_design.py."""
    g = grid
    key = np.stack([g[k] for k in IN[:12]], 1)
    _, inv = np.unique(key, axis=0, return_inverse=True)
    inv = inv.ravel()
    first = np.zeros(inv.max() + 1, np.int64)
    first[inv[::-1]] = np.arange(inv.size)[::-1]
    for k in OLD + PER_LAUNCH:
        assert np.array_equal(g[k], g[k][first[inv]]), k
    a = plan(H, T=234, mask=1, num_leaf=4, num_rx=4, num_mesh=10, num_img=0)
    assert (a["tri_bytes"], a["lds_trace"], a["lds_fused"], a["lds_records"], a["lds_image"], a["lds_shade"]) == \
        (20720, 23360, 25968, 21064, 18736, 5344)
    walk = g["t_table"] + g["t_rx"] + g["t_masks"] + g["t_scratch"]
    assert np.array_equal(g["lds_fused"], walk + 256 + g["t_mat_exp"] + g["t_tx"]) and np.all(g["t_tx"] == 1024)
    assert np.array_equal(g["lds_chain"], g["lds_fused"])
    assert np.array_equal(g["lds_records"], g["t_rows"] + g["t_rx"] + g["t_mat_exp"] + g["t_orig"])
