"""The launch plan (csrc/hrt_launch_plan.h; DESIGN.md, "the launch plan") built for the HOST and asked through ctypes:
the rows of the decision table at their boundaries, with the expected answers written out, and the invariants that
keep two kernels from disagreeing, over a grid of inputs.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIB = 1024

IN = ["variant", "T", "num_leaf", "big", "fine_built", "mask", "num_img", "lds_max", "staged_max", "num_rx", "num_mesh", "nb"]
OUT = ["tri_bytes", "in_lds", "one_block", "trees", "fine", "trace_v", "fused_v", "chain_v", "own_records", "image",
       "shade_lds_normals", "cnt_per_wave", "t_rows", "t_table", "t_rx", "t_masks", "t_scratch", "t_mat_exp", "t_tx", "t_orig",
       "t_normals", "lds_trace", "lds_fused", "lds_chain", "lds_records", "lds_image", "lds_shade"]
BOUNCES = ["0", "1", "2", "nb"]                     # the launches the per-launch answers are taken at
PER_LAUNCH = ["own", "image", "fuses", "chains"]    # -> columns "own@1", "chains@nb", ...
COLS = OUT + ["%s@%s" % (q, b) for b in BOUNCES for q in PER_LAUNCH]

_SRC = r"""
#include "hrt_launch_plan.h"
void probe_plan(const long long *in, long long *out, long n)
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
        const hrt_launch_plan p = hrt_plan(&K);
        const long long v[] = {(long long)p.tri_bytes, p.in_lds, p.one_block, p.trees, p.fine, p.trace_v, p.fused_v, p.chain_v,
            p.own_records, p.image, p.shade_lds_normals, p.cnt_per_wave, (long long)p.t_rows, (long long)p.t_table,
            (long long)p.t_rx, (long long)p.t_masks, (long long)p.t_scratch, (long long)p.t_mat_exp, (long long)p.t_tx,
            (long long)p.t_orig, (long long)p.t_normals, (long long)p.lds_trace, (long long)p.lds_fused, (long long)p.lds_chain,
            (long long)p.lds_records, (long long)p.lds_image, (long long)p.lds_shade};
        long long *o = out;
        for (unsigned k = 0; k < sizeof v / sizeof v[0]; ++k) *o++ = v[k];
        const uint32_t bs[4] = {0u, 1u, 2u, K.num_bounces};
        for (int k = 0; k < 4; ++k) {
            *o++ = hrt_plan_own_records(&p, bs[k]);
            *o++ = hrt_plan_image(&p, bs[k]);
            *o++ = hrt_plan_fuses(&p, bs[k]);
            *o++ = hrt_plan_chains(&p, bs[k], K.num_bounces);
        }
    }
}
""" % (len(IN), len(COLS))


def host_build(tmp):
    """The header compiled for the host as C99 (the way tests/exp_table_util.py builds hrt_libm.h) as a ctypes library."""
    src, so = os.path.join(str(tmp), "plan_probe.c"), os.path.join(str(tmp), "libplan_probe.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["cc", "-std=c99", "-O2", "-Wall", "-Wextra", "-Werror", "-shared", "-fPIC",
                           "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"), src, "-o", so, "-lm"])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return host_build(tmp_path_factory.mktemp("plan"))


def plans(H, rows):
    """rows [n][len(IN)] -> dict of column -> int64 array"""
    a = np.ascontiguousarray(rows, np.int64).reshape(-1, len(IN))
    out = np.zeros((a.shape[0], len(COLS)), np.int64)
    p64 = C.POINTER(C.c_longlong)
    H.probe_plan(a.ctypes.data_as(p64), out.ctypes.data_as(p64), C.c_long(a.shape[0]))
    return {c: out[:, k] for k, c in enumerate(COLS)}


def plan(H, **kw):
    """one plan under the default tune (auto walk, 40 KiB of rows in LDS, staged walk up to 6 triangles) unless overridden;
    num_leaf defaults to one leaf per 64 rows"""
    d = dict(variant=7, T=100, num_leaf=None, big=0, fine_built=0, mask=0, num_img=0, lds_max=40 * KIB, staged_max=6,
             num_rx=3, num_mesh=10, nb=4)
    d.update(kw)
    if d["num_leaf"] is None:
        d["num_leaf"] = (d["T"] + 63) // 64
    return {k: int(v[0]) for k, v in plans(H, [[d[k] for k in IN]]).items()}


# ------------------------------------------------------------------ the decision table, row by row
def test_auto_spills_out_of_lds_between_512_and_513_triangles(H):
    """40 KiB of rows at 80 bytes per row"""
    a, b = plan(H, T=512), plan(H, T=513)
    assert (a["in_lds"], a["t_rows"], a["t_table"]) == (1, 40960, 40960 + 256 * 16 + 8 * 32)
    assert (b["in_lds"], b["t_rows"], b["t_table"]) == (0, 41040, 0)
    assert a["tri_bytes"] == 45312 and b["tri_bytes"] == 41040 + 257 * 16 + 9 * 32


def test_at_the_144_kib_limit_the_ceiling_on_the_whole_image_binds(H):
    """rows + guard pairs (16 B per two rows) + leaf records (32 B): 1843 rows fit the limit, their image does not"""
    big = 144 * KIB
    assert plan(H, T=1843, num_leaf=0, lds_max=big)["t_rows"] == 147440
    assert plan(H, T=1843, num_leaf=0, lds_max=big)["in_lds"] == 0
    assert plan(H, T=1844, num_leaf=0, lds_max=big)["in_lds"] == 0
    a, b = plan(H, T=1675, num_leaf=0, lds_max=big), plan(H, T=1676, num_leaf=0, lds_max=big)
    assert (a["in_lds"], a["tri_bytes"]) == (1, 147408) and (b["in_lds"], b["tri_bytes"]) == (0, 147488)
    a, b = plan(H, T=1665, num_leaf=27, lds_max=big), plan(H, T=1666, num_leaf=27, lds_max=big)
    assert (a["in_lds"], a["tri_bytes"]) == (1, 147392) and (b["in_lds"], b["tri_bytes"]) == (0, 147472)


def test_one_block_ends_at_1024_triangles(H):
    big = 144 * KIB
    a, b = plan(H, T=1024, lds_max=big), plan(H, T=1025, lds_max=big)
    assert (a["one_block"], a["in_lds"], a["trace_v"], a["fused_v"], a["chain_v"]) == (1, 1, 2, 2, 2)
    # (auto is the flat walk on one block only; beyond, the leaf spheres of several blocks, and no chain)
    assert (b["one_block"], b["in_lds"], b["trace_v"], b["fused_v"], b["chain_v"]) == (0, 1, 5, 5, -1)
    assert plan(H, T=1025, lds_max=big, variant=2)["trace_v"] == 3 and plan(H, T=1024, lds_max=big, variant=2)["trace_v"] == 2
    assert plan(H, T=1025, lds_max=big, variant=4)["trace_v"] == 5 and plan(H, T=1024, lds_max=big, variant=4)["trace_v"] == 4


def test_auto_fuses_on_the_staged_walk_up_to_6_triangles_and_the_flat_walk_from_7(H):
    a, b = plan(H, T=6), plan(H, T=7)
    assert (a["fused_v"], a["chain_v"], a["trace_v"]) == (1, 1, 2)   # (the trace kernel has no such rule)
    assert (b["fused_v"], b["chain_v"], b["trace_v"]) == (2, 2, 2)
    assert plan(H, T=6, staged_max=0)["fused_v"] == 2
    assert plan(H, T=6, variant=4)["fused_v"] == 4 and plan(H, T=100, variant=1)["fused_v"] == 1


def test_the_records_kernel_owns_launches_from_1_on_of_patch_tables_on_a_staged_one_block_flat_table(H):
    a = plan(H, T=234, mask=1)
    assert [a["own@" + b] for b in BOUNCES] == [0, 1, 1, 1] and a["own_records"] == 1
    for v, own in ((0, 0), (1, 0), (2, 1), (3, 1), (4, 0), (5, 0), (6, 0), (7, 1), (8, 0), (9, 0)):
        p = plan(H, T=234, mask=1, variant=v)
        assert [p["own@" + b] for b in BOUNCES] == [0, own, own, own], v
    assert plan(H, T=234, mask=0)["own_records"] == 0                          # no patch masks
    assert plan(H, T=234, mask=1, lds_max=0)["own_records"] == 0               # off LDS
    assert plan(H, T=1025, mask=1, lds_max=144 * KIB, variant=2)["own_records"] == 0   # flat, staged, two blocks
    assert plan(H, T=234, mask=1, big=1)["own_records"] == 0                   # auto walks the trees: not flat
    # the images it is launched with
    a = plan(H, T=234, mask=1, num_leaf=4, num_rx=4, num_mesh=10)
    assert (a["tri_bytes"], a["lds_trace"], a["lds_fused"], a["lds_records"], a["lds_image"], a["lds_shade"]) == \
        (20720, 23360, 25968, 21064, 18736, 5344)


def test_the_image_kernel_runs_at_launch_1_only_and_only_with_image_tables(H):
    a = plan(H, T=234, mask=1, num_img=1)
    assert [a["image@" + b] for b in BOUNCES] == [0, 1, 0, 0]
    assert all(plan(H, T=234, mask=1, num_img=0)["image@" + b] == 0 for b in BOUNCES)
    assert all(plan(H, T=234, mask=0, num_img=1)["image@" + b] == 0 for b in BOUNCES)


def test_the_fine_walk_makes_launch_0_unfusable_and_counts_per_wave(H):
    a = plan(H, T=100002, fine_built=1)
    assert (a["fine"], a["trace_v"], a["cnt_per_wave"], a["in_lds"]) == (1, 9, 1, 0)
    assert [a["fuses@" + b] for b in BOUNCES] == [0, 0, 0, 0]
    assert a["t_scratch"] == 4 * (32 + 4 * 64) * 16 and a["lds_trace"] == 3 * 16 + 512 + 18432 + 16   # the candidate buffer
    b = plan(H, T=100002, fine_built=0)
    assert (b["fine"], b["trace_v"], b["cnt_per_wave"], b["fuses@0"], b["t_scratch"]) == (0, 5, 0, 1, 2048)
    c = plan(H, T=100002, fine_built=1, big=1)   # the trees win
    assert (c["fine"], c["trees"], c["trace_v"], c["cnt_per_wave"], c["fuses@0"]) == (0, 1, 6, 0, 1)
    d = plan(H, T=100002, fine_built=1, variant=9, big=1)   # variant 9 asks for the fine walk whatever was built
    assert (d["fine"], d["trees"], d["trace_v"]) == (1, 0, 9)
    assert plan(H, T=100002, fine_built=1, variant=5)["fine"] == 0
    # fine leaves built for a small table that is kept out of LDS (accel_fine_min=0,lds_tri_bytes=0)
    e = plan(H, T=234, fine_built=1, mask=1, lds_max=0)
    assert (e["fine"], e["fuses@0"], e["own_records"], e["cnt_per_wave"]) == (1, 0, 0, 1)
    assert plan(H, T=234, fine_built=1)["fine"] == 0   # staged: never fine


def test_later_launches_fuse_on_staged_one_block_walks_only(H):
    for v, walk in ((0, 0), (1, 1), (2, 2), (3, 2), (4, 4), (5, 4), (6, 4), (7, 2), (8, 4), (9, 4)):
        p = plan(H, T=100, variant=v)
        assert p["fused_v"] == walk and [p["fuses@" + b] for b in BOUNCES] == [1, 1, 1, 1], v
        q = plan(H, T=100, variant=v, lds_max=0)   # off LDS: launch 0 alone
        assert [q["fuses@" + b] for b in BOUNCES] == [1, 0, 0, 0], v
    for v, walk in ((2, 3), (3, 3), (4, 5), (7, 5)):   # staged, two blocks
        p = plan(H, T=1025, variant=v, lds_max=144 * KIB)
        assert p["fused_v"] == walk and [p["fuses@" + b] for b in BOUNCES] == [1, 0, 0, 0], v
    p = plan(H, T=100, big=1)   # trees
    assert p["fused_v"] == 6 and [p["fuses@" + b] for b in BOUNCES] == [1, 0, 0, 0]


def test_the_chain_is_out_for_own_records_off_lds_beyond_one_block_and_under_trees(H):
    a = plan(H, T=40, nb=5)
    assert a["chain_v"] == 2 and [a["chains@" + b] for b in BOUNCES] == [0, 1, 1, 1]
    assert a["lds_chain"] == a["lds_fused"] == 40 * 80 + 20 * 16 + 32 + 48 + 512 + 2048 + 256 + 1344 + 1024
    assert plan(H, T=40, nb=1)["chains@2"] == 0                                                  # past the last launch
    assert [plan(H, T=40, variant=v)["chain_v"] for v in range(10)] == [0, 1, 2, 2, 4, 4, 4, 2, 4, 4]
    assert all(plan(H, T=234, mask=1)["chains@" + b] == 0 for b in BOUNCES)                      # own records
    assert all(plan(H, T=234, mask=0)["chains@" + b] == 1 for b in BOUNCES[1:])
    assert plan(H, T=40, lds_max=0)["chain_v"] == -1                                             # off LDS
    assert plan(H, T=1025, lds_max=144 * KIB)["chain_v"] == -1                                   # two blocks
    assert plan(H, T=40, big=1)["chain_v"] == -1 and plan(H, T=40, big=1)["chains@2"] == 0       # trees
    assert plan(H, T=6, big=1)["chain_v"] == 1                                                   # (staged walk: no trees walked)


# ------------------------------------------------------------------ invariants over a grid
T_GRID = [1, 6, 7, 64, 65, 256, 257, 511, 512, 513, 1024, 1025, 1843, 1844, 100002]
PATCH_MAX_TRI = 256   # hrt_kparams.h HRT_PATCH_MAX_TRI: the host builds patch masks for tables of 65 .. 256 triangles


@pytest.fixture(scope="module")
def grid(H):
    rows = []
    for v, T, leaf, big, fine, mask, img, lds_max, staged, nrx, nb in itertools.product(
            range(10), T_GRID, (0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 40 * KIB, 144 * KIB), (0, 6), (1, 5), (1, 3)):
        rows.append((v, T, (T + 63) // 64 if leaf else 0, big, fine, mask, img, lds_max, staged, nrx, 10, nb))
    a = np.array(rows, np.int64)
    g = plans(H, a)
    g.update({k: a[:, i] for i, k in enumerate(IN)})
    return g


def test_every_lds_size_is_the_sum_of_its_named_terms(grid):
    g = grid
    assert g["T"].size == 10 * 15 * 2 ** 5 * 3 * 2 * 2 * 2
    assert np.array_equal(g["t_rows"], g["T"] * 80)
    assert np.array_equal(g["tri_bytes"], g["T"] * 80 + (g["T"] + 1) // 2 * 16 + g["num_leaf"] * 32)
    assert np.array_equal(g["t_table"], np.where(g["in_lds"] == 1, g["tri_bytes"], 0))
    assert np.array_equal(g["t_rx"], g["num_rx"] * 16) and np.all(g["t_masks"] == 512) and np.all(g["t_tx"] == 1024)
    assert np.array_equal(g["t_scratch"], np.where(g["fine"] == 1, 18432, 2048)) and np.all(g["t_mat_exp"] == 1344)
    assert np.array_equal(g["t_orig"], g["T"] * 4)
    assert np.array_equal(g["t_normals"], np.where(g["shade_lds_normals"] == 1, (g["T"] + g["num_mesh"]) * 16, 0))
    walk = g["t_table"] + g["t_rx"] + g["t_masks"] + g["t_scratch"]
    assert np.array_equal(g["lds_trace"], walk + 16)
    assert np.array_equal(g["lds_fused"], walk + 256 + g["t_mat_exp"] + g["t_tx"])
    assert np.array_equal(g["lds_chain"], g["lds_fused"])
    assert np.array_equal(g["lds_records"], g["t_rows"] + g["t_rx"] + g["t_mat_exp"] + g["t_orig"])
    assert np.array_equal(g["lds_image"], g["t_rows"] + 16)
    assert np.array_equal(g["lds_shade"], g["t_mat_exp"] + g["t_rx"] + 32 + g["t_normals"])


def test_one_kernel_claims_the_records_of_a_launch(grid):
    """The records of launch b are written by hrt_records_kernel where it owns the launch, else by the launch's shade,
    fused or chain kernel: the shims hand `own` to the shade and fused kernels as records_done, and the chain kernel
    (records_done = 0 for every launch from b0 on) must never meet a launch the records kernel owns."""
    g = grid
    assert not g["own@0"].any() and not g["image@0"].any()
    for b0 in BOUNCES:
        for b in BOUNCES:   # (own is the same for every launch >= 1: any b0 <= b)
            assert not np.any((g["chains@" + b0] == 1) & (g["own@" + b] == 1)), (b0, b)
    assert not np.any((g["own_records"] == 1) & (g["chain_v"] >= 0) & (g["chains@1"] == 1))
    # the image kernel only takes primary rays where the records kernel took the shadow rays
    for b in BOUNCES:
        assert not np.any((g["image@" + b] == 1) & (g["own@" + b] == 0)), b
    # the records kernel's table is staged, one block, walked flat: the trace kernel beside it is <true, 2>
    own = g["own_records"] == 1
    assert np.all(g["in_lds"][own] == 1) and np.all(g["one_block"][own] == 1) and np.all(g["trace_v"][own] == 2)
    assert np.all(g["fine"][own] == 0)
    # a walk off LDS is never a one-block walk, the fine walk never staged
    assert not np.any((g["in_lds"] == 0) & np.isin(g["trace_v"], (2, 4)))
    assert not np.any((g["in_lds"] == 0) & np.isin(g["fused_v"], (2, 4)))
    assert not np.any((g["fine"] == 1) & (g["in_lds"] == 1))
    assert np.array_equal(g["cnt_per_wave"], g["fine"])
    # a chain is a fused later launch
    ch = g["chain_v"] >= 0
    assert np.all(g["fuses@1"][ch] == 1) and np.array_equal(g["chain_v"][ch], g["fused_v"][ch])


def test_lds_images_fit_the_cu_and_the_records_image_the_default_limit(grid):
    g = grid
    default = (g["variant"] == 7) & (g["lds_max"] == 40 * KIB) & (g["staged_max"] == 6)
    assert default.sum() == 15 * 2 ** 5 * 2 * 2
    runs = {"lds_trace": np.ones_like(default), "lds_fused": (g["fuses@0"] == 1) | (g["fuses@1"] == 1),
            "lds_chain": g["chain_v"] >= 0, "lds_records": g["own_records"] == 1, "lds_image": g["image"] == 1,
            "lds_shade": np.ones_like(default)}
    for k, can_run in runs.items():
        assert g[k][default & can_run].max() <= 160 * KIB, k
    # The records kernel is launched with at most 64 KiB (no attribute is raised for it).  The host builds patch
    # masks for tables of 65 .. 256 triangles only (problem.c: patch_build), and on those the image fits whatever
    # else holds (here 1 and 5 receivers; 256 rows leave room for 2 600); beyond them -- inputs the host never
    # forms -- the shim refuses the launch with an error.
    own = g["own_records"] == 1
    host = own & (g["T"] >= 65) & (g["T"] <= PATCH_MAX_TRI)
    assert host.any() and g["lds_records"][host].max() <= 64 * KIB
    assert g["lds_records"][host].max() == 256 * 84 + 5 * 16 + 1344
    assert np.all(g["T"][own & (g["lds_records"] > 64 * KIB)] > PATCH_MAX_TRI)
    assert 256 * 84 + 2600 * 16 + 1344 <= 64 * KIB
