"""One case of tests/test_gpu_launch0_patch.py in a process of its own: `python -m tests.launch0_patch_child <case> <tmp
dir>` asks the launch plan (built for the host) which image launch 0 gets, runs the product and the oracle on the case and
compares every output array and the live-list lengths bit for bit; prints LAUNCH0_OK on success."""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import oracle  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.parity import compare_dense  # noqa: E402
from tests.test_gpu_launch0_patch import SCENES, TIE_TRI, case_config  # noqa: E402

_SRC = r"""
#include "hrt_launch_plan.h"
int plan_words(unsigned T, unsigned num_tx, long long *lds)
{
    static const unsigned long long masks = 0u;
    hrt_kparams K;
    memset(&K, 0, sizeof K);
    K.tune.variant = HRT_TRACE_VARIANT_DEFAULT;
    K.tune.lds_tri_bytes_max = 40u * 1024u;
    K.tune.fuse_staged_max_tri = 6u;
    K.num_tri = T; K.num_tx = num_tx; K.num_rx = 1u;
    K.patch.mask = &masks; K.patch.txcell = &masks;
    const hrt_launch_plan p = hrt_plan(&K);
    *lds = (long long)p.lds_fused0;
    return p.fused0_txcell ? (int)p.fused0_words : -1;
}
"""


def plan_words(tmp, n_tri, num_tx):
    src, so = os.path.join(tmp, "plan_words.c"), os.path.join(tmp, "libplan_words.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["cc", "-std=c99", "-O2", "-shared", "-fPIC", "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"),
                           src, "-o", so, "-lm"])
    lds = C.c_longlong(0)
    return int(C.CDLL(so).plan_words(C.c_uint(n_tri), C.c_uint(num_tx), C.byref(lds))), int(lds.value)


def problem_tables(c):
    """(triangles, table kinds) of the problem the library builds for the case's scene and endpoints
    (hrt_debug_table_info: 1 patch masks, 2 image apexes, 4 the TX cell table, 8 per-cell masks)"""
    import numpy as np
    from hermespy_rt_amd import abi, lib
    L = lib.load()
    rx = np.ascontiguousarray(np.asarray(c["rx_pos"], np.float32).reshape(-1, 3))
    tx = np.ascontiguousarray(np.asarray(c["tx_pos"], np.float32).reshape(-1, 3))
    zr, zt = np.zeros_like(rx), np.zeros_like(tx)
    V3 = C.POINTER(abi.Vec3)
    scene = L.scene_load(str(c["scene_path"]).encode())
    try:
        h = C.c_void_p()
        lib.check(L.hrt_problem_create(C.byref(scene), rx.ctypes.data_as(V3), tx.ctypes.data_as(V3), zr.ctypes.data_as(V3),
                                       zt.ctypes.data_as(V3), C.c_float(c["f_ghz"]), rx.shape[0], tx.shape[0], 0, C.byref(h)),
                  "hrt_problem_create")
    finally:
        abi.free_scene(scene)
    try:
        return int(L.hrt_problem_num_triangles(h)), int(abi.debug_table_info(L, h)["kinds"])
    finally:
        L.hrt_problem_destroy(h)


def main():
    name, tmp = sys.argv[1], sys.argv[2]
    c = case_config(name, tmp)
    n_tri, words_in = SCENES.get(name.split("-")[0], (TIE_TRI, True))
    # the problem itself: patch masks and the TX cell table built, no per-cell masks -- what sends launch 0 to the
    # instantiation under test (without them the shared one would be what is compared)
    T, kinds = problem_tables(c)
    assert T == n_tri and (kinds & 1) and (kinds & 4) and not (kinds & 8), (name, T, kinds)
    words, lds0 = plan_words(tmp, T, len(c["tx_pos"]))
    assert words == (1 if words_in else 0) and 0 < lds0 <= 163840 // 7, (name, words, lds0)
    ref = oracle.compute_paths(*K.args(c))
    live = [int(x) for x in ref["extras"]["live"]]
    from hermespy_rt_amd import abi, lib
    L = lib.load()
    st = lib.Stats()
    got = abi.run_compute_paths(L, *K.args(c), stats=st)   # (an error word that is not clean fails the call)
    assert int(L.hrt_fallback_state()) == 0, "a fused launch was switched off: the per-launch kernels were compared"
    got_live = [int(st.live[b]) for b in range(c["num_bounces"] + 1)]
    assert got_live == live, (got_live, live)
    cmp = compare_dense(got, ref)
    print(name, "words", words, "lds", lds0, "live", live, cmp, flush=True)
    assert all(v == 0 for v in cmp.values()), cmp
    print("LAUNCH0_OK", name)


if __name__ == "__main__":
    main()
