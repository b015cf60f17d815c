"""One case of tests/test_gpu_trace_patch.py in a process of its own: `python -m tests.trace_patch_child <case> <tmp dir>`
asks the launch plan (built for the host) which launches take hrt_trace_kernel's patch-table instantiation and with which
image, runs the product and the oracle on the case and compares every output array and the live-list lengths bit for
bit; prints TRACE_PATCH_OK on success."""
import ctypes as C
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
os.environ.setdefault("HRT_TUNE", "rxt_min_rays=0")   # patch tables at every size (default: big launch sets only)

from oracle import oracle  # noqa: E402
from tests import configs as K  # noqa: E402
from tests.launch0_patch_child import problem_tables  # noqa: E402
from tests.parity import compare_dense  # noqa: E402
from tests.test_gpu_launch0_patch import TIE_TRI  # noqa: E402
from tests.test_gpu_trace_patch import SCENES, case_config  # noqa: E402

_SRC = r"""
#include "hrt_launch_plan.h"
/* bit b of the answer: launch b takes the patch-table instantiation; -1: the plan has no such image */
long long plan_patch(unsigned T, unsigned num_rx, unsigned num_tx, unsigned num_bounces, long long *lds)
{
    static const unsigned long long masks = 0u;
    hrt_kparams K;
    long long bits = 0;
    memset(&K, 0, sizeof K);
    K.tune.variant = HRT_TRACE_VARIANT_DEFAULT;
    K.tune.lds_tri_bytes_max = 40u * 1024u;
    K.tune.fuse_staged_max_tri = 6u;
    K.num_tri = T; K.num_tx = num_tx; K.num_rx = num_rx; K.num_bounces = num_bounces;
    K.patch.mask = &masks; K.patch.txcell = &masks; K.patch.num_img = num_tx;
    const hrt_launch_plan p = hrt_plan(&K);
    *lds = (long long)p.lds_trace_patch;
    if (!p.trace_patch) return -1;
    for (unsigned b = 0; b <= num_bounces; ++b)
        if (hrt_plan_trace_patch(&p, b) && !hrt_plan_image(&p, b)) bits |= 1ll << b;
    return bits;
}
"""


def plan_patch(tmp, n_tri, c):
    src, so = os.path.join(tmp, "plan_patch.c"), os.path.join(tmp, "libplan_patch.so")
    with open(src, "w") as f:
        f.write(_SRC)
    subprocess.check_call(["cc", "-std=c99", "-O2", "-shared", "-fPIC", "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"),
                           src, "-o", so, "-lm"])
    h = C.CDLL(so)
    h.plan_patch.restype = C.c_longlong
    lds = C.c_longlong(0)
    bits = int(h.plan_patch(C.c_uint(n_tri), C.c_uint(len(c["rx_pos"])), C.c_uint(len(c["tx_pos"])),
                            C.c_uint(c["num_bounces"]), C.byref(lds)))
    return bits, int(lds.value)


def main():
    name, tmp = sys.argv[1], sys.argv[2]
    c, env = case_config(name, tmp)
    assert all(os.environ.get(k) == v for k, v in env.items()), env
    # without this switch the run below builds no tables at these ray counts and every launch takes the shared kernels
    assert "rxt_min_rays=0" in os.environ["HRT_TUNE"].split(","), os.environ["HRT_TUNE"]
    n_tri = SCENES.get(name.split("-")[0], TIE_TRI)
    nb = c["num_bounces"]
    # the problem itself: patch masks built (kind 1) -- what sends launches >= 1 to the records kernel and with it the
    # primary rays of launches >= 2 to the instantiation under test
    T, kinds = problem_tables(c)
    assert T == n_tri and (kinds & 1), (name, T, kinds)
    bits, lds = plan_patch(tmp, T, c)
    assert bits == sum(1 << b for b in range(2, nb + 1)), (name, bits)   # never launch 0 or 1, fused launches or not
    # rows, mask words and counters: an eighth of a CU holds them up to 249 rows (gen256: a seventh)
    assert lds == 80 * T + 512 + 16, (name, lds)
    assert (lds <= 163840 // 8) == (T <= 249) and lds <= 163840 // 7, (name, lds)
    ref = oracle.compute_paths(*K.args(c))
    live = [int(x) for x in ref["extras"]["live"]]
    assert all(live[b] > 0 for b in range(2, nb)), live   # the launches under test had entries to walk
    from hermespy_rt_amd import abi, lib
    L = lib.load()
    st = lib.Stats()
    got = abi.run_compute_paths(L, *K.args(c), stats=st)   # (an error word that is not clean fails the call)
    assert int(L.hrt_fallback_state()) == 0, "a kernel was switched off: not the launches under test were compared"
    got_live = [int(st.live[b]) for b in range(nb + 1)]
    assert got_live == live, (got_live, live)
    cmp = compare_dense(got, ref)
    print(name, "patch launches", bits, "lds", lds, "live", live, cmp, flush=True)
    assert all(v == 0 for v in cmp.values()), cmp
    print("TRACE_PATCH_OK", name)


if __name__ == "__main__":
    main()
