"""Several tracer processes on ONE GPU at the same time -- how a drop-in library is used (worker processes,
or next to torch).  The fused kernels' workgroups wait for the chunks in front of them; with chunks numbered
by dispatch (blockIdx) four such processes locked each other out for whole time slices (C4: 5.8 s per step
instead of 0.2 ms, profiles/HISTORY.md r4); now they share the GPU like any other kernels.  Default settings (HRT_FUSE unset)."""
# (what makes it safe: a fused launch gives up waiting after ~10 ms, declares the step void and the library goes
# on with two kernels per launch -- hrt_kernels.hip lb_exclusive, problem.c fuse_mode; tickets drawn at workgroup
# start were measured too: exact, but 10 % of C4's step)
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("workload,rays,procs", [("c4", 1000000, 4), ("c3", 500000, 2)])
def test_processes_sharing_one_gpu_stay_work_conserving(workload, rays, procs):
    sys.path.insert(0, os.path.join(REPO, "profiles", "tools"))
    import shared_gpu
    solo = shared_gpu.run(workload, rays, 1, 50)[0]
    both = shared_gpu.run(workload, rays, procs, 50)
    # sharing costs each process at most its share of the GPU (x procs), with a factor 2 of slack
    assert max(both) <= 2.0 * procs * solo + 1.0, (solo, both)


# One child process per drop-in entry: the fallback is global to a process (after the first void step every later
# call runs unfused and never retries), and the three entries share the retry (csrc/host/batch.c).
_FALLBACK_PRELUDE = r"""
import sys
sys.path.insert(0, %r)
import numpy as np
from hermespy_rt_amd import abi, lib
from oracle import oracle
from tests import configs as K
L = lib.load()
"""
_FALLBACK_CHILD = dict(
    dense=r"""
from tests.parity import compare_dense
for c in (K.small(K.C4_DOPPLER, 300000), K.small(K.C3, 200000), K.small(K.C4_DOPPLER, 300000)):
    st = compare_dense(abi.run_compute_paths(L, *K.args(c)), oracle.compute_paths(*K.args(c)))
    assert all(v == 0 for v in st.values()), st
""",
    # every record carries the oracle's dense bits at its slot (as tests/test_gpu_path_list_c.py)
    list=r"""
c = K.small(K.C4_DOPPLER, 300000)
sc = oracle.compute_paths(*K.args(c))["scat"]
unblocked = abi.written(sc["directions_rx"][..., 0])
P = abi.run_compute_paths_list(L, *K.args(c))
assert P["rx"].size == int(unblocked.sum()), (P["rx"].size, int(unblocked.sum()))
idx = tuple(P[k].astype(np.int64) for k in ("rx", "tx", "bounce", "path"))
assert unblocked[idx].all()
for k in ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im", "tau"):
    assert np.array_equal(P[k].view(np.uint32), sc[k][idx].view(np.uint32)), k
""",
    # one TX: the scatter part against the float64 sum of the oracle's unblocked records (as
    # tests/test_gpu_channel.py::test_scatter_matches_dense_oracle)
    channel=r"""
from tests.test_gpu_channel import DF, _check, _grid, _phase_sum
c = K.small(K.C4_DOPPLER, 300000)
c["tx_pos"], c["tx_vel"] = c["tx_pos"][:1], c["tx_vel"][:1]
sc = oracle.compute_paths(*K.args(c))["scat"]
ub = abi.written(sc["directions_rx"][..., 0])
nk = 64
f0 = _grid(c, nk)
got = abi.run_compute_channel(L, *K.args(c), abi.channel_spec(f0, DF, nk, los=False))
f, t = f0 + np.arange(nk) * DF, np.zeros(1)
H = np.zeros(got.shape, np.complex128)
S = np.zeros(got.shape[:3])
for rx in range(got.shape[0]):
    s = ub[rx, 0]
    a_te = sc["a_te_re"][rx, 0][s] + 1j * sc["a_te_im"][rx, 0][s].astype(np.float64)
    a_tm = sc["a_tm_re"][rx, 0][s] + 1j * sc["a_tm_im"][rx, 0][s].astype(np.float64)
    _phase_sum(H, S, rx, 0, a_te, a_tm, sc["tau"][rx, 0][s], sc["freq_shift"][rx, 0][s], f, t)
_check(got, H, S)
""")


@pytest.mark.parametrize("entry", sorted(_FALLBACK_CHILD))
def test_a_fused_launch_that_gives_up_is_redone_unfused(entry):
    """The fallback itself, deterministically: with lb_max_polls=0 every chunk that has to wait at all declares
    the step void at once.  The drop-in call must notice (HRT_ERR_FUSE_TIMEOUT in the counts it reads), run the
    step again as two kernels per launch, keep fusion off -- and return the oracle's bits (the channel: its
    float64 sum).  The fallback state after the call shows that the retry ran."""
    import subprocess
    code = (_FALLBACK_PRELUDE % REPO + _FALLBACK_CHILD[entry] +
            'print("FALLBACK_OK", int(L.hrt_fallback_state()))\n')
    from tests.tune import tuned
    p = subprocess.run([sys.executable, "-c", code], env=tuned(lb_max_polls=0), capture_output=True, text=True)
    assert p.returncode == 0 and "FALLBACK_OK" in p.stdout, p.stdout[-1500:] + p.stderr[-3000:]
    state = int(p.stdout.split("FALLBACK_OK")[1].split()[0])
    assert state != 0, "no void step: the retry was not exercised"
