"""The scatter records, entry by entry, on planted live lists.

The tracer writes scatter records in four places; whole-scene parity guards them all, but reaches only the states a
traced scene happens to produce and cannot say that an entry's record depends on the entry's own state alone.  Here
hrt_debug_last_launch (include/hrt_device.h) runs the LAST launch of a trace -- shadow traces and records, nothing else
-- on live lists planted where the record rule decides something (tests/records_util.py: a shadow hit at exactly one
metre and one float either side, theta carried through the RX order, f2 on both sides of 1, waves that mix served and
unserved lanes, lists that end inside a wave or on a chunk edge, moving meshes), and every record is compared with
oracle.scatter_records, the oracle's own RX loop, at tolerance 0.

Routes (one child process each, tests/records_child.py, because tune switches are latched per process):
  default        hrt_records_kernel, a workgroup per chunk (HRT_RECORDS_PREFETCH as built, 1: the `#else` branch of the
                 kernel is not built and therefore not covered);
  trace_grid=1   hrt_records_kernel's grid-stride loop with the next chunk's state prefetched: the shim caps the grid
                 at 2 * trace_grid = 2 workgroups (hrt_hip_launch_records; cap / 256 = 8 here), so the 1 025- and
                 1 280-entry lists take three and two chunks per workgroup;
  no_patch=1     no patch tables: hrt_trace_kernel (shadow units) + hrt_shade_kernel<.., true>.
Not covered: the fused body and the chain kernel (they cannot run a launch's records without its trace and compaction;
whole-scene parity keeps them).  Every child runs num_bounces = 1 and = 3 (record block 0 and 2).

Checked per route and case: every field of every unblocked record bit-equal to the oracle, no entry excluded; a blocked
record has a_* = tau = +0.0 and its direction and Doppler floats still hold the poison; the unblocked bit of every
(rx, i < n); slots i >= n of the record block and every byte outside record block nb - 1, mask block nb - 1, the control
words the entry clears and the tracer's scratch behind the mask blocks unchanged; the error word 0; prefix, permuted and
replaced-neighbour lists give the same bytes per entry; two runs and all routes give the same bytes; the entry's
refusals launch nothing.

Measured on an MI355X: a child (two problems, 24 launches, whole-workspace copies around each) takes 1.6 to 2.0 s, 2.1 to 2.5 s
with its start (nine children, the 24 tests of this module 20 s together)."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from . import records_util as RU
from .tune import tuned

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_TIMEOUT_S = 180
ROUTES = dict(default={}, trace_grid=dict(trace_grid=1), no_patch=dict(no_patch=1))
NBS = (1, 3)
LISTS = ["n%d" % n for n in RU.LENGTHS] + ["perm", "replaced", "n1025_again"]
AMP = ("a_te_re", "a_te_im", "a_tm_re", "a_tm_im")
PAIRS = [(r, c) for r in ROUTES for c in RU.CASES]

_failed = []    # the first GPU step that failed: nothing is started after it
_results = {}   # (route, case) -> the child's arrays
_refs = {}      # case -> list name -> (reference records, n)


def _states_of(c, name):
    if name == "replaced":
        return RU.replaced(c["states"]), RU.MASTER_N
    if name == "perm":
        return RU.take(c["states"], RU.PERM), RU.MASTER_N
    n = int(name.lstrip("n").split("_")[0])
    return RU.take(c["states"], np.arange(n)), n


def _case(case, tmp_path_factory):
    if case not in _refs:
        c = RU.case(case, tmp_path_factory.mktemp("records_" + case))
        refs = {}
        for name in LISTS:
            st, n = _states_of(c, name)
            refs[name] = (RU.reference(c, st), n)   # (computed once, shared, left unchanged)
        _refs[case] = (c, refs)
    return _refs[case]


def result(route, case, tmp_path_factory):
    if (route, case) in _results:
        return _results[(route, case)]
    if _failed:
        pytest.fail("not started: GPU step %s failed before" % _failed[0])
    c, _ = _case(case, tmp_path_factory)
    tmp = tmp_path_factory.mktemp("records_%s_%s" % (route, case))
    sc = c["scene"]
    job = dict(scene_path=sc["scene_path"], rx_pos=np.asarray(sc["rx_pos"]).tolist(), tx_pos=np.asarray(sc["tx_pos"]).tolist(),
               f_ghz=sc["f_ghz"], num_paths=sc["num_paths"], num_bounces=list(NBS), lists=LISTS, route=route,
               refusals=(case == "canyon"))
    jpath, spath, opath = (os.path.join(str(tmp), f) for f in ("job.json", "states.npz", "out.npz"))
    json.dump(job, open(jpath, "w"))
    rep = RU.replaced(c["states"])
    np.savez(spath, **c["states"], **{"rep_" + k: v for k, v in rep.items()})
    t0 = time.time()
    try:
        p = subprocess.run([sys.executable, "-m", "tests.records_child", jpath, spath, opath], cwd=REPO, capture_output=True,
                           text=True, timeout=STEP_TIMEOUT_S, env=tuned(**ROUTES[route]))
    except subprocess.TimeoutExpired:
        _failed.append("%s/%s (time limit)" % (route, case))
        raise
    if p.returncode != 0:
        _failed.append("%s/%s (exit %d)" % (route, case, p.returncode))
        pytest.fail("%s/%s: exit %d\n%s" % (route, case, p.returncode, p.stderr[-3000:]))
    R = dict(np.load(opath))
    print("records child %s/%s: %.2f s in the child, %.2f s with its start" % (route, case, float(R["child_seconds"]), time.time() - t0))
    _results[(route, case)] = R
    return R


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("route,case", PAIRS)
def test_records_equal_the_oracle(route, case, tmp_path_factory):
    c, refs = _case(case, tmp_path_factory)
    R = result(route, case, tmp_path_factory)
    tb = c["tb"]
    # the planting assumed the host's grids: the device's are the same, row by row
    assert np.array_equal(R["nuv"], tb["nuv"][R["tri_order"]]) or route == "no_patch"
    if route != "no_patch":
        assert np.float32(R["hmax"]) == tb["hmax"]
    cap = int(R["cap"])
    compared = 0
    for nb in NBS:
        for name in LISTS:
            ref, n = refs[name]
            key = "nb%d_%s_" % (nb, name)
            rec = R[key + "rec"]                      # [nrx][9][cap] bits
            nrx = rec.shape[0]
            assert int(R[key + "n"]) == n and int(R[key + "err"]) == 0, (key, int(R[key + "err"]))
            words = R[key + "mask"].view(np.uint64).reshape(nrx, cap // 64)
            ub = ((words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(nrx, cap)[:, :n]
            assert np.array_equal(ub, ref["unblocked"]), "%s: %d unblocked bits differ" % (key, (ub != ref["unblocked"]).sum())
            for f, fname in enumerate(RU.FIELDS):
                got, want = rec[:, f, :n], _bits(ref[fname])
                bad = np.argwhere((got != want) & ub)
                assert bad.size == 0, "%s %s: %d of %d unblocked records differ, first (rx, entry) %s: %08x != %08x (tag %s)" % (
                    key, fname, len(bad), ub.sum(), bad[0], got[tuple(bad[0])], want[tuple(bad[0])],
                    c["tag"][bad[0][1]] if name.startswith("n") else "-")
                if fname in AMP or fname == "tau":
                    assert (got[~ub] == 0).all(), "%s %s: a blocked record is not +0.0" % (key, fname)
                else:
                    assert (got[~ub] == RU.POISON).all(), "%s %s: a blocked record's %s was written" % (key, fname, fname)
                assert (rec[:, f, n:] == RU.POISON).all(), "%s %s: a slot at or past n = %d was written" % (key, fname, n)
            compared += int(ub.size)
            assert n < 255 or (ub.any() and (~ub).any())
            # nothing else was written: hit blocks, the other record and mask blocks, the LoS entries, counts[0 .. nb]
            assert int(R[key + "changed_outside"]) == 0 and bool(R[key + "rest_same_hash"]), key
    # no planted entry is left out of the comparison
    assert compared == len(NBS) * sum(refs[name][1] for name in LISTS) * len(c["scene"]["rx_pos"])


@pytest.mark.parametrize("route,case", PAIRS)
def test_an_entry_depends_on_its_own_state_alone(route, case, tmp_path_factory):
    R = result(route, case, tmp_path_factory)
    N = RU.MASTER_N
    for nb in NBS:
        rec = {name: R["nb%d_%s_rec" % (nb, name)] for name in LISTS}
        cap = rec["perm"].shape[2]
        bit = {name: (R["nb%d_%s_mask" % (nb, name)].view(np.uint64).reshape(-1, cap // 64)[:, :, None] >>
                      np.arange(64, dtype=np.uint64) & np.uint64(1)).reshape(-1, cap) for name in LISTS}
        full = rec["n1025"]
        for n in RU.LENGTHS:   # a shorter list's records are a prefix of a longer one's
            assert np.array_equal(rec["n%d" % n][:, :, :n], full[:, :, :n]), "nb %d: list of %d is no prefix" % (nb, n)
            assert np.array_equal(bit["n%d" % n][:, :n], bit["n1025"][:, :n])
        # the permuted master list against the replaced one's even slots and the prefix: the same entry, the same bytes
        inv = np.argsort(RU.PERM)
        back = rec["perm"][:, :, inv]                      # entry i of the master list
        assert np.array_equal(back[:, :, :1025], full[:, :, :1025]), "nb %d: a permuted entry's record differs" % nb
        assert np.array_equal(bit["perm"][:, inv][:, :1025], bit["n1025"][:, :1025])
        even = np.arange(0, N, 2)
        assert np.array_equal(rec["replaced"][:, :, even], back[:, :, even]), "nb %d: a record changed with its neighbours" % nb
        assert np.array_equal(bit["replaced"][:, even], bit["perm"][:, inv][:, even])
        # two runs of one list
        assert np.array_equal(rec["n1025_again"], rec["n1025"]) and np.array_equal(bit["n1025_again"], bit["n1025"])
    # record block 0 and record block 2 hold the same bytes
    for name in LISTS:
        n = int(R["nb1_%s_n" % name])
        assert np.array_equal(R["nb1_%s_rec" % name][:, :, :n], R["nb3_%s_rec" % name][:, :, :n])


@pytest.mark.parametrize("case", RU.CASES)
def test_routes_agree(case, tmp_path_factory):
    base = result("default", case, tmp_path_factory)
    for route in ROUTES:
        R = result(route, case, tmp_path_factory)
        for nb in NBS:
            for name in LISTS:
                n = int(base["nb%d_%s_n" % (nb, name)])
                k = "nb%d_%s_rec" % (nb, name)
                assert np.array_equal(R[k], base[k]), "%s nb %d %s: the record block differs from the default route's" % (route, nb, name)
                k = "nb%d_%s_mask" % (nb, name)
                nw = (n + 63) // 64 * 2
                cap = int(base["cap"])
                a, b = R[k].reshape(-1, cap // 32)[:, :nw], base[k].reshape(-1, cap // 32)[:, :nw]
                last = np.uint64((1 << (n % 64)) - 1) if n % 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
                a, b = a.copy().view(np.uint64), b.copy().view(np.uint64)
                a[:, -1] &= last; b[:, -1] &= last
                assert np.array_equal(a, b), "%s nb %d %s: unblocked bits differ from the default route's" % (route, nb, name)


@pytest.mark.parametrize("route", list(ROUTES))
def test_refusals_launch_nothing(route, tmp_path_factory):
    R = result(route, "canyon", tmp_path_factory)
    assert sorted(R["refused"].tolist()) == sorted(["counts_beyond_cap", "short_workspace", "nb_0", "null_workspace"])
