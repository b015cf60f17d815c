"""The dominant-path selection (csrc/hrt_dominant.hip) at its flush, merge and K edges: workspaces of an empty closed
room planted with exact, distinct powers in a chosen order of the selection's walk (tests/dominant_order_util.py),
every list compared with dominant.reference on bytes; there is no tolerance anywhere.  Which edge a combination is
there for, and that it reaches it, is tests/test_dominant_order_design.py (CPU); here every combination first proves
its chunk plan on the device's own scratch size.  DESIGN.md section 15."""
import ctypes as C

import numpy as np
import pytest

from hermespy_rt_amd import abi, dominant

from . import dominant_order_util as DU
from . import planted as PL
from .dominant_util import check_bytes, to_numpy
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def bench(tmp_path_factory):
    """case -> its tracer, traced once, with what the selection sees of the trace (one tracer alive at a time)"""
    state = {}

    def get(case):
        if case not in state:
            for s in state.values():
                s["tr"].close()
            state.clear()
            tr = _tracer(DU.config(case, tmp_path_factory))
            tr.trace()
            tr.torch.cuda.synchronize(tr.device)
            counts = tr.counts()
            # The closed room keeps every ray but the few that meet one of its edges exactly (3 of 262 144 in the
            # second block of `cap_1024`), so the cases are sized from the TX segments of the hit blocks (DU.describe),
            # not from the ray count: the chunk plan is asserted per call, the exact fills from the model on these
            # very segments (DU.EXACT_FILL)
            for b in range(tr.nb):
                assert 0 <= tr.ntx * tr.num_local - int(counts[b + 1]) <= DU.LOST_MAX, (case, b, counts)
            state[case] = dict(tr=tr, W=DU.describe(tr), planted=None, T=None)
        return state[case]

    yield get
    for s in state.values():
        s["tr"].close()


def _plant(s, order, live):
    if s["planted"] != (order, live):
        s["T"] = DU.plant_order(s["tr"], order, live, s["W"])
        s["planted"] = (order, live)
    return s["T"]


def _plant_records(s, amps, live):
    s["planted"] = None
    return DU.plant_records(s["tr"], s["W"], amps, live)


def _assert_plan(tr, case, K):
    """the device's scratch size is the mirrored plan's: the call has the chunks and merge lists the case is named for"""
    spec = abi.dominant_spec(K)
    need = C.c_uint64(0)
    assert tr.L.hrt_dominant_paths_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(need)) == 0
    p = DU.plan(tr, K)
    assert int(need.value) == p["bytes"], (case, K, int(need.value), p)
    assert (p["nchunks"], p["nmid"]) == (DU.CASES[case]["nchunks"], DU.CASES[case]["nmid"]), (case, K, p)


# ------------------------------------------------------------------ 1. orders, live patterns, K
@pytest.mark.parametrize("case,order,live,K", DU.SURVIVORS, ids=["%s-%s-%s-%d" % s for s in DU.SURVIVORS])
def test_planted_order(bench, case, order, live, K):
    s = bench(case)
    tr = s["tr"]
    _assert_plan(tr, case, K)
    T = _plant(s, order, live)
    got = to_numpy(tr.dominant_paths(K))
    want = DU.reference(T, tr.nrx, tr.ntx, K)
    check_bytes(got, want, (case, order, live, K))
    if (case, order, live, K) in DU.EXACT_FILL:   # on the segments of this trace, the edge is reached
        modelled, st = DU.run_model(s["W"], T, K)
        assert DU.same_bytes(modelled, want)
        for kernel in DU.EXACT_FILL[(case, order, live, K)]:
            assert st[kernel]["exact"] >= 1 and st[kernel]["max_pending"] == DU.N - K, (case, kernel, st[kernel])


# ------------------------------------------------------------------ 2. equal and extreme powers
@pytest.mark.parametrize("K", [512, 1024])
def test_equal_powers(bench, K):
    """every record of `fanin_full` with power 25: the low half of the key, (bounce, path), decides everything"""
    s = bench("fanin_full")
    tr = s["tr"]
    _assert_plan(tr, "fanin_full", K)
    T = _plant_records(s, DU.equal_amplitudes(s["W"]), DU.live_bits(s["W"], "all"))
    got = to_numpy(tr.dominant_paths(K))
    check_bytes(got, DU.reference(T, 1, 1, K), ("equal powers", K))
    assert (got["power"] == 25).all() and (got["bounce"] == 0).all() and (np.diff(got["path"][0, 0].astype(np.int64)) > 0).all()


def test_extreme_powers(bench):
    """finite extremes in one link: powers of exactly 0 from +-0.0 components, a denormal component, 3e38 in all
    four, equal powers from different components; kept = eligible < K"""
    s = bench("one_chunk")
    tr = s["tr"]
    K = DU.EXTREME_K
    _assert_plan(tr, "one_chunk", K)
    T = _plant_records(s, *DU.extreme_records(s["W"]))
    got = to_numpy(tr.dominant_paths(K))
    check_bytes(got, DU.reference(T, 1, 1, K), "extreme powers")
    n = len(DU.EXTREMES) + int(T["los"].sum())
    assert int(got["kept"][0, 0]) == int(got["eligible"][0, 0]) == n < K
    p = got["power"][0, 0, :n]
    assert np.isfinite(p).all() and (p[-3:] == 0).all() and (p[:-3] > 0).all()   # the zero powers kept, and last
    assert p[0] == p[1] == 4 * float(np.float32(3e38)) ** 2 and tuple(got["bounce"][0, 0, :2]) == (0, 1)
    ties = np.nonzero(p == 25)[0]
    key = [(int(got["bounce"][0, 0, q]), int(got["path"][0, 0, q])) for q in ties]
    assert len(ties) == 4 and key == sorted(key)
    assert np.signbit(got["a_te"][0, 0, n - 3:n].real).any()


# ------------------------------------------------------------------ 3. accumulate against a chosen `out`
@pytest.mark.parametrize("case,order", [("fanin_full", "asc"), ("merge_tail_one", "shuffled")])
@pytest.mark.parametrize("K", [3, 512, 1024])
def test_accumulate_into_a_chosen_list(bench, case, order, K):
    s = bench(case)
    tr = s["tr"]
    torch = tr.torch
    _assert_plan(tr, case, K)
    T = _plant(s, order, "all")
    new = DU.reference(T, 1, 1, K)
    check_bytes(to_numpy(tr.dominant_paths(K)), new, (case, K, "alone"))
    for kind in DU.OLD_KINDS:
        old = DU.old_list(T, K, kind, 1, 1)
        want = dominant.merge(old, new)
        assert int(want["eligible"][0, 0]) == int(old["eligible"][0, 0]) + int(new["eligible"][0, 0])
        out = torch.from_numpy(old["buffer"].copy()).to(tr.device)
        got = to_numpy(tr.dominant_paths(K, out=out, accumulate=True))
        check_bytes(got, want, (case, K, kind))
        if kind == "stronger":
            assert np.array_equal(got["buffer"][16:], old["buffer"][16:])
        if kind in ("even", "half"):   # every old record changes slot: none may be stored before all are read
            kept_old = int(old["kept"][0, 0])
            assert (DU.old_slots(want, old)[0, 0, :kept_old] != np.arange(kept_old)).all()


# ------------------------------------------------------------------ 4. poison and repetition
@pytest.mark.parametrize("case,order,live", [("fanin_full", "asc", "odd"), ("two_by_two", "shuffled", "runs")])
def test_poison_and_repetition(bench, case, order, live):
    s = bench(case)
    tr = s["tr"]
    T = _plant(s, order, live)
    clean = {}
    for K in (3, 1024):
        clean[K] = to_numpy(tr.dominant_paths(K))["buffer"].copy()
        assert np.array_equal(clean[K], DU.reference(T, tr.nrx, tr.ntx, K)["buffer"]), (case, K)
        assert np.array_equal(to_numpy(tr.dominant_paths(K))["buffer"], clean[K]), (case, K, "second call")
    s["planted"] = None
    hit = PL.poison(tr, s["W"]["counts"], np.float32(3e38))
    assert hit["blocked_records"] > 0 and hit["blocked_records"] + hit["tail_slots"] > tr.nrx * tr.num_local // 4
    for K, want in clean.items():
        assert np.array_equal(to_numpy(tr.dominant_paths(K))["buffer"], want), (case, K, "poison read")
