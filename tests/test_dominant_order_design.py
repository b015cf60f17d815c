"""The design of tests/test_gpu_dominant_order.py, checked without a device on made-up workspaces of the cases' sizes
(DU.synthetic: what the empty closed room gives, every ray a record in both blocks):

 1. DU.model, the slot mechanics of csrc/hrt_dominant.hip step by step, gives dominant.reference's bytes for every
    case x order x live pattern x K, so its counters mean something;
 2. every edge the GPU file is there for is reached, asserted from those counters, and DU.SURVIVORS is the list the
    counters leave;
 3. every misreading of the kernel in DU.WRONG changes the bytes of a named combination the GPU file runs, or is shown
    to be harmless to the bytes (and then what it does change)."""
import numpy as np
import pytest

from hermespy_rt_amd import dominant

from . import dominant_order_util as DU

N = DU.N
_SWEEPS = {}


def _sweep(case):
    """(W, the surviving combinations, {(order, live, K): (features, counters)}) of a case; every result of the
    model compared with the reference on the way"""
    if case not in _SWEEPS:
        W = DU.synthetic(case)
        assert DU.full_blocks(W)

        def check(order, live, K, T, got):
            want = DU.reference(T, W["nrx"], W["ntx"], K)
            assert DU.same_bytes(got, want), (case, order, live, K)
            if K == DU.CASES[case]["ks"][-1]:   # (DU.reference is dominant.reference but for the triangles)
                want["tri"][want["bounce"] >= 0] = 0
                assert DU.same_bytes(want, dominant.reference(T, W["nrx"], W["ntx"], K))

        keep, feats = DU.derive(case, W, check)
        _SWEEPS[case] = (W, keep, feats)
    return _SWEEPS[case]


def _counters(case, order, live, K):
    return _sweep(case)[2][(order, live, K)][1]


# ------------------------------------------------------------------ 0. the plan and the slot rules on one chunk
@pytest.mark.parametrize("case", sorted(DU.CASES))
def test_plan(case):
    c = DU.CASES[case]
    for K in DU.KS_ALL:
        p = DU.plan_of(c["rays"], DU.NB, c["nrx"], c["ntx"], K)
        assert (p["nchunks"], p["nmid"]) == (c["nchunks"], c["nmid"]), (case, K, p)
    n = c["rays"]
    starts = DU.chunk_starts(n, c["nchunks"])
    size = np.diff(starts)
    if case == "fanin_full":
        assert starts[1] == 512 and starts[2] == 1025 and (starts[1:-1] % 64 != 0).any()   # 512.5 c
    if case == "cap_1024":
        assert (size == 1024).all()
    if case == "cap_1536":
        assert (size == 1536).all()
    if case in ("merge_tail_one", "two_by_two"):
        assert c["nchunks"] % DU.FANIN == 1 and (starts[1:-1] % 64 != 0).any()


@pytest.mark.parametrize("K,used,exact", [(512, 2048, 2), (1024, 2048, 4), (511, 2047, 0), (513, 1537, 0),
                                          (1023, 2047, 0)])
def test_one_ascending_chunk_of_4096(K, used, exact):
    """an all-live chunk of 4 096 records of one block, powers ascending: the largest number of used slots and the
    steps that end with all 2 048 in use"""
    v = np.arange(1, 4097)
    hi, lo = DU.keys_of(v.astype(np.float64) ** 2, np.zeros(4096, int), v)
    chunk = [dict(n=4096, off=np.arange(4096), hi=hi, lo=lo, id=np.arange(4096))]
    cols = {k: np.zeros((4096,) + ((3,) if k.startswith("u_") else ())) for k in dominant.FIELDS}
    out, st = DU.model([dict(chunks=[chunk], los=None)], K, 1, 1, cols)
    assert K + st["partial"]["max_pending"] == used and st["partial"]["exact"] == exact
    assert int(out["kept"][0, 0]) == K and int(out["eligible"][0, 0]) == 4096


# ------------------------------------------------------------------ 1. + 2. the model, the edges, the survivors
@pytest.mark.parametrize("case", list(DU.CASES))
def test_model_is_the_reference_and_survivors(case):
    W, keep, feats = _sweep(case)
    assert len(feats) == len(DU.combos(case)) * len(DU.CASES[case]["ks"])
    assert tuple(keep) == tuple(s for s in DU.SURVIVORS if s[0] == case)
    assert set(DU.NAMED) <= set(DU.SURVIVORS)


def test_named_edges_are_reached():
    # the pending slots filled exactly to N - K, kernel by kernel
    for case, K in (("cap_1024", 1024), ("cap_1536", 512)):
        st = _counters(case, "asc", "all", K)["partial"]
        assert st["exact"] >= 1 and st["max_pending"] == N - K, (case, K, st)
    st = _counters("merge_two_full", "asc", "all", 1024)["merge"]
    assert st["exact"] >= 1 and st["max_pending"] == N - 1024
    for case in ("fanin_full", "cap_1024"):
        st = _counters(case, "asc", "all", 1024)["final"]
        assert st["exact"] >= 1 and st["max_pending"] == N - 1024
    for combo, kernels in DU.EXACT_FILL.items():   # (the same, as the GPU file asserts it on its own segments)
        assert combo in DU.SURVIVORS and all(_counters(*combo)[k]["exact"] >= 1 for k in kernels), combo
    # one below: the slot behind the last is never needed (K odd leaves one slot over, or fills with the LoS entry)
    assert _counters("cap_1024", "asc", "all", 1023)["partial"]["max_pending"] == 1024 < N - 1023
    assert _counters("cap_1024", "asc", "all", 1023)["final"]["max_pending"] == N - 1023   # 1 LoS + 1 024
    # the merge tree
    assert _counters("one_chunk", "asc", "all", 1024)["merge"]["flushes"] == 0
    assert _counters("fanin_full", "asc", "all", 1024)["merge"]["flushes"] == 0
    for case, groups, single in (("merge_tail_one", 2, 1), ("merge_two_full", 2, 0), ("cap_1024", 16, 0),
                                 ("two_by_two", 8, 4)):
        st = _counters(case, "asc", "all", 1024)
        assert len(st["merge"]["kept_flushes"]) == groups and st["single"] == single, (case, st)
    # ascending: every flush of every workgroup keeps something; descending: one per chunk does
    for case in DU.BIG:
        for K in DU.KS_BIG:
            asc, desc = (_counters(case, o, "all", K)["partial"] for o in ("asc", "desc"))
            assert set(desc["kept_flushes"]) == {1} and desc["flushes"] > len(desc["kept_flushes"])
            assert asc["flushes"] == sum(asc["kept_flushes"]) > desc["flushes"] / 2
    # a chunk starts inside a mask word of mixed bits
    for case in ("fanin_full", "merge_tail_one", "two_by_two"):
        for live in ("odd", "runs"):
            assert ("split_word", True) in _sweep(case)[2][("asc", live, 1024)][0], (case, live)


# ------------------------------------------------------------------ 3. the wrong readings
def _run(case, order, live, K, wrong, **kw):
    W = _sweep(case)[0]
    T = DU.order_terms(W, order, live)
    got, st = DU.run_model(W, T, K, wrong=wrong, **kw)
    return got, st, DU.reference(T, W["nrx"], W["ntx"], K), _counters(case, order, live, K)


# the reading -> the surviving combination whose bytes it changes
CHANGES = {
    "room_late": ("fanin_full", "asc", "all", 1024),        # the 513th record of a block, a chunk's largest, is lost
    "merge_unclamped": ("two_by_two", "desc", "all", 1024),   # the next link's first lists hold ITS largest
    "merge_skips_last": ("merge_two_full", "asc", "all", 1024),   # the winners are all in the last list
    "final_reads_la": ("merge_tail_one", "asc", "all", 1024),
    "count_not_summed": ("merge_tail_one", "asc", "all", 3),      # `eligible` alone
}


@pytest.mark.parametrize("wrong", sorted(CHANGES))
def test_wrong_reading_changes_bytes(wrong):
    combo = CHANGES[wrong]
    assert combo in DU.SURVIVORS
    kw = dict(other=[1, 2, 3, 0]) if wrong == "merge_unclamped" else {}
    got, st, want, _ = _run(*combo, wrong, **kw)
    assert not DU.same_bytes(got, want)
    if wrong == "count_not_summed":
        assert np.array_equal(got["buffer"][16:], want["buffer"][16:]) and got["eligible"][0, 0] < want["eligible"][0, 0]


def test_room_ge_is_benign():
    """flushing when the step would fill the pending slots exactly sorts more often and keeps the same list"""
    for combo in (("cap_1024", "asc", "all", 1024), ("cap_1536", "asc", "all", 512)):
        got, st, want, right = _run(*combo, "room_ge")
        assert DU.same_bytes(got, want)
        assert st["partial"]["flushes"] > right["partial"]["flushes"] and st["partial"]["exact"] == 0


def _equal(wrong=None, K=1024):
    W = DU.synthetic("fanin_full")
    T = DU.terms(W, DU.equal_amplitudes(W), DU.live_bits(W, "all"))
    got, st = DU.run_model(W, T, K, wrong=wrong)
    return got, st, DU.reference(T, 1, 1, K)


def test_threshold_and_sort_on_equal_powers():
    """With distinct powers the low half of the key decides nothing, so these three readings show on equal powers
    (the GPU file's test_equal_powers): every record of `fanin_full` with power 25, the order (bounce, path) alone."""
    for K in (512, 1024):
        got, right, want = _equal(K=K)
        assert DU.same_bytes(got, want)
        # thr_ge, a candidate that only ties with the threshold on `hi` is pushed: sorted away again.  Harmless to the
        # bytes (dm_room leaves room for a whole step whatever is pushed): only more candidates wait and are sorted
        got, st, _ = _equal("thr_ge", K)
        assert DU.same_bytes(got, want) and st["final"]["pushed"] > right["final"]["pushed"]
        # ... while one that is pushed only when `hi` is larger loses every record behind the first flush, and a sort
        # on `hi` alone keeps whichever of the equal ones the network leaves in front
        for wrong in ("thr_gt_hi", "hi_only_sort"):
            assert not DU.same_bytes(_equal(wrong, K)[0], want), (wrong, K)


@pytest.mark.parametrize("case,order", [("fanin_full", "asc"), ("merge_tail_one", "shuffled")])
@pytest.mark.parametrize("K", [3, 512, 1024])
def test_accumulate_design(case, order, K):
    W = _sweep(case)[0]
    T = DU.order_terms(W, order, "all")
    tbc, cols = DU.chunk_terms(W, T), DU.cols_of(T)
    new = DU.reference(T, 1, 1, K)
    for kind in DU.OLD_KINDS:
        old = DU.old_list(T, K, kind, 1, 1)
        want = dominant.merge(old, new)
        got, st = DU.model(tbc, K, 1, 1, cols, old=old)
        assert DU.same_bytes(got, want), (case, K, kind)
        assert int(want["eligible"][0, 0]) == int(old["eligible"][0, 0]) + int(new["eligible"][0, 0])
        slots = DU.old_slots(want, old)[0, 0]
        kept_old = int(old["kept"][0, 0])
        if kind == "stronger":
            assert np.array_equal(slots, np.arange(K)) and np.array_equal(want["buffer"][16:], old["buffer"][16:])
            assert st["final"]["exact"] >= (K == 1024)   # K old records fill the pending slots of K = 1 024 exactly
        if kind == "weaker":
            assert (slots == -1).all() and DU.same_bytes(want, _with_eligible(new, want))
        if kind in ("even", "half"):
            assert kept_old == (K if kind == "even" else max(K // 2, 1))
            moved = slots[:kept_old]
            assert (moved != np.arange(kept_old)).all()                # every old record changes slot or leaves
            assert np.array_equal(moved[moved >= 0], 2 * np.nonzero(moved >= 0)[0] + 1)
        # kept_old is clamped for a header no call writes: on these it changes nothing
        assert DU.same_bytes(DU.model(tbc, K, 1, 1, cols, old=old, wrong="kept_unclamped")[0], want)
        # storing a winner before all old slots are read shows where old records move up the list
        wrong = DU.model(tbc, K, 1, 1, cols, old=old, wrong="old_in_place")[0]
        assert DU.same_bytes(wrong, want) == (kind in ("stronger", "weaker")), (case, K, kind)


def _with_eligible(res, like):
    out = dominant.empty(*res["power"].shape)
    out["buffer"][:] = res["buffer"]
    out["eligible"][...] = like["eligible"]
    return out


def test_extreme_records_design():
    W = DU.synthetic("one_chunk")
    amps, live = DU.extreme_records(W)
    T = DU.terms(W, amps, live)
    K = DU.EXTREME_K
    want = DU.reference(T, 1, 1, K)
    assert DU.same_bytes(DU.run_model(W, T, K)[0], want)
    n = len(DU.EXTREMES) + 1
    assert int(want["kept"][0, 0]) == int(want["eligible"][0, 0]) == n < K
    p = want["power"][0, 0, :n]
    assert np.isfinite(p).all() and (p[-3:] == 0).all() and (p[:-3] > 0).all() and (np.diff(p) <= 0).all()
    assert (p[:2] == p[0]).all() and (want["bounce"][0, 0, :2] == (0, 1)).all()
    ties = np.nonzero(p == 25)[0]
    key = [(int(want["bounce"][0, 0, s]), int(want["path"][0, 0, s])) for s in ties]
    assert len(ties) == 4 and key == sorted(key) and {b for b, _ in key} == {0, 1}
    assert np.signbit(want["a_te"][0, 0, n - 3:n].real).any()   # a -0.0 keeps its sign
