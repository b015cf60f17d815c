"""The planted live lists of tests/test_gpu_records_planted.py are what they claim to be -- checked with the oracle alone,
no GPU: every class of tests/records_util.py is non-empty where it is planted, the states are rows of the table with
values no two entries share, the served lanes lie inside what the patch masks are proven for, the reference changes with
the RX order, and every wrong reading of the record rule (records_util.CONTROLS) differs from the reference on the planted
lists.  The class counts are printed (records_util's module text keeps the first run's)."""
import numpy as np
import pytest

from oracle import oracle

from . import candidates_util as CU
from . import records_util as RU

#: class -> the cases that must have it
PLANTED = dict(
    t_eq1=("slab",), t_above=("slab",), t_below=("slab",),
    carry=RU.CASES, converse=RU.CASES, blocked0=RU.CASES,
    f2_below=("slab",), f2_above=RU.CASES,
    served=RU.CASES, off_grid=RU.CASES, unserved_row=("slab",),
    mixed_waves=RU.CASES, distinct_row_waves=RU.CASES,
    moving=("slab",), blocker_moves=("slab",),
)
#: control -> the cases whose lists must catch it (the canyon is static and has no float coincidence)
CAUGHT = dict(
    blocked_at_t_lt_1=("slab",), theta_not_carried=RU.CASES, theta_from_blocking_hits_only=RU.CASES,
    always_divide=("slab",), rx_order_reversed=RU.CASES, dfs_from_w_plus_d=("slab",), mvel_of_the_blocker=("slab",),
    te_tm_swapped=RU.CASES, tau_without_own=RU.CASES,
)

_cl = {}


def _case(name, tmp_path_factory):
    if name not in _cl:
        c = RU.case(name, tmp_path_factory.mktemp("records_design"))
        _cl[name] = (c, RU.classes(c))
    return _cl[name]


@pytest.mark.parametrize("name", RU.CASES)
def test_states_are_valid(name, tmp_path_factory):
    c, _ = _case(name, tmp_path_factory)
    st, tb = c["states"], c["tb"]
    n = RU.MASTER_N
    assert st["tri"].shape == (n,) and n <= 2048 and len(c["scene"]["rx_pos"]) <= 4
    assert (st["tri"] < tb["T"]).all(), "a planted state leaves the table"
    assert 65 <= tb["T"] <= CU.PATCH_MAX_TRI, "no patch tables on this scene"
    for k in ("o", "d", "theta", "amp", "tau"):
        assert np.isfinite(st[k]).all(), k
    assert np.unique(st["theta"]).size == n and np.unique(st["tau"]).size == n
    assert np.unique(st["amp"]).size == 4 * n and (st["amp"] != 0).all()
    assert ((st["theta"] > 0) & (st["theta"] < np.float32(np.pi / 2))).all()
    # d is a unit vector leaving the plane the origin was advanced from: o - 1e-4 d lies within hmax of the triangle's plane
    assert np.allclose((st["d"].astype(np.float64) ** 2).sum(axis=1), 1.0, atol=1e-5)
    _, _, h = CU.cell_coords(tb["g"], st["tri"].astype(np.int64), np.maximum(tb["nuv"], 1), st["o"].astype(np.float64))
    assert (np.abs(h) <= float(tb["hmax"])).all()
    # the served lanes: an independent statement of "inside the grid, close to the plane" (candidates_util.classes is
    # checked by tests/test_candidates_design.py)
    served = c["cls"] == CU.MUST
    fu, fv, h = CU.cell_coords(tb["g"], st["tri"][served].astype(np.int64), tb["nuv"], st["o"][served].astype(np.float64))
    nuv = tb["nuv"][st["tri"][served]].astype(np.float64)
    assert ((fu >= -1 / 64) & (fu <= nuv[:, 0] + 1 / 64) & (fv >= -1 / 64) & (fv <= nuv[:, 1] + 1 / 64)).all()
    assert (np.abs(h) <= float(tb["hmax"]) - 1e-5).all()
    # lists: prefixes, a permutation that moves entries across waves and chunks, replaced neighbours
    assert sorted(RU.PERM.tolist()) == list(range(n))
    assert (RU.PERM // 64 != np.arange(n) // 64).mean() > 0.9 and (RU.PERM // 256 != np.arange(n) // 256).mean() > 0.5
    rep = RU.replaced(st)
    odd = np.arange(n) % 2 == 1
    assert np.array_equal(rep["o"][~odd], st["o"][~odd]) and np.array_equal(rep["tau"][~odd], st["tau"][~odd])
    assert (rep["tau"][odd] != st["tau"][odd]).all()
    assert max(RU.LENGTHS) <= n and set(RU.LENGTHS) == {1, 63, 64, 65, 255, 256, 257, 1023, 1025}


@pytest.mark.parametrize("name", RU.CASES)
def test_classes_are_planted(name, tmp_path_factory):
    c, cl = _case(name, tmp_path_factory)
    counts = {k: int(len(v)) for k, v in cl.items() if not k.startswith("_")}
    print("records classes %s: %s" % (name, counts))
    for k, cases in PLANTED.items():
        if name in cases:
            assert counts[k] > 0, "class %s is empty on %s" % (k, name)
    assert counts["distinct_row_waves"] >= 2 and counts["mixed_waves"] >= 6
    if name == "slab":
        tb = c["tb"]
        assert (tb["nuv"][:, 0] == 0).sum() == 1, "the needle alone is refused a grid"
        # mixed waves hold all three kinds of lane at once
        w = np.arange(RU.MASTER_N) // 64
        full = [k for k in cl["mixed_waves"] if np.isin(cl["unserved_row"], np.flatnonzero(w == k)).any()
                and np.isin(cl["off_grid"], np.flatnonzero(w == k)).any()]
        assert len(full) >= 6
        # the searched states are what the oracle says they are, and served
        for k in ("t_eq1", "t_above", "t_below", "f2_below"):
            assert (c["cls"][cl[k]] == CU.MUST).all(), k
        ub = cl["_ref"]["unblocked"]
        assert not ub[1, cl["t_eq1"]].any() and not ub[1, cl["t_below"]].any() and ub[1, cl["t_above"]].all()
        print("records classes slab: f2 == 1.0f exactly in %d entries (not required)" % counts["f2_exact"])


def test_reference_changes_with_the_rx_order(tmp_path_factory):
    a, cla = _case("canyon", tmp_path_factory)
    b, clb = _case("canyon_rxperm", tmp_path_factory)
    for k in ("tri", "o", "d", "theta", "amp", "tau"):
        assert np.array_equal(a["states"][k], b["states"][k])
    ra, rb = cla["_ref"], clb["_ref"]
    back = np.argsort(RU.RX_PERM)   # receiver k of the canyon is receiver back[k] of the permuted list
    same_rx = {f: rb[f][back] for f in rb}
    assert np.array_equal(same_rx["unblocked"], ra["unblocked"]), "blocking does not depend on the order"
    assert np.array_equal(same_rx["tau"].view(np.uint32), ra["tau"].view(np.uint32))
    assert RU.differs(ra, same_rx) > 100, "the carried theta must make the records depend on the RX order"


@pytest.mark.parametrize("name", RU.CASES)
def test_wrong_readings_are_caught(name, tmp_path_factory):
    c, cl = _case(name, tmp_path_factory)
    ref = cl["_ref"]
    ok = ref["unblocked"]
    # the numpy Doppler term the controls build on is the oracle's, bit for bit
    assert np.array_equal(RU.dfs_numpy(c, ref).view(np.uint32)[ok], ref["dfs"].view(np.uint32)[ok])
    for ctl in RU.CONTROLS:
        n = RU.differs(ref, RU.control(c, ctl, cl))
        print("records control %s on %s: %d slots differ" % (ctl, name, n))
        if name in CAUGHT[ctl]:
            assert n > 0, "the planted lists of %s do not catch %s" % (name, ctl)
    # `f2 >= 1` is no wrong reading: dividing by exactly 1 changes no bit (records_util's module text)
    assert RU.differs(ref, RU.control(c, "f2_ge_1", cl)) == 0
    # the prefix lists are caught too where the class sits in the prefix: the shortest list that catches each control
    if name == "slab":
        for ctl in ("theta_not_carried", "te_tm_swapped"):
            assert RU.differs(ref, RU.control(c, ctl, cl), n=63) > 0


def test_prefix_and_independence_hold_in_the_reference(tmp_path_factory):
    """what the GPU test asks of the device holds for the oracle: an entry's record depends on its own state alone"""
    c, cl = _case("slab", tmp_path_factory)
    ref = cl["_ref"]
    p = RU.reference(c, RU.take(c["states"], RU.PERM))
    rep = RU.reference(c, RU.replaced(c["states"]))
    for f in RU.FIELDS:
        assert np.array_equal(p[f].view(np.uint32), ref[f][:, RU.PERM].view(np.uint32))
        assert np.array_equal(rep[f][:, ::2].view(np.uint32), ref[f][:, ::2].view(np.uint32))
    short = RU.reference(c, RU.take(c["states"], np.arange(65)))
    assert RU.differs(short, {k: v[:, :65] for k, v in ref.items()}) == 0
    assert oracle.SENTINEL_U32 != RU.POISON


def test_the_entry_refuses_null_arguments_without_a_device(product_lib):
    import ctypes as C

    from hermespy_rt_amd import lib as hlib
    sh = hlib.Shard(2048, 0, 1, 0, 1)
    assert product_lib.hrt_debug_last_launch(None, C.byref(sh), None, 0) == -1
    assert b"hrt_debug_last_launch" in product_lib.hrt_last_error()
