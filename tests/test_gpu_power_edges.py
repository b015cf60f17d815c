"""The bin rules of the power profiles (include/hermespy_rt.h, hrt_compute_power_profiles) on records planted ON the
bin edges (tests/power_edges_util.py; the design is checked without a device by tests/test_power_edges_design.py).

C4_DOPPLER at 1100 rays: 2 x 2 links, two record chunks.  After PL.plant, every unblocked scatter record and every
clear LoS entry gets a delay and a direction from the edge classes: tau0 + k dtau for k = 0, Ld - 1, Ld and their
float32 neighbours, the axes and poles with both signs of every zero, |u_z| > 1, the thirds, the diagonals.  Powers
stay dyadic, so every comparison of a histogram here is at tolerance 0, against the header's formulas in float64 numpy:

  pdp, arrival     exact for every part, grid, Ld (the LDS and the global form of the hist kernel) and tau0;
  departure        exact with scatter=False (the LoS u_tx is planted).  A scatter record's u_tx is the launch
                   direction of its ray, which comes from the launch table and cannot be planted: with scatter the
                   departure spectrum keeps pathsum_util.power_check (its edge slack is 0 unless a launch direction
                   happens to stand within 1e-6 of an edge);
  moments          COUNT, P, P_TAU, P_NU, P_NU2, P_LOS, P_URX_* exact: their float64 sums are exact in any order
                   (PE.sum_is_exact).  P_TAU2 is exact on the planting without the float32 neighbours; with them the
                   squares carry 48 bits at 2^-114 against sums near 2^-30, no float64 sum of them is exact, and
                   P_TAU2 is held to the rounding bound of a float64 sum, (N - 1) 2^-53 sum |w|, below a sixteenth of
                   its smallest term (test_power_edges_design.py);
  closure          arrival.sum() == P, pdp.sum() == P - P_outside, exactly;
  negative controls  the device output fails the check against every wrong rule of PE.VARIANTS and against the
                   reference changed in one record (PL.control_records x PL.MUTATIONS)."""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import planted as PL
from . import power_edges_util as PE
from .pathsum_util import PARTS, _expect_failure, _force_los_classes, _tracer, power_check, power_reference

pytestmark = pytest.mark.gpu

RAYS = 1100
PW_LDS_MAX = 80 << 10   # csrc/hrt_power.h HRT_PW_LDS_MAX
ALL_LD = PE.LDS + (PE.LD_GLOBAL,)
EXACT = tuple(n for n in PE.MOMENTS.values() if n != "P_TAU2")


def _np(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _sel(T, los, scatter):
    return PL.select(T, (T["los"] & los) | (~T["los"] & scatter))


def _plant(tr, ld, tau0, salt=0, neighbours=True, keyed=False):
    return PE.plant_edges(tr, PL.plant(tr, keyed=keyed), ld, tau0, salt, neighbours)


def _run(tr, tau0, ld, grid, **kw):
    return _np(tr.power_profiles(tau0, PE.DTAU, ld, grid[0], grid[1], **kw))


def _form(ld, grid):
    return "global" if 2 * (ld + 2 * grid[0] * grid[1]) * 8 > PW_LDS_MAX else "lds"


def _check(got, T, tr, tau0, ld, grid, scatter, tag, moments=EXACT):
    """every check of this module on one output against the terms T"""
    nrx, ntx = tr.nrx, tr.ntx
    ref = PE.edge_reference(T, nrx, ntx, tau0, PE.DTAU, ld, grid[0], grid[1])
    PE.check_edges(got, ref, str(tag), ("pdp", "arrival"), T, ntx)
    if scatter:
        power_check(got, power_reference(PL.power_terms(T, nrx, ntx), tau0, PE.DTAU, ld, grid[0], grid[1]), tag)
    else:
        PE.check_edges(got, ref, str(tag), ("departure",), T, ntx)
    PE.check_moments(got, T, nrx, ntx, want_exact=moments)
    P = got["moments"][..., abi.POWER_P]
    assert np.array_equal(got["arrival"].sum(axis=(-2, -1)), P), (tag, "arrival closure")
    assert np.array_equal(got["departure"].sum(axis=(-2, -1)), P), (tag, "departure closure")
    assert np.array_equal(got["pdp"].sum(axis=-1), P - ref["outside"]), (tag, "pdp closure")
    return ref


@pytest.fixture(scope="module")
def traced():
    tr = _tracer(K.small(K.C4_DOPPLER, RAYS))
    tr.trace()
    yield tr
    tr.close()


def test_every_link_holds_every_class(traced):
    tr = traced
    assert (tr.nrx, tr.ntx) == (2, 2)
    for salt in (0, 1):
        T, dc, ac = _plant(tr, 3, 0.0, salt)
        sc = ~T["los"]
        link = PL.link_of(T, tr.ntx)
        print("salt", salt, "scatter terms per link", np.bincount(link[sc], minlength=4), "LoS terms", int((~sc).sum()))
        for lk in range(4):
            s = sc & (link == lk)
            assert set(dc[s]) == set(range(len(PE.DELAY_CLASSES))), (salt, lk, "delay", np.bincount(dc[s]))
            assert set(ac[s]) == set(range(len(PE.DIRS))), (salt, lk, "direction", np.bincount(ac[s]))
        # the window cuts terms off on both sides, and they stay in the moments (checked below)
        x = (T["tau"] - 0.0) / PE.DTAU
        assert (x < 0).any() and (x >= 3).any()


@pytest.mark.parametrize("tau0", PE.TAU0S, ids=["tau0_0", "tau0_16"])
@pytest.mark.parametrize("ld", ALL_LD)
def test_pdp_arrival_and_moments_are_exact(traced, ld, tau0):
    tr = traced
    T, _, _ = _plant(tr, ld, tau0)
    forms = set()
    for grid in PE.GRIDS:
        forms.add(_form(ld, grid))
        for los, scatter in PARTS:
            got = _run(tr, tau0, ld, grid, los=los, scatter=scatter)
            _check(got, _sel(T, los, scatter), tr, tau0, ld, grid, scatter, (ld, tau0, grid, los, scatter))
    assert forms == ({"global"} if ld == PE.LD_GLOBAL else {"lds", "global"})


@pytest.mark.parametrize("ld", [3, PE.LD_GLOBAL])
def test_every_moment_is_exact_without_the_float32_neighbours(traced, ld):
    tr = traced
    tau0 = PE.TAU0S[1]
    T, _, _ = _plant(tr, ld, tau0, neighbours=False)
    for los, scatter in PARTS:
        got = _run(tr, tau0, ld, (3, 5), los=los, scatter=scatter)
        _check(got, _sel(T, los, scatter), tr, tau0, ld, (3, 5), scatter, ("plain", ld), tuple(PE.MOMENTS.values()))


def test_both_forms_of_the_hist_kernel_agree(traced):
    tr = traced
    tau0, grid = 0.0, (3, 5)
    T, _, _ = _plant(tr, 64, tau0)
    assert _form(64, grid) == "lds" and _form(PE.LD_GLOBAL, grid) == "global"
    a = _run(tr, tau0, 64, grid)
    b = _run(tr, tau0, PE.LD_GLOBAL, grid)
    _check(a, T, tr, tau0, 64, grid, True, "lds")
    _check(b, T, tr, tau0, PE.LD_GLOBAL, grid, True, "global")
    assert np.array_equal(a["pdp"], b["pdp"][..., :64])
    assert (b["pdp"][..., 64] > 0).all() and not b["pdp"][..., 65:].any()   # the `end` classes, nothing beyond
    for k in ("arrival", "departure", "moments"):
        assert np.array_equal(a[k], b[k]), k


LOS_WANTED = [j for j, (kind, v) in enumerate(PE.DIRS)
              if (kind == "axis" and v[1] == 0) or kind == "clamp" or (kind == "near" and v[0] == -1)]
LOS_GRIDS = [(1, 1), (2, 4), (3, 5), (8, 8)]   # even and odd Nth, Nph


def _los_salts(T, clear):
    """{salt: class}: for every direction class of LOS_WANTED the least salt that gives it to a clear LoS entry"""
    Tl = PL.select(T, clear)
    found = {}
    for salt in range(1 << 14):
        _, ac, _ = PE.classes(Tl, salt)
        for c in ac:
            if c in LOS_WANTED and c not in found.values():
                found[salt] = int(c)
        if len(found) == len(LOS_WANTED):
            break
    return found


def test_los_through_the_reduce_kernel():
    """scatter=False: the reduce kernel bins the LoS term itself.  A coincident and a blocked entry are forced; the
    clear entries take the edge classes, u_rx = -(double)u_tx with the zeros' signs flipped, the salts chosen so that
    they reach the x axis on both sides of the azimuth wrap, the poles with every atan2(+-0, +-0), |u_z| > 1 and the
    directions just inside the wrap; the coincident term lands in the bins of the header's u_rx = (1, 0, 0),
    u_tx = (-1, 0, 0)"""
    tr = _tracer(K.small(K.C4_DOPPLER, RAYS))
    tr.trace()
    _force_los_classes(tr)
    st = PL.los_status(tr)
    assert (st == 0).sum() >= 1 and (st == 1).sum() >= 1 and (st == 2).sum() >= 1, st
    T0 = PL.plant(tr)
    clear = T0["los"] & (st[np.maximum(T0["rx"], 0), np.maximum(T0["tx"], 0)] == 2)
    salts = _los_salts(T0, clear)
    assert sorted(salts.values()) == sorted(LOS_WANTED)
    for n, salt in enumerate(salts):
        tau0, ld = PE.TAU0S[n % 2], (3, 1)[n % 2]
        T, dc, ac = PE.plant_edges(tr, T0, ld, tau0, salt)
        assert salts[salt] in ac[clear]
        Tl = _sel(T, True, False)
        assert Tl["rx"].size == int((st != 1).sum())
        for grid in LOS_GRIDS:
            nth, nph = grid
            got = _run(tr, tau0, ld, grid, scatter=False)
            _check(got, Tl, tr, tau0, ld, grid, False, ("los", grid, salt, PE.DIRS[salts[salt]]))
            for rx, tx in np.argwhere(st == 0):      # coincident: one unit term per polarisation
                want_a = np.zeros((nth, nph))
                want_a[min(nth // 2, nth - 1), nph // 2] = 1.0      # theta = pi / 2, phi = 0: x = Nth / 2, Nph / 2
                want_d = np.zeros((nth, nph))
                want_d[min(nth // 2, nth - 1), 0] = 1.0             # phi = pi: index Nph wraps to 0
                want_p = np.zeros(ld)
                if tau0 == 0.0:
                    want_p[0] = 1.0                             # tau = tau0: bin 0; tau0 = 16 dtau: before the window
                for pol in range(2):
                    assert np.array_equal(got["arrival"][rx, tx, pol], want_a), (grid, salt, "arrival")
                    assert np.array_equal(got["departure"][rx, tx, pol], want_d), (grid, salt, "departure")
                    assert np.array_equal(got["pdp"][rx, tx, pol], want_p), (grid, salt, "pdp")
            for rx, tx in np.argwhere(st == 1):      # blocked: nothing
                for k in ("moments", "pdp", "arrival", "departure"):
                    assert not got[k][rx, tx].any(), (grid, salt, k)
    tr.close()


def test_accumulate_twice_is_twice(traced):
    tr = traced
    tau0, ld, grid = PE.TAU0S[1], 64, (8, 8)
    _plant(tr, ld, tau0)
    once = tr.power_profiles(tau0, PE.DTAU, ld, *grid)["buffer"].clone()
    out = tr.torch.zeros_like(once)
    for _ in range(2):
        tr.power_profiles(tau0, PE.DTAU, ld, *grid, out=out, accumulate=True)
    assert bool(tr.torch.equal(out, 2.0 * once))
    assert bool((once != 0).any())


def test_shards_accumulate_to_the_whole(traced):
    """world = 2 shards (chunk = 64) planted by global identity accumulate to exactly the whole launch set's bins"""
    c = K.small(K.C4_DOPPLER, RAYS)
    tau0, ld, grid, world = 0.0, 3, (3, 5), 2
    T, _, _ = _plant(traced, ld, tau0, keyed=True)
    whole = _run(traced, tau0, ld, grid)
    _check(whole, T, traced, tau0, ld, grid, True, "whole")
    pw, parts = None, []
    for r in range(world):
        ts = _tracer(c, rank=r, world=world, chunk=64)
        ts.trace()
        U, _, _ = _plant(ts, ld, tau0, keyed=True)
        parts.append(PL.select(U, ~U["los"]))
        a = pw is not None
        pw = ts.power_profiles(tau0, PE.DTAU, ld, *grid, out=pw["buffer"] if a else None, accumulate=a)
        ts.torch.cuda.synchronize(ts.device)
        got = _np(pw)
        ts.close()
    S, Tsc = PL.concat(*parts), PL.select(T, ~T["los"])
    key = lambda X: np.lexsort((X["bounce"], X["path"], X["tx"], X["rx"]))   # noqa: E731
    a, b = key(S), key(Tsc)
    for k in ("rx", "tx", "path", "bounce", "a_te", "a_tm", "nu", "tau", "urx"):
        assert np.array_equal(S[k][a], Tsc[k][b]), k
    _check(got, T, traced, tau0, ld, grid, True, "shards")
    for k in ("pdp", "arrival", "departure"):
        assert np.array_equal(got[k], whole[k]), k


@pytest.mark.parametrize("ld,tau0,grid", [(3, PE.TAU0S[0], (3, 5)), (64, PE.TAU0S[1], (8, 8)),
                                          (PE.LD_GLOBAL, PE.TAU0S[0], (2, 4))])
def test_negative_controls(traced, ld, tau0, grid):
    """the device output passes against the header's rules, fails against every wrong rule and every changed record"""
    tr = traced
    T, _, _ = _plant(tr, ld, tau0)
    got = _run(tr, tau0, ld, grid)
    keys = ("pdp", "arrival")
    PE.check_edges(got, PE.edge_reference(T, tr.nrx, tr.ntx, tau0, PE.DTAU, ld, *grid), "true", keys)
    for v, what in PE.VARIANTS.items():
        var = PE.edge_reference(T, tr.nrx, tr.ntx, tau0, PE.DTAU, ld, *grid, variant=v)
        with pytest.raises(AssertionError):
            PE.check_edges(got, var, v, keys)
            print("the check passed against variant %s (%s)" % (v, what))
    _expect_failure(lambda U: PE.check_edges(got, PE.edge_reference(U, tr.nrx, tr.ntx, tau0, PE.DTAU, ld, *grid),
                                             "control", keys), T, "power edges")
    # LoS alone: the departure rule through the reduce kernel
    got = _run(tr, tau0, ld, grid, scatter=False)
    Tl = _sel(T, True, False)
    PE.check_edges(got, PE.edge_reference(Tl, tr.nrx, tr.ntx, tau0, PE.DTAU, ld, *grid), "los")
    k = int(np.nonzero(T["los"])[0][0])
    for how in PL.MUTATIONS[:2]:
        with pytest.raises(AssertionError):
            PE.check_edges(got, PE.edge_reference(_sel(PL.mutate(T, k, how), True, False), tr.nrx, tr.ntx, tau0,
                                                  PE.DTAU, ld, *grid), "los " + how)
