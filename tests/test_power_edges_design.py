"""The design of tests/test_gpu_power_edges.py, checked without a device on PL.synthetic_terms given the edge classes
of tests/power_edges_util.py, so that the GPU file cannot pass vacuously: every class's bin coordinate, by the
formulas of include/hermespy_rt.h in float64 numpy, is the exact integer it is planted for and lands in the stated
bin; every link holds every class; every wrong rule of PE.VARIANTS moves at least one bin of every link; and the
moment sums are exact in any order where the GPU file compares them at tolerance 0."""
import numpy as np
import pytest

from . import planted as PL
from . import power_edges_util as PE
from .pathsum_util import _azi, _zen

NRX, NTX = 2, 2
PER_LINK = 450     # the GPU file's trace leaves 454 or 455 scatter terms per link
ALL_LD = PE.LDS + (PE.LD_GLOBAL,)


@pytest.fixture(scope="module")
def terms():
    return PL.synthetic_terms(NRX, NTX, PER_LINK, seed=4)


def _name(dc):
    return np.array([c[0] for c in PE.DELAY_CLASSES])[dc]


def test_the_delay_grid_is_what_the_module_says():
    k = np.arange(0, 2 * PE.LD_GLOBAL + 64)
    for tau0 in PE.TAU0S:
        tau = PE.delay_value(k, np.zeros_like(k), tau0).astype(np.float64)   # (asserts exactness in float32)
        assert np.array_equal((tau - tau0) / PE.DTAU, k.astype(np.float64))
    for ks in PE.SMALL_K + ALL_LD + tuple(ld // 2 for ld in ALL_LD if ld > 1):
        assert (ks * PE.DTAU) * (1.0 / PE.DTAU) < ks, ks
    assert np.float32(PE.DTAU) == PE.DTAU and np.float32(PE.TAU0S[1]) == PE.TAU0S[1]


@pytest.mark.parametrize("tau0", PE.TAU0S)
@pytest.mark.parametrize("ld", ALL_LD)
def test_delay_classes_land_in_their_bins(terms, ld, tau0):
    U, dc, _ = PE.edge_values(terms, ld, tau0)
    assert np.array_equal(U["tau"].astype(np.float32).astype(np.float64), U["tau"])
    x = (U["tau"] - tau0) / PE.DTAU
    kd, ok = PE.delay_bins(U["tau"], tau0, PE.DTAU, ld)
    name = _name(dc)
    want = {"first": (0, True), "middle": (ld // 2, True), "last": (ld - 1, True), "end": (ld, False)}
    for cls, (k, kept) in want.items():
        s = name == cls
        assert s.any() and np.all(x[s] == k) and np.all(ok[s] == kept), cls
        assert np.all(kd[s] == k), cls
    s = name == "small"
    assert np.all(x[s] == np.rint(x[s])) and np.all(ok[s]) and np.isin(x[s], np.asarray(PE.SMALL_K) % ld).all()
    s = name == "first-"
    assert s.any() and np.all((x[s] > -1) & (x[s] < 0)) and not ok[s].any()
    s = name == "first+"
    assert s.any() and np.all((x[s] > 0) & (x[s] < 1)) and ok[s].all() and np.all(kd[s] == 0)
    s = name == "end-"
    assert s.any() and np.all((x[s] > ld - 1) & (x[s] < ld)) and ok[s].all() and np.all(kd[s] == ld - 1)
    s = name == "end+"
    assert s.any() and np.all((x[s] > ld) & (x[s] < ld + 1)) and not ok[s].any()
    # the neighbours are neighbours: one float32 step from the edge
    for cls, k in (("first-", 0), ("first+", 0), ("end-", ld), ("end+", ld)):
        edge = np.float32(tau0 + k * PE.DTAU)
        t = U["tau"][name == cls].astype(np.float32)
        side = np.float32(np.inf if cls.endswith("+") else -np.inf)
        assert np.all(t == np.nextafter(edge, side)), cls
    # without the neighbours every coordinate is an integer
    V, _, _ = PE.edge_values(terms, ld, tau0, neighbours=False)
    xv = (V["tau"] - tau0) / PE.DTAU
    assert np.array_equal(xv, np.rint(xv))


@pytest.mark.parametrize("grid", PE.GRIDS)
def test_direction_classes_land_in_their_bins(grid):
    nth, nph = grid
    u = PE.DIR_U.astype(np.float64)
    zi, zx = _zen(u, nth)
    ai, ax = _azi(u, nph)
    assert np.isfinite(zx).all() and np.isfinite(ax).all()
    assert zi.min() >= 0 and zi.max() < nth and ai.min() >= 0 and ai.max() < nph
    for j, (kind, v) in enumerate(PE.DIRS):
        x, y, z = v
        neg = lambda c: np.signbit(c)   # noqa: E731
        if kind == "axis" and x == -1:        # the wrap: phi = +pi -> index Nph -> bin 0; phi = -pi -> index 0
            assert ax[j] == (0.0 if neg(y) else nph) and ai[j] == 0, v
        if kind == "axis" and x == 1:         # phi = +-0
            assert ax[j] == nph / 2 and ai[j] == nph // 2, v
        if kind == "axis" and abs(y) == 1:
            assert ax[j] == (0.75 if y > 0 else 0.25) * nph, v
        if kind == "axis" and z == 0:
            assert zx[j] == nth / 2 and zi[j] == min(nth // 2, nth - 1), v
        if kind == "axis" and abs(z) == 1:    # the poles, with atan2(+-0, +-0)
            assert zx[j] == (0.0 if z > 0 else nth) and zi[j] == (0 if z > 0 else nth - 1), v
            phi = {(False, False): 0.0, (False, True): np.pi, (True, True): -np.pi, (True, False): -0.0}[
                (bool(neg(y)), bool(neg(x)))]
            assert np.arctan2(y, x) == phi and ai[j] == (0 if neg(x) else nph // 2), v
        if kind == "clamp":                   # acos of the unclamped value is NaN
            assert abs(z) > 1 and zx[j] == (0.0 if z > 0 else nth) and zi[j] == (0 if z > 0 else nth - 1), v
            with np.errstate(invalid="ignore"):
                assert np.isnan(np.arccos(z))
        if kind == "equator":
            assert zx[j] == nth / 2 and zi[j] == min(nth // 2, nth - 1), v
        if kind == "third":
            assert zx[j] * 3 == (nth if z > 0 else 2 * nth), v
            assert zi[j] == min((nth if z > 0 else 2 * nth) // 3, nth - 1), v
        if kind == "diagonal":
            eighth = {(1, 1): 5, (1, -1): 3, (-1, 1): 7, (-1, -1): 1}[(int(x), int(y))]
            assert ax[j] * 8 == eighth * nph and zx[j] == nth / 2, v
        if kind == "near" and x == -1:        # just inside the wrap, on either side
            assert (nph - 1e-6 < ax[j] < nph and ai[j] == nph - 1) if y > 0 else (0 < ax[j] < 1e-6 and ai[j] == 0), v
        if kind == "near" and x != -1:        # just north / south of the equator
            assert 0 < abs(zx[j] - nth / 2) < 1e-6 and zi[j] == min(int(np.floor(nth / 2 - z)), nth - 1), v
        if kind == "generic":
            for c in (zx[j], ax[j]):
                assert abs(c - np.rint(c)) > 0.15, (v, grid, c)


@pytest.mark.parametrize("salt", [0, 1, 2, 3])
def test_every_link_holds_every_class(terms, salt):
    dc, ac, pick = PE.classes(terms, salt)
    sc = ~terms["los"]
    link = PL.link_of(terms, NTX)
    for lk in range(NRX * NTX):
        s = sc & (link == lk)
        assert set(dc[s]) == set(range(len(PE.DELAY_CLASSES))), (lk, "delay")
        assert set(ac[s]) == set(range(len(PE.DIRS))), (lk, "direction")
        assert set(pick[s & (dc == len(PE.DELAY_CLASSES) - 1)]) == set(range(len(PE.SMALL_K))), (lk, "small k")


def test_los_terms_are_formed_as_the_kernel_forms_them(terms):
    """u_tx is the planted float32 direction, u_rx = -(double)u_tx with the zeros' signs flipped; over the salts the
    LoS entries of four links reach both sides of the azimuth wrap"""
    seen = set()
    for salt in range(64):
        U, dc, ac = PE.edge_values(terms, 3, 0.0, salt)
        s = U["los"]
        assert np.array_equal(U["utx"][s], PE.DIR_U[ac[s]].astype(np.float64))
        assert np.array_equal(U["urx"][s], -U["utx"][s])
        assert np.array_equal(np.signbit(U["urx"][s]), ~np.signbit(U["utx"][s]))
        seen |= set(ac[s])
        # scatter terms keep their traced u_tx
        assert np.array_equal(U["utx"][~s], terms["utx"][~s])
    wrap = {j for j, (k, v) in enumerate(PE.DIRS) if k == "axis" and v[0] == 1}   # u_rx = (-1, -+0, -+0)
    assert wrap <= seen


@pytest.mark.parametrize("tau0", PE.TAU0S)
@pytest.mark.parametrize("ld", ALL_LD)
@pytest.mark.parametrize("grid", PE.GRIDS)
def test_every_variant_moves_a_bin_of_every_link(terms, grid, ld, tau0):
    nth, nph = grid
    U, _, _ = PE.edge_values(terms, ld, tau0)
    ref = PE.edge_reference(U, NRX, NTX, tau0, PE.DTAU, ld, nth, nph)
    PE.check_edges(ref, ref, "self")
    P = np.stack([np.bincount(PL.link_of(U, NTX), weights=PE.powers(U)[:, q], minlength=NRX * NTX)
                  for q in range(2)], axis=1).reshape(NRX, NTX, 2)
    assert np.array_equal(ref["arrival"].sum(axis=(-2, -1)), P)
    assert np.array_equal(ref["pdp"].sum(axis=-1), P - ref["outside"]) and (ref["outside"] > 0).all()
    for v in PE.VARIANTS:
        var = PE.edge_reference(U, NRX, NTX, tau0, PE.DTAU, ld, nth, nph, variant=v)
        d = PE.differs_per_link(ref, var)
        if v == "c" and nph == 1:     # one azimuth bin: clamping index 1 to 0 and wrapping it to 0 are the same rule
            assert not d.any()
            continue
        if v == "g" and grid == (1, 1):
            # one angular bin takes every direction, and on this delay grid the float32 quotient is the float64 one:
            # tau, tau0 and dtau are float32 values, tau - tau0 is exact in float32 and a float32 neighbour of an
            # edge is a whole float32 ulp away from it, which the rounded quotient keeps
            assert not d.any()
            continue
        assert d.all(), (v, PE.VARIANTS[v], grid, ld, tau0, d)
        with pytest.raises(AssertionError):
            PE.check_edges(ref, var, v, keys=("pdp", "arrival"))
        # LoS terms alone (scatter=False on the device) tell the variants of the departure rule apart as well where
        # their classes reach it; not asserted per link: there is one LoS term per link


@pytest.mark.parametrize("tau0", PE.TAU0S)
@pytest.mark.parametrize("ld", ALL_LD)
def test_moment_sums_are_exact_in_any_order(terms, ld, tau0):
    """with the float32 neighbours planted every moment but P_TAU2 is exact in any order (the squares of the
    neighbours carry 48 bits, 2^-114 at the finest against sums near 2^-30: their float64 sum rounds); without them
    P_TAU2 is exact too"""
    for neighbours, inexact in ((True, {"P_TAU2"}), (False, set())):
        U, _, _ = PE.edge_values(terms, ld, tau0, neighbours=neighbours)
        for f, (ref, ex, bd) in PE.moments_reference(U, NRX, NTX).items():
            if PE.MOMENTS[f] in inexact:
                # the rounding bound stays below a sixteenth of the smallest single term
                w = np.abs(PE.moment_terms(U)[f])
                assert bd.max() < w[w > PE.TINY].min() / 16, (PE.MOMENTS[f], bd.max())
                continue
            assert ex.all() and not bd.any(), (PE.MOMENTS[f], neighbours, ld, tau0)


def test_sum_is_exact_tells_the_cases_apart():
    assert PE.sum_is_exact([1.0, 0.25, 4.0] * 1000)
    assert PE.sum_is_exact([1.0, 2.0 ** -149, -2.0 ** -149])
    assert not PE.sum_is_exact([1.0, 2.0 ** -60])
    assert not PE.sum_is_exact([(2.0 ** 24 + 1) ** 2 * 2.0 ** -114] * 100 + [49.0 ** 2 * 2.0 ** -78] * 2000)
