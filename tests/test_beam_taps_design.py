"""The references and the design of the GPU tests of the beamformed taps, checked without a device on
PL.synthetic_terms, so that the GPU files cannot pass vacuously.

The float64 reference (tests/beam_taps_util.py): the direct sum from the definition equals beams.apply of a float64
array-taps sum, and the bound sees an unconjugated combiner, a conjugated precoder, swapped beam axes and a gain added
to the phase instead of multiplied.  The cases of tests/test_gpu_beam_taps_edges.py: every case's reference alone
meets the case's conditions, every negative control moves the reference by more than the tolerance, and every case
reaches the form and the edge it names (BT.tiling restates the tiling rule: this checks the cases, not the kernel)."""
import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_taps_util as BT
from . import beam_util as BU
from . import configs as K
from . import planted as PL

FA = K.C3["f_ghz"] * 1e9
LAM = PL.C0 / FA
NRX, NTX = len(K.C3["rx_pos"]), len(K.C3["tx_pos"])
MARGIN = 2.0


@pytest.fixture(scope="module")
def terms():
    return PL.synthetic_terms(NRX, NTX, 100, seed=9)


def _geometry():
    from .pathsum_util import _random, _upa
    return _random(7, 4 * LAM, 11), _upa(3, 5, LAM / 2), BU.random_weights(3, 7, 1), BU.random_weights(5, 15, 2)


# ------------------------------------------------------------------ the float64 reference
@pytest.mark.parametrize("fs,l_min", [(PL.FS, -3), (122.88e6, 0)], ids=["integer_delays", "fractional_delays"])
def test_direct_sum_is_the_contracted_array_taps(terms, fs, l_min):
    rxe, txe, wr, wt = _geometry()
    t = 3 * PL.DT + PL.DT * np.arange(3)
    fc = PL.FC if fs == PL.FS else FA
    ref, = BT.beam_taps_direct(terms, NRX, NTX, rxe, txe, [(wr, wt)], 0.75 * FA, fs, fc, 40, l_min, t)
    h = BT.array_taps_direct(terms, NRX, NTX, rxe, txe, 0.75 * FA, fs, fc, 40, l_min, t)
    want = beams.apply(h, wr.astype(np.complex128), wt.astype(np.complex128))
    assert np.abs(want).max() > 1.0
    assert np.abs(ref - want).max() <= 1e-9 * np.abs(want).max()
    # with one beam of one unit weight on an element at the origin it is the plain taps sum
    one, w1 = np.zeros((1, 3)), np.ones((1, 1))
    ref, = BT.beam_taps_direct(terms, NRX, NTX, one, one, [(w1, w1)], FA, fs, fc, 40, l_min, t)
    assert np.abs(ref[:, :, 0, 0] - PL.taps_direct(terms, NRX, NTX, fs, fc, 40, l_min, t)).max() <= 1e-12


def test_the_bound_sees_a_wrong_convention(terms):
    """each wrong reading of the definition misses the bound, by a wide margin"""
    rxe, txe, wr, wt = _geometry()
    t = PL.DT * np.arange(2)
    S = BU.amplitude_sums(terms, NRX, NTX)
    args = (terms, NRX, NTX, rxe, txe)
    grid = (FA, 122.88e6, FA, 24, -2, t)
    ref, = BT.beam_taps_direct(*args, [(wr, wt)], *grid)
    BU.check(ref.astype(np.complex64), ref, S, wr, wt, what="the reference itself")
    wrong = {
        "unconjugated combiner": BT.beam_taps_direct(*args, [(wr, wt)], *grid, conj_rx=False)[0],
        "conjugated precoder": BT.beam_taps_direct(*args, [(wr, wt)], *grid, conj_tx=True)[0],
        "gain added to the phase": BT.beam_taps_direct(*args, [(wr, wt)], *grid, gain_as_phase=True)[0],
    }
    lim = BU.bound(S, wr, wt)
    for what, h in wrong.items():
        err = np.abs(h - ref).reshape(*ref.shape[:5], -1).max(axis=-1)
        print("%s: %.3g times the bound" % (what, (err / lim).max()))
        assert (err / lim).max() > 100.0, what
        with pytest.raises(AssertionError):
            BU.check(h.astype(np.complex64), ref, S, wr, wt, what=what)
    # swapped beam axes: square codebooks on the same elements, so that the shapes agree
    ws = BU.random_weights(3, 7, 5)
    a, = BT.beam_taps_direct(terms, NRX, NTX, rxe, rxe, [(wr, ws)], *grid)
    err = np.abs(a.transpose(0, 1, 3, 2, 4, 5, 6) - a).reshape(*a.shape[:5], -1).max(axis=-1)
    assert (err / BU.bound(S, wr, ws)).max() > 100.0
    with pytest.raises(AssertionError):
        BU.check(np.ascontiguousarray(a.transpose(0, 1, 3, 2, 4, 5, 6)).astype(np.complex64), a, S, wr, ws, what="swapped")


# ------------------------------------------------------------------ the tiling mirror and the edge cases
def test_tiling_mirror_on_the_limits():
    """the slot rule holds for every small shape and at the limits (the mirror's own consistency)"""
    for br in (1, 2, 3, 5, 13, 64, 65, 256):
        for bt in (1, 2, 4, 5, 12, 13, 63, 64, 65, 66, 256):
            for nt in (1, 2, 3, 5, 63, 64, 65):
                if br * bt * nt <= 1 << 16:
                    assert not BT.tiling_errors(br, bt, nt, 17), (br, bt, nt)
    assert BT.tiling(3, 4, 1, 16)["form"] == 1 and BT.tiling(13, 1, 1, 16)["form"] == 4
    assert BT.tiling(1, 1, 12, 16)["form"] == 1 and BT.tiling(1, 1, 13, 16)["form"] == 4


@pytest.mark.parametrize("name", BT.EDGE_NAMES)
def test_case_reaches_the_form_and_edge_it_names(name):
    c = BT.edge_case(name, LAM)
    br, bt = c["wr"].shape[0], c["wt"].shape[0]
    assert (br, bt, c["nt"], c["nl"], c["rxe"].shape[0], c["txe"].shape[0]) == BT.EDGE_SHAPES[name][:6]
    tl = BT.tiling(br, bt, c["nt"], c["nl"])
    form, rblocks, cblocks, pairs = c["expect"]
    assert (tl["form"], tl["rblocks"], tl["cblocks"]) == (form, rblocks, cblocks), (name, tl)
    assert [(b["pf"], b["pl"]) for b in tl["blocks"]] == pairs, name
    assert not BT.tiling_errors(br, bt, c["nt"], c["nl"])
    assert len(c["controls"]) >= 2, name
    inside = [b["row0"] % c["nt"] != 0 for b in tl["blocks"]]
    per_pair = bt > tl["cap"]
    wraps = [any(b["tx"][s] < b["tx"][s - 1] for s in range(1, len(b["tx"]))) for b in tl["blocks"]]
    what = {"f12_t3": inside == [False, True, True], "t3": inside == [False, True, True], "t5": inside == [False, True],
            "t64": not any(inside) and all(b["pf"] == b["pl"] for b in tl["blocks"]),
            "t65": inside == [False, True, True, True, True],
            "f12_bt12": per_pair, "tx65": per_pair, "tx256": per_pair, "tx63": not per_pair, "tx64": not per_pair,
            "bt65_wrap": per_pair and wraps == [False, True, True, False],
            "p64": tl["blocks"][0]["na"] == 8 and len(tl["blocks"][0]["tx"]) == 8,
            "p65": [b["na"] for b in tl["blocks"]] == [5, 1], "p130": [b["na"] for b in tl["blocks"]] == [5, 6, 1],
            "rx65": [b["na"] for b in tl["blocks"]] == [64, 1] and all(b["tx"] == [0] for b in tl["blocks"]),
            "f13": tl["blocks"][0]["na"] == 13}
    assert what.get(name, True), (name, tl)


def test_the_cases_cover_the_element_tiles_and_column_tiles():
    shapes = BT.EDGE_SHAPES.values()
    assert {1, 32, 33, 256} <= {s[4] for s in shapes} and {1, 32, 33, 256} <= {s[5] for s in shapes}
    assert {1, 15, 17, 65} <= {s[3] for s in shapes}
    assert any(s[6] < 0 for s in shapes) and any(s[7] != 0 for s in shapes) and any(s[8] != 1.0 for s in shapes)
    assert {s[0] * s[1] * s[2] for s in shapes} >= {12, 13, 64, 65, 130}


def _unit_bound(c):
    return BU.UNIT_TOL * np.abs(c["wr"]).sum(axis=1)[:, None] * np.abs(c["wt"]).sum(axis=1)[None, :]


def _over_bound(d, c):
    """max |d| / bound per (rx, tx, a, b) over (pol, m, l)"""
    return (np.abs(d).reshape(*d.shape[:4], -1).max(axis=-1) / _unit_bound(c)).max()


@pytest.mark.parametrize("name", BT.EDGE_NAMES)
def test_reference_meets_its_conditions_and_every_control_moves_it(terms, name):
    c = BT.edge_case(name, LAM)
    books = [(c["wr"], c["wt"])] + [BU.change_weight(c["wr"], c["wt"], *ctl[1:]) for ctl in c["controls"]]
    refs = BT.edge_direct(terms, NRX, NTX, c, books, FA)
    # the right reference passes its own check, so a failure under a control is the control's; every tap of the window
    # holds at most one term per link (integer delays), and some tap holds one
    BU.check_unit(refs[0].astype(np.complex64), refs[0], c["wr"], c["wt"], name)
    k = terms["n"] - c["l_min"]
    seen = (k >= 0) & (k < c["nl"])
    per_tap = np.bincount(PL.link_of(terms, NTX)[seen] * c["nl"] + k[seen], minlength=NRX * NTX * c["nl"])
    assert per_tap.max() == 1 and seen.any()
    empty = np.nonzero(per_tap.reshape(NRX, NTX, c["nl"]) == 0)
    assert (refs[0][empty[0], empty[1], ..., empty[2]] == 0).all()
    for ctl, ref in zip(c["controls"], refs[1:]):
        ratio = _over_bound(ref - refs[0], c)
        print("%s, %s (%s beam %d element %d %s): %.3g times the bound" % ((name,) + ctl + (ratio,)))
        assert ratio >= MARGIN, (name, ctl, ratio)
        with pytest.raises(AssertionError):
            BU.check_unit(refs[0].astype(np.complex64), ref, c["wr"], c["wt"], name)
    # one planted record of the window changed: the reference moves by that record's own term
    for what, i in BT.window_records(terms, c):
        one = PL.select(terms, np.array([i]))
        own, = BT.edge_direct(one, NRX, NTX, c, books[:1], FA)
        swapped, = BT.edge_direct(PL.mutate(one, 0, "swap"), NRX, NTX, c, books[:1], FA)
        for how, d in (("drop", own), ("double", own), ("swap", swapped - own)):
            ratio = _over_bound(d, c)
            print("%s, record %s %s: %.3g times the bound" % (name, what, how, ratio))
            assert ratio >= MARGIN, (name, what, how, ratio)
