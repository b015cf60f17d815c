"""The design of tests/test_gpu_beam_edges.py, checked without a device on PL.synthetic_terms, so that the GPU file
cannot pass vacuously: the probe codebooks are what tests/beam_util.py promises, every case reaches the block, slot
and tile arithmetic it is there for (restated in BU.block_slots: this checks the cases, not the kernel), and every
negative control moves the float64 reference by at least twice the bound somewhere."""
import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_util as BU
from . import configs as K
from . import planted as PL

FA = K.C3["f_ghz"] * 1e9
NRX, NTX = len(K.C3["rx_pos"]), len(K.C3["tx_pos"])
MARGIN = 2.0


@pytest.fixture(scope="module")
def cases():
    return BU.edge_cases(PL.C0 / FA)


@pytest.fixture(scope="module")
def terms():
    # half the records per link of the GPU file's trace: a changed weight moves a sum of N unrelated terms by about
    # sqrt(N), the bound does not grow with N, so fewer records are the harder case for the controls
    return PL.synthetic_terms(NRX, NTX, 1500, seed=9)


def _blocks(c):
    br, bt = c["wr"].shape[0], c["wt"].shape[0]
    return [BU.block_slots(pb, br, bt) for pb in range(-(-br * bt // BU.PAIRS))]


def _wraps(tx):
    """slots s > 0 where the TX beam falls back to 0"""
    return [s for s in range(1, len(tx)) if tx[s] < tx[s - 1]]


def _tiles(W):
    return [sorted({int(e) // BU.ETILE for e in np.nonzero(w)[0]}) for w in W]


@pytest.mark.parametrize("beams_,elements,seed", [(256, 256, 0), (256, 256, 1), (32, 33, 0), (3, 64, 2), (3, 2, 0),
                                                  (5, 1, 0), (40, 65, 3)])
def test_probe_codebooks(beams_, elements, seed):
    W = BU.probe_weights(beams_, elements, seed)
    assert W.shape == (beams_, elements) and W.dtype == np.complex64
    nz = W != 0
    per = nz.sum(axis=1)
    assert per.min() >= 1 and per.max() <= 4
    assert np.abs(np.abs(W[nz]) - 1).max() < 1e-6
    ph = np.sort(np.angle(W[nz].astype(np.complex128)) / (2 * np.pi) % 1.0)
    if ph.size > 1:
        assert np.diff(ph).min() > 1e-5                     # distinct
        both = np.concatenate([ph, (-ph) % 1.0, (ph + 0.5) % 1.0, (0.5 - ph) % 1.0])
        assert np.diff(np.sort(both)).min() > 1e-6          # no conjugate, negated or mirrored partner either
    want = 1 + (np.arange(beams_) + seed) % 4
    assert (per <= want).all() and (per[want == 1] == 1).all()
    if elements > BU.ETILE:   # (a first weight that stands on a border leaves one border fewer for the others)
        assert (per >= np.minimum(want, 3)).all()
    borders = {e for e in (0, 31, 32, 63, 64, elements - 1) if e < elements}
    for a in range(beams_):
        e = np.nonzero(nz[a])[0]
        assert (37 * a + 5) % elements in e
        assert set(e) - {(37 * a + 5) % elements} <= borders
    if elements > BU.ETILE and beams_ >= 4:
        # every run of 32 consecutive beams (the RX slots of a block, or its TX slots) has a beam in two tiles
        two = np.array([len(t) >= 2 for t in _tiles(W)])
        assert all(two[a:a + 4].any() for a in range(beams_ - 3))


def test_cases_reach_what_they_are_there_for(cases):
    A, B, C, D32, D31, E, F = (_blocks(cases[n]) for n in ("A", "B", "C", "D32", "D31", "E", "F"))
    # A: na = 32 in every one of eight blocks, a0 = 32 pb; eight RX element tiles; one TX slot
    assert len(A) == 8 and all(b == (32 * pb, 32, [0], 32) for pb, b in enumerate(A))
    assert cases["A"]["rxe"].shape[0] == 8 * BU.ETILE and cases["A"]["txe"].shape[0] == 1
    # B: per-pair TX slots without a wrap, eight blocks and eight TX tiles
    assert len(B) == 8 and all(b == (0, 1, list(range(32 * pb, 32 * pb + 32)), 32) for pb, b in enumerate(B))
    assert cases["B"]["txe"].shape[0] == 8 * BU.ETILE
    # C: Bt = 33: the wrap stands at another slot in each block, inside the pairs of blocks 1 and 2; the last block has
    # 3 pairs; TX tiles 32 + 32 + 1
    assert len(C) == 4 and [b[3] for b in C] == [32, 32, 32, 3]
    wr = [_wraps(b[2]) for b in C]
    assert wr == [[], [1], [2], [3]] and all(w[0] < b[3] for w, b in zip(wr[1:3], C[1:3]))
    assert [b[:2] for b in C] == [(0, 1), (0, 2), (1, 2), (2, 1)]
    assert cases["C"]["txe"].shape[0] == 2 * BU.ETILE + 1
    # D: Bt = 32: one RX beam per block, every TX beam a slot; Bt = 31: the blocks straddle two RX beams; two full RX
    # tiles, TX tile + 1
    assert [b[:2] for b in D32] == [(0, 1), (1, 1)] and all(b[2] == list(range(32)) for b in D32)
    assert [b[:2] for b in D31] == [(0, 2), (1, 2), (2, 1)] and [b[3] for b in D31] == [32, 32, 29]
    assert cases["D32"]["rxe"].shape[0] == 2 * BU.ETILE and cases["D32"]["txe"].shape[0] == BU.ETILE + 1
    # E: Bt = 40 with a wrap inside blocks 1 and 2, two tiles on the RX side and three on the TX side
    assert len(E) == 3 and [_wraps(b[2]) for b in E] == [[], [8], [16]] and [b[3] for b in E] == [32, 32, 16]
    assert cases["E"]["rxe"].shape[0] == BU.ETILE + 1 and cases["E"]["txe"].shape[0] == 2 * BU.ETILE + 1
    # F: the element limit on both sides, one block of all pairs
    assert F == [(0, 4, list(range(8)), 32)]
    assert cases["F"]["rxe"].shape[0] == cases["F"]["txe"].shape[0] == 256
    # the probe sides: at least one beam of every block's slots has weights in two tiles
    for name, side in (("A", "rx"), ("B", "tx"), ("D32", "rx"), ("D32", "tx"), ("D31", "rx"), ("D31", "tx")):
        c = cases[name]
        tiles = _tiles(c["wt"] if side == "tx" else c["wr"])
        for a0, na, tx, pairs in _blocks(c):
            slots = range(a0, a0 + na) if side == "rx" else (tx[:pairs] if len(tiles) > BU.PAIRS else tx)
            assert any(len(tiles[s]) >= 2 for s in slots), (name, side, a0)


def _unit_bound(c):
    return BU.UNIT_TOL * np.abs(c["wr"]).sum(axis=1)[:, None] * np.abs(c["wt"]).sum(axis=1)[None, :]


def _over_bound(d, c):
    """max |d| / bound per (rx, tx, a, b) over (pol, m, k)"""
    return (np.abs(d).reshape(*d.shape[:4], -1).max(axis=-1) / _unit_bound(c)).max()


@pytest.mark.parametrize("name", ["A", "B", "C", "D32", "D31", "E", "F"])
def test_every_control_moves_the_reference_by_twice_the_bound(cases, terms, name):
    c = cases[name]
    _, _, f, t = BU.edge_grid(1, 1)
    books = [(c["wr"], c["wt"])] + [BU.change_weight(c["wr"], c["wt"], *ctl[1:]) for ctl in c["controls"]]
    assert len(books) >= 2
    refs = BU.beam_direct(terms, NRX, NTX, c["rxe"], c["txe"], books, FA, f, t)
    # the right reference passes its own check, so a failure under a control is the control's
    BU.check_unit(refs[0].astype(np.complex64), refs[0], c["wr"], c["wt"], name)
    for ctl, ref in zip(c["controls"], refs[1:]):
        ratio = _over_bound(ref - refs[0], c)
        print("%s, %s (%s beam %d element %d %s): %.3g times the bound" % ((name,) + ctl + (ratio,)))
        assert ratio >= MARGIN, (name, ctl, ratio)
        with pytest.raises(AssertionError):
            BU.check_unit(refs[0].astype(np.complex64), ref, c["wr"], c["wt"], name)
    if not c["probe"]:
        return
    # one planted record changed: the reference moves by that record's own term (the sum is linear in the terms)
    for what, k in PL.control_records(terms):
        one = PL.select(terms, np.array([k]))
        own, = BU.beam_direct(one, NRX, NTX, c["rxe"], c["txe"], books[:1], FA, f, t)
        swapped, = BU.beam_direct(PL.mutate(one, 0, "swap"), NRX, NTX, c["rxe"], c["txe"], books[:1], FA, f, t)
        for how, d in (("drop", own), ("double", own), ("swap", swapped - own)):
            ratio = _over_bound(d, c)
            print("%s, record %s %s: %.3g times the bound" % (name, what, how, ratio))
            assert ratio >= MARGIN, (name, what, how, ratio)


def test_dense_reference_is_the_contracted_array_channel(cases, terms):
    """case C on its largest grid, with t0 != 0 and an array frequency off the carrier"""
    c = cases["C"]
    T = PL.select(terms, np.arange(terms["rx"].size) % 5 == 0)
    for k, nt in ((17, 3), (16, 17)):
        _, _, f, t = BU.edge_grid(k, nt, 3 * PL.DT)
        ref, = BU.beam_direct(T, NRX, NTX, c["rxe"], c["txe"], [(c["wr"], c["wt"])], 0.75 * FA, f, t)
        H = PL.array_direct(T, NRX, NTX, c["rxe"], c["txe"], 0.75 * FA, f, t)
        want = beams.apply(H, c["wr"].astype(np.complex128), c["wt"].astype(np.complex128))
        assert np.abs(ref - want).max() <= 1e-9 * np.abs(want).max()
