"""The beamformed taps (Tracer.beam_taps) where the index arithmetic of the gain stage and of the tiling can go wrong
(csrc/hrt_beam_taps.hip): the switch between the two forms at Br Bt T = 12 / 13, blocks of 64 rows that cover 1 to 64
beam pairs and begin inside a pair, the RX slots and the two rules for the TX slots at the block's capacity, element
tiles of 32 up to the limit of 256 a side, column tiles and a second column block, l_min < 0, t0 != 0, an array
frequency off the carrier, and links so thin that a chunk stages fewer than 32 records or none at all.

The workspaces are planted (tests/planted.py: integer delays at f_s = PL.FS, so every record has exactly one non-zero
tap and, the delays of a link being distinct, every tap holds at most one record) and the reference is
BT.beam_taps_direct on the planted terms, float64 from the definition.  The cases, their probe codebooks
(BU.probe_weights) and their controls are BT.EDGE_SHAPES / BT.edge_case; tests/test_beam_taps_design.py checks on the
CPU that each case reaches what it is there for and that each control moves the reference by at least twice the
bound.  Bound: BU.UNIT_TOL ||W_rx[a]||_1 ||W_tx[b]||_1 per (link, a, b) over all (pol, m, l) (BU.check_unit).
Negative controls, under each of which the check must fail: the reference's codebook changed in one weight (zeroed, or
moved to the next beam), and one planted record of the window dropped, doubled or moved to the other polarisation."""
import ctypes as C

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import beam_taps_util as BT
from . import beam_util as BU
from . import configs as K
from . import planted as PL
from .pathsum_util import PARTS, _expect_failure, _lam, _thin, _tracer
from .test_gpu_beam_edges import _clear_first_halves, _segments

pytestmark = pytest.mark.gpu

CFG = K.small(K.C3, 2000)   # about 3 000 records per link, several record chunks


def _call(tr, c, los=True, scatter=True, t0=None, fa_scale=None):
    fa = (c["fa_scale"] if fa_scale is None else fa_scale) * tr.f_ghz * 1e9
    return tr.beam_taps(c["rxe"], c["txe"], c["wr"], c["wt"], PL.FS, c["nl"], c["l_min"], fc=PL.FC,
                        t0=c["t0"] if t0 is None else t0, dt=PL.DT, num_times=c["nt"], los=los, scatter=scatter,
                        array_frequency=fa).cpu().numpy()


def _must_fail(got, ref, c, what):
    with pytest.raises(AssertionError):
        BU.check_unit(got, ref, c["wr"], c["wt"], what)
        print("%s: the check passed under the control" % what)


@pytest.fixture(scope="module")
def planted():
    tr = _tracer(CFG)
    tr.trace()
    T = PL.plant(tr)
    assert not PL.design_errors(T), PL.design_errors(T)
    per = np.bincount(PL.link_of(T, tr.ntx), minlength=tr.nrx * tr.ntx)
    assert per.min() > 1000, per
    yield tr, T
    tr.close()


@pytest.mark.parametrize("name", BT.EDGE_NAMES)
def test_case_against_float64_with_controls(planted, name):
    """LoS + scatter: the case, then every control of BT.edge_case against the same output"""
    tr, T = planted
    c = BT.edge_case(name, _lam(CFG))
    fa = tr.f_ghz * 1e9
    books = [(c["wr"], c["wt"])] + [BU.change_weight(c["wr"], c["wt"], *ctl[1:]) for ctl in c["controls"]]
    refs = BT.edge_direct(T, tr.nrx, tr.ntx, c, books, fa)
    got = _call(tr, c)
    assert got.dtype == np.complex64
    worst = BU.check_unit(got, refs[0], c["wr"], c["wt"], name)
    print("beam taps edges %s (%s): max |err| / bound = %.3g" % (name, c["why"], worst))
    # a tap that holds no record of its link is an exact zero
    k = T["n"] - c["l_min"]
    seen = (k >= 0) & (k < c["nl"])
    held = np.zeros((tr.nrx * tr.ntx, c["nl"]), bool)
    held[PL.link_of(T, tr.ntx)[seen], k[seen]] = True
    empty = np.nonzero(~held.reshape(tr.nrx, tr.ntx, c["nl"]))
    assert (got[empty[0], empty[1], ..., empty[2]] == 0).all()
    for ctl, ref in zip(c["controls"], refs[1:]):
        _must_fail(got, ref, c, "%s, %s (%s beam %d element %d %s)" % ((name,) + ctl))
    _expect_failure(lambda U: BU.check_unit(got, BT.edge_direct(U, tr.nrx, tr.ntx, c, books[:1], fa)[0], c["wr"],
                                            c["wt"], name), T, "beam taps edges " + name, BT.window_records(T, c))


@pytest.mark.parametrize("name", ["t3", "t5", "e256", "f12_t3"])
def test_parts_t0_and_array_frequency_are_seen(planted, name):
    """every part (the sum is linear in the terms); the output at another t0 or with the carrier for the array
    frequency fails the check"""
    tr, T = planted
    c = BT.edge_case(name, _lam(CFG))
    fa = tr.f_ghz * 1e9
    books = [(c["wr"], c["wt"])]
    for los, scatter in PARTS:
        Ts = PL.select(T, (T["los"] & los) | (~T["los"] & scatter))
        ref = BT.edge_direct(Ts, tr.nrx, tr.ntx, c, books, fa)[0]
        BU.check_unit(_call(tr, c, los, scatter), ref, c["wr"], c["wt"], "%s %s" % (name, (los, scatter)))
    full = BT.edge_direct(T, tr.nrx, tr.ntx, c, books, fa)[0]
    _must_fail(_call(tr, c, t0=c["t0"] + PL.DT), full, c, name + " at another t0")
    if c["fa_scale"] != 1.0:
        _must_fail(_call(tr, c, fa_scale=1.0), full, c, name + " with f_a = the carrier")


# ------------------------------------------------------------------ thin links
def _nchunks(tr, c):
    """the record chunks of a beam taps call (host/channel.c bt_plan), from its scratch size: seg, the partial sums of
    every chunk, the LoS gains"""
    spec = abi.taps_spec(PL.FS, c["nl"], c["l_min"], PL.FC, 0.0, PL.DT, c["nt"])
    buf = np.zeros(16, np.float32)
    br, bt = c["wr"].shape[0], c["wt"].shape[0]
    arr = abi.ArraySpec(c["rxe"].shape[0], c["txe"].shape[0], buf.ctypes.data, buf.ctypes.data, 3e9)
    bm = abi.BeamSpec(br, bt, buf.ctypes.data, buf.ctypes.data)
    need = C.c_uint64(0)
    assert tr.L.hrt_beam_taps_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(arr), C.byref(bm),
                                            C.byref(need)) == 0
    up = lambda n: (n + 255) // 256 * 256   # noqa: E731
    links = tr.nrx * tr.ntx
    per = links * 2 * br * bt * c["nt"] * c["nl"] * 8
    rest = need.value - up(tr.nb * (tr.ntx + 1) * 4) - up(links * br * bt * 8)
    n = rest // per
    assert n >= 1 and up(n * per) == rest, (need.value, per, rest)
    return n


def _chunk0_terms(tr, T, c, nchunks):
    """[link]: the scatter terms of T inside the window of case c that lie in chunk 0 of their TX segment (chunk_range
    of csrc/hrt_pathsum.h: the first n / nchunks records of a segment of n)"""
    cnt = np.zeros(tr.nrx * tr.ntx, np.int64)
    seg = dict(_segments(tr))
    k = T["n"] - c["l_min"]
    for i in np.nonzero(~T["los"] & (k >= 0) & (k < c["nl"]))[0]:
        s = seg[int(T["bounce"][i])]
        tx = int(T["tx"][i])
        s0, n = int(s[tx]), int(s[tx + 1] - s[tx])
        cnt[int(T["rx"][i]) * tr.ntx + tx] += int(T["index"][i]) < s0 + n // nchunks
    return cnt


def test_thin_links_after_a_dense_call():
    """About 5 unblocked records per link: every chunk stages fewer than 32 records in its only batch, and chunk 0 of
    the links of receiver 0 has none (_clear_first_halves; asserted from the term list).  Its partial sums must be
    written all the same, as zeros: the reduce kernel adds every chunk, and the scratch, cached on the Tracer, holds
    the sums of the dense call of the same shapes made just before -- non-zero in chunk 0 of those links, which is
    asserted too.  Both forms: 5 x 13 beams (<4, 4, 4>) and 3 x 4 beams (<1, 4, 1>)."""
    tr = _tracer(CFG)
    tr.trace()
    dense = PL.plant(tr)
    ws_dense = tr.ws.clone()
    _thin(tr, 5)
    _clear_first_halves(tr, 0)
    T = PL.plant(tr)
    ws_thin = tr.ws.clone()
    assert not PL.design_errors(dense) and not PL.design_errors(T)
    links = tr.nrx * tr.ntx
    per = np.bincount(PL.link_of(T, tr.ntx), minlength=links)
    assert 0 < per.min() and per.max() < 32, per
    fa = tr.f_ghz * 1e9
    for name in ("p65", "f12"):
        c = dict(BT.edge_case(name, _lam(CFG)), nl=1025, l_min=0)   # a window over every thin record, a third of the dense ones
        books = [(c["wr"], c["wt"])]
        nchunks = _nchunks(tr, c)
        assert nchunks >= 2, nchunks
        assert int(T["n"].max()) < c["nl"]
        tr.ws.copy_(ws_dense)
        assert (_chunk0_terms(tr, dense, c, nchunks)[:tr.ntx] > 0).all()
        got = _call(tr, c)
        BU.check_unit(got, BT.edge_direct(dense, tr.nrx, tr.ntx, c, books, fa)[0], c["wr"], c["wt"], name + " dense")
        scratch = tr._bt_scratch

        tr.ws.copy_(ws_thin)
        scat = np.bincount(PL.link_of(T, tr.ntx)[~T["los"]], minlength=links)
        assert (_chunk0_terms(tr, T, c, nchunks)[:tr.ntx] == 0).all() and (scat[:tr.ntx] > 0).all(), scat
        got = _call(tr, c)
        assert tr._bt_scratch.data_ptr() == scratch.data_ptr()   # the dense call's partial sums were in it
        worst = BU.check_unit(got, BT.edge_direct(T, tr.nrx, tr.ntx, c, books, fa)[0], c["wr"], c["wt"], name + " thin")
        print("beam taps edges thin %s: max |err| / bound = %.3g" % (name, worst))
        s = np.nonzero(~T["los"])[0]
        records = [("receiver 0", int(s[T["rx"][s] == 0][0])), ("last", int(s[-1]))]
        _expect_failure(lambda U: BU.check_unit(got, BT.edge_direct(U, tr.nrx, tr.ntx, c, books, fa)[0], c["wr"],
                                                c["wt"], name), T, "beam taps edges thin " + name, records)
    tr.close()
