"""The beamformed channel (Tracer.beam_channel) where the index arithmetic of its S stage can go wrong
(csrc/hrt_beam_channel.hip): the RX slots of a pair block up to all 32, the two rules for its TX slots at Bt = 31, 32,
33, 40 and 256, element tiles of 32 up to the limit of 256 on either side and on both, t0 != 0, an array frequency off
the carrier, two column blocks, and links so thin that a chunk stages fewer than 32 records or none at all.

The workspaces are planted (tests/planted.py) and the reference is BU.beam_direct on the planted terms, float64 from
the definition.  The cases, their codebooks and their controls are BU.edge_cases; tests/test_beam_edges_design.py
checks on the CPU that each case reaches what it is there for and that each control moves the reference by at least
twice the bound.  Bound: that of tests/test_gpu_beam_planted.py, UNIT_TOL ||W_rx[a]||_1 ||W_tx[b]||_1 per (link, a, b)
over all (pol, m, k) (BU.check_unit).  Negative controls, under each of which the check must fail: the reference's
codebook changed in one weight (zeroed, or moved to the next beam) and, where a codebook has single-weight beams, one
planted record dropped, doubled or moved to the other polarisation."""
import numpy as np
import pytest

from . import beam_util as BU
from . import configs as K
from . import planted as PL
from .pathsum_util import PARTS, _expect_failure, _lam, _thin, _tracer

pytestmark = pytest.mark.gpu

CFG = K.small(K.C3, 2000)   # about 3 000 records per link, several record chunks
T0 = 3 * PL.DT
GRIDS = [("C", 17, 3), ("C", 16, 17), ("E", 17, 3)]   # (16, 17): 17 rows, so two column blocks with four pair blocks


def _sel(T, los, scatter):
    return PL.select(T, (T["los"] & los) | (~T["los"] & scatter))


def _call(tr, c, k, nt, t0=0.0, fa=None, los=True, scatter=True):
    f0, df, _, _ = BU.edge_grid(k, nt, t0)
    return tr.beam_channel(c["rxe"], c["txe"], c["wr"], c["wt"], f0, df, k, t0, PL.DT, nt, los=los, scatter=scatter,
                           array_frequency=fa).cpu().numpy()


def _direct(tr, T, c, books, k, nt, t0=0.0, fa=None):
    _, _, f, t = BU.edge_grid(k, nt, t0)
    return BU.beam_direct(T, tr.nrx, tr.ntx, c["rxe"], c["txe"], books, tr.f_ghz * 1e9 if fa is None else fa, f, t)


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
    yield tr, T, BU.edge_cases(_lam(CFG))
    tr.close()


@pytest.mark.parametrize("name", ["A", "B", "C", "D32", "D31", "E", "F"])
def test_case_against_float64_with_controls(planted, name):
    """(K, T) = (1, 1), LoS + scatter: the case, then every control of BU.edge_cases against the same output"""
    tr, T, cases = planted
    c = cases[name]
    books = [(c["wr"], c["wt"])] + [BU.change_weight(c["wr"], c["wt"], *ctl[1:]) for ctl in c["controls"]]
    refs = _direct(tr, T, c, books, 1, 1)
    got = _call(tr, c, 1, 1)
    worst = BU.check_unit(got, refs[0], c["wr"], c["wt"], name)
    print("beam edges %s (1, 1): max |err| / bound = %.3g" % (name, worst))
    for ctl, ref in zip(c["controls"], refs[1:]):
        _must_fail(got, ref, c, "%s, %s (%s beam %d element %d %s)" % ((name,) + ctl))
    if c["probe"]:
        _expect_failure(lambda U: BU.check_unit(got, _direct(tr, U, c, books[:1], 1, 1)[0], c["wr"], c["wt"], name), T,
                        "beam edges " + name)


@pytest.mark.parametrize("name,k,nt", GRIDS, ids=["%s_%dx%d" % g for g in GRIDS])
def test_grids_parts_t0_and_array_frequency(planted, name, k, nt):
    """every part at t0 = 3 dt with the array frequency at 0.75 of the carrier (the sum is linear in the terms: the
    reference of LoS + scatter is the sum of the two parts' references)"""
    tr, T, cases = planted
    c = cases[name]
    fa = 0.75 * tr.f_ghz * 1e9
    books = [(c["wr"], c["wt"])]
    ref = {(True, False): _direct(tr, _sel(T, True, False), c, books, k, nt, T0, fa)[0],
           (False, True): _direct(tr, _sel(T, False, True), c, books, k, nt, T0, fa)[0]}
    ref[(True, True)] = ref[(True, False)] + ref[(False, True)]
    for parts in PARTS:
        got = _call(tr, c, k, nt, T0, fa, *parts)
        worst = BU.check_unit(got, ref[parts], c["wr"], c["wt"], "%s (%d, %d) %s" % (name, k, nt, parts))
        print("beam edges %s (%d, %d) %s: max |err| / bound = %.3g" % (name, k, nt, parts, worst))
    # the arguments are seen: the output at t0 = 0, or with the carrier for the array frequency, fails this check
    full = ref[(True, True)]
    _must_fail(_call(tr, c, k, nt, 0.0, fa), full, c, "%s (%d, %d) with t0 = 0" % (name, k, nt))
    _must_fail(_call(tr, c, k, nt, T0, None), full, c, "%s (%d, %d) with f_a = the carrier" % (name, k, nt))


# ------------------------------------------------------------------ thin links
def _segments(tr):
    """[(block, [first hit of TX segment t, t <= ntx])] of the last trace"""
    counts = tr.counts()
    out = []
    for b in range(tr.nb):
        n = int(counts[b + 1])
        if n == 0:
            continue
        ray = tr.hit_block(b)[PL.HIT_RAY, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        tx, _ = tr.global_path(ray)
        assert (np.diff(tx) >= 0).all()
        out.append((b, np.searchsorted(tx, np.arange(tr.ntx + 1))))
    return out


def _clear_first_halves(tr, rx):
    """clear the unblocked bits of receiver rx in the first half of every TX segment of every block: with two chunks
    or more, chunk 0 of every link of rx is then empty (chunk 0 of a segment of n records is its first n / nchunks)"""
    torch = tr.torch
    for b, seg in _segments(tr):
        m = tr.mask_block(b).view(torch.int64)
        row = m[rx].cpu().numpy().view(np.uint64).copy()
        for t in range(tr.ntx):
            s0, n = int(seg[t]), int(seg[t + 1] - seg[t])
            for i in range(s0, s0 + n // 2):
                row[i >> 6] &= ~(np.uint64(1) << np.uint64(i & 63))
        m[rx] = torch.from_numpy(row.view(np.int64)).to(tr.device)
    torch.cuda.synchronize(tr.device)


def _first_half_terms(tr, T):
    """[link]: the scatter terms of T in the first half of their TX segment (chunk_range of csrc/hrt_pathsum.h: chunk 0
    of a segment of n records is its first n / nchunks, within the first half for two chunks or more)"""
    cnt = np.zeros(tr.nrx * tr.ntx, np.int64)
    seg = dict(_segments(tr))
    for k in np.nonzero(~T["los"])[0]:
        s = seg[int(T["bounce"][k])]
        tx = int(T["tx"][k])
        s0, n = int(s[tx]), int(s[tx + 1] - s[tx])
        cnt[int(T["rx"][k]) * tr.ntx + tx] += int(T["index"][k]) < s0 + n // 2
    return cnt


def test_thin_links_after_a_dense_call():
    """About 5 unblocked records per link: every chunk stages fewer than 32 records in its only batch, and chunk 0 of
    the links of receiver 0 has none: with two chunks or more, which the scratch size shows, chunk 0 lies in the first
    half of its segment, where _clear_first_halves leaves receiver 0 no record (asserted from the term list below).  Its partial sums must
    be written all the same, as zeros: the reduce kernel adds every chunk, and the scratch, cached on the Tracer, holds
    the sums of the dense call of the same shapes made just before."""
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
    lam = _lam(CFG)
    c35 = dict(rxe=np.array([[0, 0, 0], [0, lam / 2, 0]], np.float32),
               txe=np.array([[0, 0, 0], [lam / 2, 0, lam / 3], [0, lam / 4, lam / 2]], np.float32))
    c35["wr"], c35["wt"] = BU.planted_codebooks(2, 3)
    # receiver 0's links have records, none of them in the first half of a segment; a dense link has many there
    scat = np.bincount(PL.link_of(T, tr.ntx)[~T["los"]], minlength=links)
    assert (_first_half_terms(tr, T)[:tr.ntx] == 0).all() and (scat[:tr.ntx] > 0).all(), scat
    assert (_first_half_terms(tr, dense) > 32).all()
    first = True
    for name, c in (("C", BU.edge_cases(lam)["C"]), ("3x5", c35)):
        books = [(c["wr"], c["wt"])]

        tr.ws.copy_(ws_dense)
        got = _call(tr, c, 1, 1)
        BU.check_unit(got, _direct(tr, dense, c, books, 1, 1)[0], c["wr"], c["wt"], name + " dense")
        scratch = tr._bm_scratch
        if first:   # a fresh Tracer's scratch is what this call asked for: room for the partial sums of two chunks or
            # more, each the size of the output (the TX segments and the LoS gains beside them are smaller than one)
            assert scratch.numel() >= 2 * got.nbytes, (scratch.numel(), got.nbytes)
            first = False

        tr.ws.copy_(ws_thin)
        got = _call(tr, c, 1, 1)
        assert tr._bm_scratch.data_ptr() == scratch.data_ptr()   # the dense call's partial sums were in it
        worst = BU.check_unit(got, _direct(tr, T, c, books, 1, 1)[0], c["wr"], c["wt"], name + " thin")
        print("beam edges thin %s: max |err| / bound = %.3g" % (name, worst))
        # one record of a link of receiver 0 (an empty chunk beside it), and the last record of the last block (the
        # terms stand block by block, receiver by receiver, the LoS terms behind them)
        scat = np.nonzero(~T["los"])[0]
        records = [("receiver 0", int(scat[T["rx"][scat] == 0][0])), ("last", int(scat[-1]))]
        _expect_failure(lambda U: BU.check_unit(got, _direct(tr, U, c, books, 1, 1)[0], c["wr"], c["wt"], name), T,
                        "beam edges thin " + name, records)
    tr.close()
