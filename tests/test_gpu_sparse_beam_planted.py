"""Tracer.sparse_beam_channel (csrc/hrt_sparse_beam.hip) on planted lists and planted codebooks, at tolerance 0: the
exact planting of tests/sparse_beam_util.py (every output a Gaussian integer whose intermediates stay below 2^24, proved
without a device in tests/test_sparse_beam_design.py) compared value for value over the batch edge, the largest list,
the beam-pair tile and block, the TX beam slots, the element tiles, the inner length and the column block, several links
with different `kept`, one-hot lists and one-hot codebooks; then what must not reach the output (slots at or beyond
kept, another link's non-finite fields), accumulate, and the repeatability of the bytes.  No trace is needed: the tracer
is only the handle of the device."""
import numpy as np
import pytest

from . import configs as K
from . import sparse_beam_util as U
from .pathsum_util import _bits, _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))
    yield t
    t.close()


def _run(tr, v, re, te, wr, wt, nk, nt, **kw):
    return tr.sparse_beam_channel(v, re, te, wr, wt, U.F0, U.DF, nk, U.T0, U.DT, nt, array_frequency=U.F_A, **kw)


def _check(tr, name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    B = _run(tr, v, re, te, wr, wt, c["nk"], c["nt_"])
    assert tuple(B.shape) == (c["nrx"], c["ntx"], c["br"], c["bt"], 2, c["nt_"], c["nk"])
    E = U.exact_reference(v, re, te, wr, wt, c["nk"], c["nt_"])
    U.check_exact(B.cpu().numpy(), E, name)
    return B, E, (v, re, te, wr, wt)


@pytest.mark.parametrize("k", [1, 31, 32, 33, 1024])
def test_full_lists_over_the_batch_edge_and_the_largest_list(tr, k):
    _, E, _ = _check(tr, "K%d" % k)
    assert np.abs(E).max() >= 1


def test_the_largest_list_with_sparse_codebooks_over_two_and_three_element_tiles(tr):
    _, E, _ = _check(tr, "K1024_sparse")
    assert E.any(axis=(4, 5, 6)).all()


@pytest.mark.parametrize("kept", [0, 1, 32])
def test_kept_below_the_list_length(tr, kept):
    _, E, _ = _check(tr, "kept%d" % kept)
    assert bool(E.any()) == (kept > 0)


@pytest.mark.parametrize("br,bt", [(1, 1), (1, 31), (4, 8), (3, 11)])
def test_beam_pair_tile_and_block_edges(tr, br, bt):
    """Br Bt = 1, 31, 32, 33"""
    _check(tr, "pairs%dx%d" % (br, bt))


@pytest.mark.parametrize("name", ["bt31", "bt32", "bt33", "bt40", "bt256", "br256"])
def test_beam_slot_edges(tr, name):
    """Bt <= 32: TX slot s is beam s; Bt > 32: the beam of pair p0 + s, wrapping inside a block; Br = 256: 32 RX slots"""
    _, E, _ = _check(tr, name)
    assert E.any(axis=(0, 1, 4, 5, 6)).all()     # every beam pair is hit


def test_four_pair_blocks_with_two_column_blocks(tr):
    _check(tr, "bt40_br3")


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 256])
@pytest.mark.parametrize("side", ["rx", "tx", "both"])
def test_element_tile_edges(tr, side, n):
    _check(tr, "%s%d" % (side, n))


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("nk", [1, 15, 16, 17, 256, 257])
def test_inner_length_and_column_block_edges(tr, nk, nt):
    _check(tr, "grid%dx%d" % (nk, nt))


def test_five_links_with_different_kept_and_the_wrong_readings(tr):
    B, E, (v, re, te, wr, wt) = _check(tr, "links5")
    assert not E[0, 0].any() and E[0, 1:].any(axis=(1, 2, 3, 4, 5)).all()
    # the device result is none of the wrong readings (tests/test_sparse_beam_design.py)
    got = B.cpu().numpy()
    differ = 0
    for name in U.MUTANTS:
        W = U.mutant(name, v, re, te, wr, wt, 17, 3)
        if not np.array_equal(W, E):
            differ += 1
            with pytest.raises(AssertionError):
                U.check_exact(got, W, name)
    assert differ >= 8


@pytest.mark.parametrize("name", ["bt40_br3", "both33"])
def test_the_slot_and_tile_readings_on_their_own_cases(tr, name):
    """the TX slot, a0 and element tile readings differ from the truth only where Bt > 32 or a side has two tiles"""
    B, E, (v, re, te, wr, wt) = _check(tr, name)
    c = U.CASES[name]
    got = B.cpu().numpy()
    for m in ("tx_slot_is_beam", "a0_rounded_up") if name == "bt40_br3" else ("last_element_tile_only",):
        W = U.mutant(m, v, re, te, wr, wt, c["nk"], c["nt_"])
        assert not np.array_equal(W, E), m
        with pytest.raises(AssertionError):
            U.check_exact(got, W, m)


def test_one_hot_lists_and_one_hot_codebooks_hit_every_index_once(tr):
    """one live slot with one nonzero amplitude component, one non-zero weight a side: every (link, a, b, pol, m, k) of
    2 x 3 beams, T = 2, K_f = 17 is hit by its own case and by no other"""
    nk, nt = 17, 2
    re, te = U.elements(2, 3)
    hit = np.zeros((1, 3, 2, 3, 2, nt, nk), np.int64)
    for link in range(3):
        for comp in range(4):
            v = U.one_hot(1, 3, link, comp, salt=link)
            for a in range(2):
                for b in range(3):
                    wr = U.one_hot_codebook(2, 2, a, (a + comp) % 2, 1 + 2j)
                    wt = U.one_hot_codebook(3, 3, b, (b + link) % 3, 2 - 1j)
                    B = _run(tr, v, re, te, wr, wt, nk, nt).cpu().numpy()
                    U.check_exact(B, U.exact_reference(v, re, te, wr, wt, nk, nt), ("one hot", link, comp, a, b))
                    hit += (B != 0)
    assert (hit == 2).all()     # the re and the im component of its polarisation, nothing else


def _poisoned(v, kept_header=None):
    """v with 0xFF bytes (NaN floats) in every slot at or beyond kept, and optionally another header word"""
    w = U.copy(v)
    nrx, ntx, k = w["tau"].shape
    recs = w["buffer"][16 * nrx * ntx:].reshape(nrx, ntx, k, 72)
    dead = np.arange(k) >= np.minimum(w["kept"], np.uint64(k)).astype(np.int64)[..., None]
    recs[dead] = 0xFF
    if kept_header is not None:
        w["kept"][...] = kept_header
    return w


def _arrays(nr=4, nt=5, br=3, bt=5, salt=4):
    re, te = U.elements(nr, nt)
    return re, te, U.codebook(br, nr, 0, salt=salt), U.codebook(bt, nt, 1, salt=salt)


def test_slots_at_or_beyond_kept_do_not_reach_the_output(tr):
    A = _arrays()
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]], salt=4)
    clean = _run(tr, v, *A, 17, 2)
    w = _poisoned(v)
    assert np.isnan(w["tau"][0, 0]).all() and np.isnan(w["a_te"][0, 1, 1:]).all() and not np.isnan(w["tau"][1, 0]).any()
    assert tr.torch.equal(_bits(_run(tr, w, *A, 17, 2)), _bits(clean))
    U.check_exact(clean.cpu().numpy(), U.exact_reference(v, *A, 17, 2), "clean")
    # kept > K in the header: min(kept, K) slots are read
    full = U.planted(2, 3, 33, 33, salt=4)
    over = U.copy(full)
    over["kept"][...] = np.array([[34, 1 << 20, 1 << 40], [(1 << 64) - 1, 33, 1 << 32]], np.uint64)
    assert tr.torch.equal(_bits(_run(tr, over, *A, 17, 2)), _bits(_run(tr, full, *A, 17, 2)))


def test_non_finite_fields_stay_within_their_link(tr):
    A = _arrays(salt=6)
    v = U.planted(2, 3, 33, [[33, 1, 32], [33, 7, 31]], salt=6)
    clean = _run(tr, v, *A, 17, 2)
    w = U.copy(v)
    w["a_te"][0, 0, 5] = np.nan
    w["tau"][0, 0, 17] = np.inf
    w["u_rx"][0, 0, 32, 1] = np.nan
    bad = _run(tr, w, *A, 17, 2)
    assert tr.torch.equal(_bits(bad[0, 1:]), _bits(clean[0, 1:])) and tr.torch.equal(_bits(bad[1]), _bits(clean[1]))
    assert bool(tr.torch.isnan(tr.torch.view_as_real(bad[0, 0])).any())


def test_accumulate_and_repeatability(tr):
    torch = tr.torch
    A = _arrays(salt=8)
    v = U.planted(1, 3, 64, [[64, 0, 31]], salt=8)
    a = _run(tr, v, *A, 33, 2)
    b = _run(tr, v, *A, 33, 2)
    assert torch.equal(_bits(a), _bits(b))                       # two calls: identical bytes
    U.check_exact(a.cpu().numpy(), U.exact_reference(v, *A, 33, 2), "accumulate base")
    # every byte is written: a NaN-filled `out` holds no NaN afterwards and the same bytes
    out = torch.full_like(a, complex(float("nan"), float("nan")))
    assert _run(tr, v, *A, 33, 2, out=out) is out and torch.equal(_bits(out), _bits(a))
    # accumulate doubles the result bit for bit; the link with n = 0 stays as it was, bit for bit
    out = a.clone()
    out[0, 1] = complex(-0.0, 7.5)
    _run(tr, v, *A, 33, 2, out=out, accumulate=True)
    want = a + a
    want[0, 1] = complex(-0.0, 7.5)
    assert torch.equal(_bits(out), _bits(want))
    with pytest.raises(ValueError, match="accumulate=True needs `out`"):
        _run(tr, v, *A, 33, 2, accumulate=True)
    with pytest.raises(ValueError, match="out must be a contiguous complex64 tensor"):
        _run(tr, v, *A, 33, 2, out=out[:, :2])


def test_device_buffer_and_numpy_upload_give_the_same_bytes(tr):
    """a result dict of device tensors (what dominant_paths() returns) is read where it is; torch codebooks are taken"""
    from hermespy_rt_amd import abi
    re, te, wr, wt = _arrays(2, 3, 2, 3, salt=2)
    v = U.planted(2, 2, 7, [[7, 3], [0, 5]], salt=2)
    d = abi.dominant_views(tr.torch.from_numpy(v["buffer"]).to(tr.device), 2, 2, 7)
    a, b = _run(tr, v, re, te, wr, wt, 17, 2), _run(tr, d, re, te, wr, wt, 17, 2)
    assert tr.torch.equal(_bits(a), _bits(b))
    c = _run(tr, v, re, te, tr.torch.from_numpy(wr).to(tr.device), tr.torch.from_numpy(wt), 17, 2)
    assert tr.torch.equal(_bits(a), _bits(c))


def test_tracer_refuses_what_is_its_own_to_refuse_and_passes_on_the_library_s_refusals(tr):
    from hermespy_rt_amd.device import Tracer
    t = Tracer.__new__(Tracer)          # (the checks read these attributes only; tr stays the owner of the device)
    t.torch, t.device, t.nrx, t.ntx, t.f_ghz = tr.torch, tr.device, 2, 3, tr.f_ghz
    t.L = tr.L
    U.tracer_value_errors(t)
    v = U.planted(2, 3, 8, 5)
    el, w = U.elements(2, 2), (U.codebook(2, 2, 0), U.codebook(3, 2, 1))
    a = t.sparse_beam_channel(v, *el, *w, U.F0, U.DF, 4)
    assert tr.torch.equal(_bits(t.sparse_beam_channel(v["buffer"], *el, *w, U.F0, U.DF, 4)), _bits(a))
    with pytest.raises(ValueError, match="hrt_sparse_beam_channel: .*array frequency"):
        t.sparse_beam_channel(v, *el, *w, U.F0, U.DF, 4, array_frequency=-1.0)
    with pytest.raises(ValueError, match="hrt_sparse_beam_channel: .*num_freqs"):
        t.sparse_beam_channel(v, *el, *w, U.F0, U.DF, 0)
    with pytest.raises(ValueError, match=r"hrt_sparse_beam_channel: .*2\^24"):     # (refused before any allocation)
        t.sparse_beam_channel(v, *U.elements(1, 1), np.ones((64, 1), np.complex64), np.ones((16, 1), np.complex64),
                              U.F0, U.DF, 129, num_times=128)
    with pytest.raises(ValueError, match="hrt_sparse_beam_channel: .*257 RX"):
        t.sparse_beam_channel(v, np.zeros((257, 3), np.float32), np.zeros((1, 3), np.float32),
                              np.ones((1, 257), np.complex64), np.ones((1, 1), np.complex64), U.F0, U.DF, 4)
    with pytest.raises(ValueError, match="hrt_sparse_beam_channel: .*1 RX and 257 TX beams"):
        t.sparse_beam_channel(v, *U.elements(1, 1), np.ones((1, 1), np.complex64), np.ones((257, 1), np.complex64),
                              U.F0, U.DF, 4)
