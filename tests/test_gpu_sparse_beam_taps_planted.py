"""Tracer.sparse_beam_taps (csrc/hrt_sparse_beam_taps.hip) on planted lists and planted codebooks, at tolerance 0: the
exact planting of tests/sparse_beam_taps_util.py (every output a Gaussian integer whose intermediates stay below 2^24,
proved without a device in tests/test_sparse_beam_taps_design.py) compared value for value over the 4-slot MFMA step and
the batch edge, the largest list, the switch between the two forms of the kernel, the row-block edges (with blocks that
begin inside a pair), the RX and TX beam slots, the element tiles, the column tile and column block of both forms, tap
windows left of, at and right of zero, several links with different `kept`, one-hot lists and one-hot codebooks; then
what must not reach the output (slots at or beyond kept, another link's non-finite fields), accumulate, the
repeatability of the bytes, and the sinc weights at off-grid delays.  No trace is needed: the tracer is only the handle
of the device."""
import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import configs as K
from . import sparse_beam_taps_util as U
from .pathsum_util import _bits, _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))
    yield t
    t.close()


def _run(tr, v, re, te, wr, wt, l_min, L, nt, **kw):
    return tr.sparse_beam_taps(v, re, te, wr, wt, U.FS, L, l_min, U.FC, U.T0, U.DT, nt, array_frequency=U.F_A, **kw)


def _check(tr, name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    h = _run(tr, v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
    assert tuple(h.shape) == (c["nrx"], c["ntx"], c["br"], c["bt"], 2, c["T"], c["L"])
    E = U.exact_reference(v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
    U.check_exact(h.cpu().numpy(), E, name)
    return h, E, (v, re, te, wr, wt)


@pytest.mark.parametrize("form", ["rt1", "rt4"])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 31, 32, 33, 1024])
def test_full_lists_over_the_mfma_step_the_batch_edge_and_the_largest_list(tr, k, form):
    _, E, _ = _check(tr, "K%d_%s" % (k, form))
    assert np.abs(E).max() >= 1


def test_the_largest_list_with_sparse_codebooks_over_two_and_three_element_tiles(tr):
    _, E, _ = _check(tr, "K1024_sparse")
    assert E.any(axis=(4, 5, 6)).all()


@pytest.mark.parametrize("form", ["rt1", "rt4"])
@pytest.mark.parametrize("kept", [0, 1, 32])
def test_kept_below_the_list_length(tr, kept, form):
    _, E, _ = _check(tr, "kept%d_%s" % (kept, form))
    assert bool(E.any()) == (kept > 0)


@pytest.mark.parametrize("br,bt,nt", [(2, 3, 2), (13, 1, 1), (4, 1, 3), (1, 13, 1), (1, 1, 1), (1, 1, 13)])
def test_the_switch_between_the_two_forms(tr, br, bt, nt):
    """Br Bt T = 12 (three row tiles: 1 x 4 tiles a wave) and 13 (four: 4 x 4 tiles a wave), and the smallest grid"""
    _check(tr, "form%dx%dx%d" % (br, bt, nt))


@pytest.mark.parametrize("br,bt,nt", [(7, 9, 1), (8, 8, 1), (5, 13, 1), (10, 13, 1), (3, 7, 3), (2, 11, 3)])
def test_row_block_edges(tr, br, bt, nt):
    """63, 64, 65 and 130 pairs with T = 1; 63 and 66 rows with T = 3 (the second block begins at time 1 of pair 21)"""
    _check(tr, "rows%dx%dx%d" % (br, bt, nt))


@pytest.mark.parametrize("name", ["T64", "T65"])
def test_a_pair_that_fills_a_block_and_blocks_that_begin_inside_a_pair(tr, name):
    _check(tr, name)


@pytest.mark.parametrize("name", ["br65", "bt63", "bt64", "bt65", "bt256", "br256", "bt65_T3"])
def test_beam_slot_edges(tr, name):
    """Bt <= 64: TX slot s is beam s; Bt > 64: the beam of pair pf + s; Br = 65 and 256: 64 RX slots a block"""
    _, E, _ = _check(tr, name)
    assert E.any(axis=(0, 1, 4, 5, 6)).all()     # every beam pair is hit


def test_the_tx_beam_wraps_inside_a_block_and_the_slot_readings_differ_there(tr):
    """Bt = 65 with three RX beams: four row blocks x two column blocks; the TX slot and a0 readings differ from the
    truth there and the device result is neither"""
    h, E, (v, re, te, wr, wt) = _check(tr, "bt65_wrap")
    c = U.CASES["bt65_wrap"]
    got = h.cpu().numpy()
    for m in ("tx_slot_is_beam", "a0_rounded_up"):
        W = U.mutant(m, v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
        assert not np.array_equal(W, E), m
        with pytest.raises(AssertionError):
            U.check_exact(got, W, m)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64, 256])
@pytest.mark.parametrize("side", ["rx", "tx", "both"])
def test_element_tile_edges(tr, side, n):
    h, E, (v, re, te, wr, wt) = _check(tr, "%s%d" % (side, n))
    if (side, n) == ("both", 33):     # the element tile reading differs only where a side has two tiles
        c = U.CASES["both33"]
        W = U.mutant("last_element_tile_only", v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
        assert not np.array_equal(W, E)
        with pytest.raises(AssertionError):
            U.check_exact(h.cpu().numpy(), W, "last_element_tile_only")


@pytest.mark.parametrize("l_min", [-70, 0, 9])
@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64, 65])
def test_column_tile_and_column_block_edges_of_the_four_tile_form(tr, L, l_min):
    """the planted delays include l_min - 1 and l_min + L, one tap outside the window on either side"""
    _check(tr, "taps%d_%d" % (L, l_min))


@pytest.mark.parametrize("L", [255, 256, 257])
def test_column_tile_and_column_block_edges_of_the_one_tile_form(tr, L):
    _check(tr, "taps%d_rt1" % L)


@pytest.mark.parametrize("name", ["links5", "links5_rt1"])
def test_five_links_with_different_kept_and_the_wrong_readings(tr, name):
    h, E, (v, re, te, wr, wt) = _check(tr, name)
    c = U.CASES[name]
    assert not E[0, 0].any() and E[0, 1:].any(axis=(1, 2, 3, 4, 5)).all()
    # the device result is none of the wrong readings (tests/test_sparse_beam_taps_design.py)
    got = h.cpu().numpy()
    differ = 0
    for m in U.MUTANTS:
        W = U.mutant(m, v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
        if not np.array_equal(W, E):
            differ += 1
            with pytest.raises(AssertionError):
                U.check_exact(got, W, m)
    assert differ >= 12


def test_one_hot_lists_and_one_hot_codebooks_hit_every_index_once(tr):
    """one live slot with one nonzero amplitude component at one tap, one non-zero weight a side: every (link, a, b,
    pol, m, l) of 2 x 3 beams, T = 2, L = 3 is hit by its own case and by no other"""
    l_min, L, nt = -1, 3, 2
    re, te = U.elements(2, 3)
    hit = np.zeros((1, 3, 2, 3, 2, nt, L), np.int64)
    for link in range(3):
        for comp in range(4):
            for k in range(L):
                v = U.one_hot(1, 3, link, comp, l_min + k, salt=link)
                for a in range(2):
                    for b in range(3):
                        wr = U.one_hot_codebook(2, 2, a, (a + comp) % 2, 1 + 2j)
                        wt = U.one_hot_codebook(3, 3, b, (b + k) % 3, 2 - 1j)
                        h = _run(tr, v, re, te, wr, wt, l_min, L, nt).cpu().numpy()
                        U.check_exact(h, U.exact_reference(v, re, te, wr, wt, l_min, L, nt),
                                      ("one hot", link, comp, k, a, b))
                        hit += (h != 0)
    assert (hit == 2).all()     # the re and the im component of its polarisation at its tap, nothing else


def _poisoned(v):
    """v with 0xFF bytes (NaN floats) in every slot at or beyond kept"""
    w = U.copy(v)
    nrx, ntx, k = w["tau"].shape
    recs = w["buffer"][16 * nrx * ntx:].reshape(nrx, ntx, k, 72)
    dead = np.arange(k) >= np.minimum(w["kept"], np.uint64(k)).astype(np.int64)[..., None]
    recs[dead] = 0xFF
    return w


FORMS = {"rt1": (2, 3, 2, 3), "rt4": (4, 5, 3, 5)}     # nr, nt, br, bt with T = 2: 12 and 30 rows
L_MIN, L, NT = -3, 17, 2


def _arrays(form, salt):
    nr, nt, br, bt = FORMS[form]
    re, te = U.elements(nr, nt)
    return re, te, U.codebook(br, nr, 0, salt=salt), U.codebook(bt, nt, 1, salt=salt)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_slots_at_or_beyond_kept_do_not_reach_the_output(tr, form):
    A = _arrays(form, 4)
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]], L_MIN, L, salt=4)
    clean = _run(tr, v, *A, L_MIN, L, NT)
    w = _poisoned(v)
    assert np.isnan(w["tau"][0, 0]).all() and np.isnan(w["a_te"][0, 1, 1:]).all() and not np.isnan(w["tau"][1, 0]).any()
    assert tr.torch.equal(_bits(_run(tr, w, *A, L_MIN, L, NT)), _bits(clean))
    U.check_exact(clean.cpu().numpy(), U.exact_reference(v, *A, L_MIN, L, NT), "clean")
    # kept > K in the header: min(kept, K) slots are read
    full = U.planted(2, 3, 33, 33, L_MIN, L, salt=4)
    over = U.copy(full)
    over["kept"][...] = np.array([[34, 1 << 20, 1 << 40], [(1 << 64) - 1, 33, 1 << 32]], np.uint64)
    assert tr.torch.equal(_bits(_run(tr, over, *A, L_MIN, L, NT)), _bits(_run(tr, full, *A, L_MIN, L, NT)))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_non_finite_fields_stay_within_their_link(tr, form):
    A = _arrays(form, 6)
    v = U.planted(2, 3, 33, [[33, 1, 32], [33, 7, 31]], L_MIN, L, salt=6)
    clean = _run(tr, v, *A, L_MIN, L, NT)
    w = U.copy(v)
    w["a_te"][0, 0, 5] = np.nan
    w["tau"][0, 0, 17] = np.inf
    w["u_rx"][0, 0, 32, 1] = np.nan
    bad = _run(tr, w, *A, L_MIN, L, NT)
    assert tr.torch.equal(_bits(bad[0, 1:]), _bits(clean[0, 1:])) and tr.torch.equal(_bits(bad[1]), _bits(clean[1]))
    assert bool(tr.torch.isnan(tr.torch.view_as_real(bad[0, 0])).any())


@pytest.mark.parametrize("form", sorted(FORMS))
def test_accumulate_and_repeatability(tr, form):
    torch = tr.torch
    A = _arrays(form, 8)
    v = U.planted(1, 3, 64, [[64, 0, 31]], L_MIN, 33, salt=8)
    a = _run(tr, v, *A, L_MIN, 33, NT)
    b = _run(tr, v, *A, L_MIN, 33, NT)
    assert torch.equal(_bits(a), _bits(b)) and float(a.abs().max()) >= 1      # two calls: identical bytes
    U.check_exact(a.cpu().numpy(), U.exact_reference(v, *A, L_MIN, 33, NT), "accumulate base")
    # every byte is written: a NaN-filled `out` holds no NaN afterwards and the same bytes
    out = torch.full_like(a, complex(float("nan"), float("nan")))
    assert _run(tr, v, *A, L_MIN, 33, NT, out=out) is out and torch.equal(_bits(out), _bits(a))
    # accumulate doubles the result bit for bit; the link with n = 0 stays as it was, bit for bit
    out = a.clone()
    out[0, 1] = complex(-0.0, 7.5)
    _run(tr, v, *A, L_MIN, 33, NT, out=out, accumulate=True)
    want = a + a
    want[0, 1] = complex(-0.0, 7.5)
    assert torch.equal(_bits(out), _bits(want))
    with pytest.raises(ValueError, match="accumulate=True needs `out`"):
        _run(tr, v, *A, L_MIN, 33, NT, accumulate=True)
    with pytest.raises(ValueError, match="out must be a contiguous complex64 tensor"):
        _run(tr, v, *A, L_MIN, 33, NT, out=out[:, :2])


def test_device_buffer_and_numpy_upload_give_the_same_bytes(tr):
    """a result dict of device tensors (what dominant_paths() returns) is read where it is; torch codebooks are taken"""
    from hermespy_rt_amd import abi
    re, te, wr, wt = _arrays("rt1", 2)
    v = U.planted(2, 2, 7, [[7, 3], [0, 5]], L_MIN, L, salt=2)
    d = abi.dominant_views(tr.torch.from_numpy(v["buffer"]).to(tr.device), 2, 2, 7)
    a, b = _run(tr, v, re, te, wr, wt, L_MIN, L, NT), _run(tr, d, re, te, wr, wt, L_MIN, L, NT)
    assert tr.torch.equal(_bits(a), _bits(b))
    c = _run(tr, v, re, te, tr.torch.from_numpy(wr).to(tr.device), tr.torch.from_numpy(wt), L_MIN, L, NT)
    assert tr.torch.equal(_bits(a), _bits(c))


@pytest.mark.parametrize("br,bt", [(1, 1), (2, 7)])
def test_sinc_weights_at_off_grid_delays(tr, br, bt):
    """one live slot of amplitude 1 and phase 0 per link (f_c = 0, nu = 0, one element at the origin a side) at
    half-integer, tiny-fraction and negative delays x = f_s tau (exact in float32), with a one-hot unit-gain codebook
    (every beam the weight 1): every tap is sinc(l - x) within 10 * 2^-24, the bound tests/sinc_util.py derives for the
    weights of csrc/hrt_sinc.h"""
    x = np.array([2.5, 7.0 + 2.0 ** -12, -3.25, 0.5, -0.5, 60.75, -2.0 ** -14, 31.0 - 2.0 ** -10])
    n = len(x)
    dirs = np.tile([1.0, 0.0, 0.0], (n, 1))
    v = sparse.cluster_list(1, n, 1, np.arange(n), np.ones(n), np.zeros(n), x * U.TAU_STEP, np.zeros(n), dirs, -dirs)
    assert np.array_equal(v["tau"][0, :, 0].astype(np.float64) * U.FS, x) and (v["kept"] == 1).all()
    l_min, L = -8, 64
    z = np.zeros((1, 3), np.float32)
    wr, wt = np.ones((br, 1), np.complex64), np.ones((bt, 1), np.complex64)
    h = tr.sparse_beam_taps(v, z, z, wr, wt, U.FS, L, l_min, 0.0, array_frequency=U.F_A).cpu().numpy()
    want = np.sinc((l_min + np.arange(L))[None, :] - x[:, None])                     # [link, L]
    err = np.abs(h[0, :, :, :, 0, 0, :] - want[:, None, None, :]).max()
    print("worst |tap - sinc| = %.3g = %.2f * 2^-24" % (err, err * 2.0 ** 24))
    assert err <= 10 * 2.0 ** -24
    assert not h[0, :, :, :, 1].any() and not h[..., 0, 0, :].imag.any()
    ref, _ = sparse.beam_taps_reference(v, z, z, wr, wt, U.F_A, U.FS, 0.0, l_min + np.arange(L), [0.0])
    assert np.abs(h - ref).max() <= 10 * 2.0 ** -24


def test_tracer_refuses_what_is_its_own_to_refuse_and_passes_on_the_library_s_refusals(tr):
    from hermespy_rt_amd.device import Tracer
    t = Tracer.__new__(Tracer)          # (the checks read these attributes only; tr stays the owner of the device)
    t.torch, t.device, t.nrx, t.ntx, t.f_ghz = tr.torch, tr.device, 2, 3, tr.f_ghz
    t.L = tr.L
    U.tracer_value_errors(t)
    v = U.planted(2, 3, 8, 5, 0, 4)
    el, w = U.elements(2, 2), (U.codebook(2, 2, 0), U.codebook(3, 2, 1))
    a = t.sparse_beam_taps(v, *el, *w, U.FS, 4)
    assert tr.torch.equal(_bits(t.sparse_beam_taps(v["buffer"], *el, *w, U.FS, 4)), _bits(a))
    with pytest.raises(ValueError, match="hrt_sparse_beam_taps: .*array frequency"):
        t.sparse_beam_taps(v, *el, *w, U.FS, 4, array_frequency=-1.0)
    with pytest.raises(ValueError, match="hrt_sparse_beam_taps: .*num_taps"):
        t.sparse_beam_taps(v, *el, *w, U.FS, 0)
    with pytest.raises(ValueError, match="hrt_sparse_beam_taps: .*sampling rate"):
        t.sparse_beam_taps(v, *el, *w, 0.0, 4)
    with pytest.raises(ValueError, match=r"hrt_sparse_beam_taps: .*2\^24"):     # (refused before any allocation)
        t.sparse_beam_taps(v, *U.elements(1, 1), np.ones((64, 1), np.complex64), np.ones((16, 1), np.complex64),
                           U.FS, 129, num_times=128)
    with pytest.raises(ValueError, match="hrt_sparse_beam_taps: .*257 RX"):
        t.sparse_beam_taps(v, np.zeros((257, 3), np.float32), np.zeros((1, 3), np.float32),
                           np.ones((1, 257), np.complex64), np.ones((1, 1), np.complex64), U.FS, 4)
    with pytest.raises(ValueError, match="hrt_sparse_beam_taps: .*1 RX and 257 TX beams"):
        t.sparse_beam_taps(v, *U.elements(1, 1), np.ones((1, 1), np.complex64), np.ones((257, 1), np.complex64),
                           U.FS, 4)
