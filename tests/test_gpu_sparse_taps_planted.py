"""Tracer.sparse_array_taps (csrc/hrt_sparse_taps.hip) on planted lists, at tolerance 0: the exact planting of
tests/sparse_taps_util.py (every output a Gaussian integer, proved without a device in tests/test_sparse_taps_design.py)
compared value for value over the 4-slot MFMA step and the batch edge, the largest list, the switch between the two
forms of the kernel, the row-block edge (with a block that begins inside a pair), the column tile and column block of
both forms, tap windows left of, at and right of zero, several links with different `kept`, and one-hot lists; then what
must not reach the output (slots at or beyond kept, another link's non-finite fields), accumulate, the repeatability of
the bytes, and the sinc weights at off-grid delays.  No trace is needed: the tracer is only the handle of the device."""
import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import configs as K
from . import sparse_taps_util as U
from .pathsum_util import _bits, _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))
    yield t
    t.close()


def _run(tr, v, re, te, l_min, L, nt, **kw):
    return tr.sparse_array_taps(v, re, te, U.FS, L, l_min, U.FC, U.T0, U.DT, nt, array_frequency=U.F_A, **kw)


def _check(tr, v, nr, nt_, l_min, L, nt, what):
    re, te = U.elements(nr, nt_)
    h = _run(tr, v, re, te, l_min, L, nt)
    nrx, ntx, _ = v["tau"].shape
    assert tuple(h.shape) == (nrx, ntx, nr, nt_, 2, nt, L)
    E = U.exact_reference(v, re, te, l_min, L, nt)
    U.check_exact(h.cpu().numpy(), E, what)
    return h, E


@pytest.mark.parametrize("form", ["rt1", "rt4"])
@pytest.mark.parametrize("k", [1, 3, 4, 5, 31, 32, 33, 1024])
def test_full_lists_over_the_mfma_step_the_batch_edge_and_the_largest_list(tr, k, form):
    nr, nt_ = (2, 3) if form == "rt1" else (2, 7)
    _, E = _check(tr, U.planted(1, 1, k, k, -3, 17, salt=k), nr, nt_, -3, 17, 2, ("K", k, form))
    assert k < 8 or np.abs(E).max() >= 1


@pytest.mark.parametrize("kept", [0, 1, 32])
def test_kept_below_the_list_length(tr, kept):
    for nr, nt_ in ((2, 3), (2, 7)):
        v = U.planted(1, 1, 33, kept, -3, 17, salt=3)
        if kept == 1:
            v["tau"][0, 0, 0] = np.float32(2 * U.TAU_STEP)      # the one live slot inside the window
        h, E = _check(tr, v, nr, nt_, -3, 17, 2, ("kept", kept))
        assert bool(E.any()) == (kept > 0)


@pytest.mark.parametrize("nr,nt_,nt", [(2, 3, 2), (13, 1, 1), (4, 1, 3), (1, 13, 1), (1, 1, 1), (1, 1, 13)])
def test_the_switch_between_the_two_forms(tr, nr, nt_, nt):
    """Nr Nt T = 12 (three row tiles: 1 x 4 tiles a wave) and 13 (four: 4 x 4 tiles a wave), and the smallest grid"""
    _check(tr, U.planted(1, 1, 33, 33, -3, 17, salt=nr + nt), nr, nt_, -3, 17, nt, ("form", nr, nt_, nt))


@pytest.mark.parametrize("nr,nt_,nt", [(7, 9, 1), (8, 8, 1), (5, 13, 1), (3, 7, 3), (2, 11, 3), (2, 2, 16), (5, 13, 2)])
def test_row_block_edges(tr, nr, nt_, nt):
    """63, 64 and 65 rows with T = 1; 63 and 66 rows with T = 3 (the second block begins at time 1 of pair 21); 64 rows of
    4 pairs; 130 rows (three blocks)"""
    _check(tr, U.planted(1, 1, 9, 9, 2, 17, salt=nr * nt), nr, nt_, 2, 17, nt, ("rows", nr, nt_, nt))


@pytest.mark.parametrize("l_min", [-70, 0, 9])
@pytest.mark.parametrize("L", [1, 15, 16, 17, 63, 64, 65])
def test_column_tile_and_column_block_edges_of_the_four_tile_form(tr, L, l_min):
    _check(tr, U.planted(1, 1, 12, 12, l_min, L, salt=L), 2, 7, l_min, L, 1, ("taps rt4", L, l_min))


@pytest.mark.parametrize("L,l_min", [(1, 0), (63, -5), (65, 3), (255, -300), (256, 0), (257, 11)])
def test_column_tile_and_column_block_edges_of_the_one_tile_form(tr, L, l_min):
    _check(tr, U.planted(1, 1, 12, 12, l_min, L, salt=L), 2, 3, l_min, L, 2, ("taps rt1", L, l_min))


@pytest.mark.parametrize("nr,nt_", [(2, 3), (3, 11)])
def test_five_links_with_different_kept_and_the_wrong_readings(tr, nr, nt_):
    l_min, L, nt = -40, 17, 3
    v = U.planted(1, 5, 33, [[0, 1, 33, 32, 7]], l_min, L, salt=9)
    h, E = _check(tr, v, nr, nt_, l_min, L, nt, "five links")
    assert not E[0, 0].any() and E[0, 2:].any(axis=(1, 2, 3, 4, 5)).all()
    # the device result is none of the wrong readings (tests/test_sparse_taps_design.py: each differs from E on such cases)
    re, te = U.elements(nr, nt_)
    got = h.cpu().numpy()
    for name in U.MUTANTS:
        W = U.mutant(name, v, re, te, l_min, L, nt)
        assert not np.array_equal(W, E), name
        with pytest.raises(AssertionError):
            U.check_exact(got, W, name)


def test_one_hot_lists_hit_every_index_once(tr):
    """one live slot, one nonzero amplitude component, at every tap of the window in turn: every (link, pair, pol, m, l)
    of a 2 x 3 array, T = 2, L = 5"""
    l_min, L, nt = -2, 5, 2
    re, te = U.elements(2, 3)
    hit = np.zeros((1, 3, 2, 3, 2, nt, L), np.int64)
    for link in range(3):
        for comp in range(4):
            for k in range(L):
                v = U.one_hot(1, 3, link, comp, l_min + k, salt=link)
                h = _run(tr, v, re, te, l_min, L, nt).cpu().numpy()
                U.check_exact(h, U.exact_reference(v, re, te, l_min, L, nt), ("one hot", link, comp, k))
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


@pytest.mark.parametrize("nr,nt_", [(2, 3), (4, 5)])
def test_slots_at_or_beyond_kept_do_not_reach_the_output(tr, nr, nt_):
    l_min, L, nt = -3, 17, 2
    re, te = U.elements(nr, nt_)
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]], l_min, L, salt=4)
    clean = _run(tr, v, re, te, l_min, L, nt)
    w = _poisoned(v)
    assert np.isnan(w["tau"][0, 0]).all() and np.isnan(w["a_te"][0, 1, 1:]).all() and not np.isnan(w["tau"][1, 0]).any()
    assert tr.torch.equal(_bits(_run(tr, w, re, te, l_min, L, nt)), _bits(clean))
    U.check_exact(clean.cpu().numpy(), U.exact_reference(v, re, te, l_min, L, nt), "clean")
    # kept > K in the header: min(kept, K) slots are read
    full = U.planted(2, 3, 33, 33, l_min, L, salt=4)
    over = U.copy(full)
    over["kept"][...] = np.array([[34, 1 << 20, 1 << 40], [(1 << 64) - 1, 33, 1 << 32]], np.uint64)
    assert tr.torch.equal(_bits(_run(tr, over, re, te, l_min, L, nt)), _bits(_run(tr, full, re, te, l_min, L, nt)))


@pytest.mark.parametrize("nr,nt_", [(2, 3), (4, 5)])
def test_non_finite_fields_stay_within_their_link(tr, nr, nt_):
    l_min, L, nt = -3, 17, 2
    re, te = U.elements(nr, nt_)
    v = U.planted(2, 3, 33, [[33, 1, 32], [33, 7, 31]], l_min, L, salt=6)
    clean = _run(tr, v, re, te, l_min, L, nt)
    w = U.copy(v)
    w["a_te"][0, 0, 5] = np.nan
    w["tau"][0, 0, 17] = np.inf
    w["u_rx"][0, 0, 32, 1] = np.nan
    bad = _run(tr, w, re, te, l_min, L, nt)
    assert tr.torch.equal(_bits(bad[0, 1:]), _bits(clean[0, 1:])) and tr.torch.equal(_bits(bad[1]), _bits(clean[1]))
    assert bool(tr.torch.isnan(tr.torch.view_as_real(bad[0, 0])).any())


@pytest.mark.parametrize("nr,nt_", [(2, 3), (4, 5)])
def test_accumulate_and_repeatability(tr, nr, nt_):
    torch = tr.torch
    l_min, L, nt = -3, 33, 2
    re, te = U.elements(nr, nt_)
    v = U.planted(1, 3, 64, [[64, 0, 31]], l_min, L, salt=8)
    a = _run(tr, v, re, te, l_min, L, nt)
    b = _run(tr, v, re, te, l_min, L, nt)
    assert torch.equal(_bits(a), _bits(b)) and float(a.abs().max()) >= 1      # two calls: identical bytes
    # every byte is written: a NaN-filled `out` holds no NaN afterwards and the same bytes
    out = torch.full_like(a, complex(float("nan"), float("nan")))
    assert _run(tr, v, re, te, l_min, L, nt, out=out) is out and torch.equal(_bits(out), _bits(a))
    # accumulate doubles the result bit for bit; the link with n = 0 stays as it was, bit for bit
    out = a.clone()
    out[0, 1] = complex(-0.0, 7.5)
    _run(tr, v, re, te, l_min, L, nt, out=out, accumulate=True)
    want = a + a
    want[0, 1] = complex(-0.0, 7.5)
    assert torch.equal(_bits(out), _bits(want))
    with pytest.raises(ValueError, match="accumulate=True needs `out`"):
        _run(tr, v, re, te, l_min, L, nt, accumulate=True)
    with pytest.raises(ValueError, match="out must be a contiguous complex64 tensor"):
        _run(tr, v, re, te, l_min, L, nt, out=out[:, :2])


def test_device_buffer_and_numpy_upload_give_the_same_bytes(tr):
    """a result dict of device tensors (what dominant_paths() returns) is read where it is"""
    from hermespy_rt_amd import abi
    re, te = U.elements(2, 3)
    v = U.planted(2, 2, 7, [[7, 3], [0, 5]], -3, 17, salt=2)
    d = abi.dominant_views(tr.torch.from_numpy(v["buffer"]).to(tr.device), 2, 2, 7)
    a, b = _run(tr, v, re, te, -3, 17, 2), _run(tr, d, re, te, -3, 17, 2)
    assert tr.torch.equal(_bits(a), _bits(b))
    # sparse_taps: one zero-offset element, taps()'s layout
    z = np.zeros((1, 3), np.float32)
    s = tr.sparse_taps(v, U.FS, 17, -3, U.FC, U.T0, U.DT, 2)
    assert tuple(s.shape) == (2, 2, 2, 2, 17)
    assert tr.torch.equal(_bits(s), _bits(_run(tr, v, z, z, -3, 17, 2)[:, :, 0, 0]))


@pytest.mark.parametrize("nr,nt_", [(1, 1), (2, 7)])
def test_sinc_weights_at_off_grid_delays(tr, nr, nt_):
    """one live slot of amplitude 1 and phase 0 per link (f_c = 0, nu = 0, every element at the origin) at half-integer,
    tiny-fraction and negative delays x = f_s tau (exact in float32): every tap is sinc(l - x) within 10 * 2^-24, the
    bound tests/sinc_util.py derives for the weights of csrc/hrt_sinc.h"""
    x = np.array([2.5, 7.0 + 2.0 ** -12, -3.25, 0.5, -0.5, 60.75, -2.0 ** -14, 31.0 - 2.0 ** -10])
    n = len(x)
    dirs = np.tile([1.0, 0.0, 0.0], (n, 1))
    v = sparse.cluster_list(1, n, 1, np.arange(n), np.ones(n), np.zeros(n), x * U.TAU_STEP, np.zeros(n), dirs, -dirs)
    assert np.array_equal(v["tau"][0, :, 0].astype(np.float64) * U.FS, x) and (v["kept"] == 1).all()
    l_min, L = -8, 64
    zr, zt = np.zeros((nr, 3), np.float32), np.zeros((nt_, 3), np.float32)
    h = tr.sparse_array_taps(v, zr, zt, U.FS, L, l_min, 0.0, array_frequency=U.F_A).cpu().numpy()
    want = np.sinc((l_min + np.arange(L))[None, :] - x[:, None])                     # [link, L]
    err = np.abs(h[0, :, :, :, 0, 0, :] - want[:, None, None, :]).max()
    print("worst |tap - sinc| = %.3g = %.2f * 2^-24" % (err, err * 2.0 ** 24))
    assert err <= 10 * 2.0 ** -24
    assert not h[0, :, :, :, 1].any() and not h[..., 0, 0, :].imag.any()
    ref, _ = sparse.taps_reference(v, zr, zt, U.F_A, U.FS, 0.0, l_min + np.arange(L), [0.0])
    assert np.abs(h - ref).max() <= 10 * 2.0 ** -24


def test_tracer_refuses_lists_of_the_wrong_dtype_device_or_size(tr):
    from hermespy_rt_amd.device import Tracer
    t = Tracer.__new__(Tracer)          # (the checks read these five attributes only; tr stays the owner of the device)
    t.torch, t.device, t.nrx, t.ntx, t.f_ghz = tr.torch, tr.device, 2, 3, tr.f_ghz
    t.L = tr.L
    U.tracer_value_errors(t)
    # a bare buffer of this tracer's links is accepted, and what the library refuses arrives as a ValueError too
    v = U.planted(2, 3, 8, 5, 0, 4)
    el = U.elements(2, 2)
    a = t.sparse_array_taps(v, *el, U.FS, 4)
    assert tr.torch.equal(_bits(t.sparse_array_taps(v["buffer"], *el, U.FS, 4)), _bits(a))
    with pytest.raises(ValueError, match="hrt_sparse_array_taps: .*array frequency"):
        t.sparse_array_taps(v, *el, U.FS, 4, array_frequency=-1.0)
    with pytest.raises(ValueError, match="hrt_sparse_array_taps: .*num_taps"):
        t.sparse_array_taps(v, *el, U.FS, 0)
    with pytest.raises(ValueError, match="hrt_sparse_array_taps: .*sampling rate"):
        t.sparse_array_taps(v, *el, 0.0, 4)
    with pytest.raises(ValueError, match=r"hrt_sparse_array_taps: .*2\^24"):     # (refused before any allocation)
        t.sparse_array_taps(v, *U.elements(64, 16), U.FS, 129, num_times=128)
    with pytest.raises(ValueError, match="hrt_sparse_array_taps: .*1025 RX"):
        t.sparse_array_taps(v, np.zeros((1025, 3), np.float32), np.zeros((1, 3), np.float32), U.FS, 4)
