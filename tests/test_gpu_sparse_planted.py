"""Tracer.sparse_array_channel (csrc/hrt_sparse_channel.hip) on planted lists, at tolerance 0: the exact planting of
tests/sparse_util.py (every output a Gaussian integer, proved without a device in tests/test_sparse_design.py) compared
value for value over the batch edge, the largest list, the pair tile and pair block, the inner length and the column
block, several links with different `kept`, and one-hot lists; then what must not reach the output (slots at or beyond
kept, another link's non-finite fields), accumulate, and the repeatability of the bytes.  No trace is needed: the
tracer is only the handle of the device."""
import numpy as np
import pytest

from . import configs as K
from . import sparse_util as U
from .pathsum_util import _bits, _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))
    yield t
    t.close()


def _run(tr, v, re, te, nk, nt, **kw):
    return tr.sparse_array_channel(v, re, te, U.F0, U.DF, nk, U.T0, U.DT, nt, array_frequency=U.F_A, **kw)


def _check(tr, v, nr, nt_, nk, nt, what):
    re, te = U.elements(nr, nt_)
    H = _run(tr, v, re, te, nk, nt)
    nrx, ntx, _ = v["tau"].shape
    assert tuple(H.shape) == (nrx, ntx, nr, nt_, 2, nt, nk)
    E = U.exact_reference(v, re, te, nk, nt)
    U.check_exact(H.cpu().numpy(), E, what)
    return H, E


@pytest.mark.parametrize("k", [1, 31, 32, 33, 1024])
def test_full_lists_over_the_batch_edge_and_the_largest_list(tr, k):
    _, E = _check(tr, U.planted(1, 1, k, k, salt=k), 2, 3, 17, 2, ("K", k))
    assert np.abs(E).max() >= 1


@pytest.mark.parametrize("kept", [0, 1, 32])
def test_kept_below_the_list_length(tr, kept):
    H, E = _check(tr, U.planted(1, 1, 33, kept, salt=3), 2, 3, 17, 2, ("kept", kept))
    assert bool(E.any()) == (kept > 0)


@pytest.mark.parametrize("nr,nt_", [(1, 1), (2, 8), (17, 1), (4, 8), (3, 11)])
def test_pair_tile_and_pair_block_edges(tr, nr, nt_):
    """Nr Nt = 1, 16, 17, 32, 33"""
    _check(tr, U.planted(1, 1, 33, 33, salt=nr), nr, nt_, 17, 1, ("pairs", nr, nt_))


@pytest.mark.parametrize("nt", [1, 3])
@pytest.mark.parametrize("nk", [1, 15, 16, 17, 256, 257])
def test_inner_length_and_column_block_edges(tr, nk, nt):
    _check(tr, U.planted(1, 1, 5, 5, salt=nk + nt), 2, 3, nk, nt, ("grid", nk, nt))


def test_five_links_with_different_kept_and_the_wrong_readings(tr):
    v = U.planted(1, 5, 33, [[0, 1, 33, 32, 7]], salt=9)
    H, E = _check(tr, v, 3, 11, 17, 3, "five links")
    assert not E[0, 0].any() and E[0, 1:].any(axis=(1, 2, 3, 4, 5)).all()
    # the device result is none of the wrong readings (tests/test_sparse_design.py: each differs from E on such cases)
    re, te = U.elements(3, 11)
    got = H.cpu().numpy()
    for name in U.MUTANTS:
        W = U.mutant(name, v, re, te, 17, 3)
        assert not np.array_equal(W, E), name
        with pytest.raises(AssertionError):
            U.check_exact(got, W, name)


def test_one_hot_lists_hit_every_index_once(tr):
    """one live slot, one nonzero amplitude component: every (link, pair, pol, m, k) of a 2 x 3 array, T = 2, K_f = 17"""
    nk, nt = 17, 2
    re, te = U.elements(2, 3)
    hit = np.zeros((1, 3, 2, 3, 2, nt, nk), np.int64)
    for link in range(3):
        for comp in range(4):
            v = U.one_hot(1, 3, link, comp, salt=link)
            H = _run(tr, v, re, te, nk, nt).cpu().numpy()
            U.check_exact(H, U.exact_reference(v, re, te, nk, nt), ("one hot", link, comp))
            hit += (H != 0)
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


def test_slots_at_or_beyond_kept_do_not_reach_the_output(tr):
    re, te = U.elements(4, 5)
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]], salt=4)
    clean = _run(tr, v, re, te, 17, 2)
    w = _poisoned(v)
    assert np.isnan(w["tau"][0, 0]).all() and np.isnan(w["a_te"][0, 1, 1:]).all() and not np.isnan(w["tau"][1, 0]).any()
    assert tr.torch.equal(_bits(_run(tr, w, re, te, 17, 2)), _bits(clean))
    U.check_exact(clean.cpu().numpy(), U.exact_reference(v, re, te, 17, 2), "clean")
    # kept > K in the header: min(kept, K) slots are read
    full = U.planted(2, 3, 33, 33, salt=4)
    over = U.copy(full)
    over["kept"][...] = np.array([[34, 1 << 20, 1 << 40], [(1 << 64) - 1, 33, 1 << 32]], np.uint64)
    assert tr.torch.equal(_bits(_run(tr, over, re, te, 17, 2)), _bits(_run(tr, full, re, te, 17, 2)))


def test_non_finite_fields_stay_within_their_link(tr):
    re, te = U.elements(4, 5)
    v = U.planted(2, 3, 33, [[33, 1, 32], [33, 7, 31]], salt=6)
    clean = _run(tr, v, re, te, 17, 2)
    w = U.copy(v)
    w["a_te"][0, 0, 5] = np.nan
    w["tau"][0, 0, 17] = np.inf
    w["u_rx"][0, 0, 32, 1] = np.nan
    bad = _run(tr, w, re, te, 17, 2)
    assert tr.torch.equal(_bits(bad[0, 1:]), _bits(clean[0, 1:])) and tr.torch.equal(_bits(bad[1]), _bits(clean[1]))
    assert bool(tr.torch.isnan(tr.torch.view_as_real(bad[0, 0])).any())


def test_accumulate_and_repeatability(tr):
    torch = tr.torch
    re, te = U.elements(4, 5)
    v = U.planted(1, 3, 64, [[64, 0, 31]], salt=8)
    a = _run(tr, v, re, te, 33, 2)
    b = _run(tr, v, re, te, 33, 2)
    assert torch.equal(_bits(a), _bits(b))                       # two calls: identical bytes
    # every byte is written: a NaN-filled `out` holds no NaN afterwards and the same bytes
    out = torch.full_like(a, complex(float("nan"), float("nan")))
    assert _run(tr, v, re, te, 33, 2, out=out) is out and torch.equal(_bits(out), _bits(a))
    # accumulate doubles the result bit for bit; the link with n = 0 stays as it was, bit for bit
    out = a.clone()
    out[0, 1] = complex(-0.0, 7.5)
    _run(tr, v, re, te, 33, 2, out=out, accumulate=True)
    want = a + a
    want[0, 1] = complex(-0.0, 7.5)
    assert torch.equal(_bits(out), _bits(want))
    with pytest.raises(ValueError, match="accumulate=True needs `out`"):
        _run(tr, v, re, te, 33, 2, accumulate=True)
    with pytest.raises(ValueError, match="out must be a contiguous complex64 tensor"):
        _run(tr, v, re, te, 33, 2, out=out[:, :2])


def test_device_buffer_and_numpy_upload_give_the_same_bytes(tr):
    """a result dict of device tensors (what dominant_paths() returns) is read where it is"""
    from hermespy_rt_amd import abi
    re, te = U.elements(2, 3)
    v = U.planted(2, 2, 7, [[7, 3], [0, 5]], salt=2)
    d = abi.dominant_views(tr.torch.from_numpy(v["buffer"]).to(tr.device), 2, 2, 7)
    a, b = _run(tr, v, re, te, 17, 2), _run(tr, d, re, te, 17, 2)
    assert tr.torch.equal(_bits(a), _bits(b))
    # sparse_channel: one zero-offset element, channel()'s layout
    z = np.zeros((1, 3), np.float32)
    s = tr.sparse_channel(v, U.F0, U.DF, 17, U.T0, U.DT, 2)
    assert tuple(s.shape) == (2, 2, 2, 2, 17)
    assert tr.torch.equal(_bits(s), _bits(_run(tr, v, z, z, 17, 2)[:, :, 0, 0]))


def test_tracer_refuses_lists_of_the_wrong_dtype_device_or_size(tr):
    from hermespy_rt_amd.device import Tracer
    t = Tracer.__new__(Tracer)          # (the checks read these five attributes only; tr stays the owner of the device)
    t.torch, t.device, t.nrx, t.ntx, t.f_ghz = tr.torch, tr.device, 2, 3, tr.f_ghz
    t.L = tr.L
    U.tracer_value_errors(t)
    # a bare buffer of this tracer's links is accepted, and what the library refuses arrives as a ValueError too
    v = U.planted(2, 3, 8, 5)
    a = t.sparse_array_channel(v, *U.elements(2, 2), U.F0, U.DF, 4)
    assert tr.torch.equal(_bits(t.sparse_array_channel(v["buffer"], *U.elements(2, 2), U.F0, U.DF, 4)), _bits(a))
    with pytest.raises(ValueError, match="hrt_sparse_array_channel: .*array frequency"):
        t.sparse_array_channel(v, *U.elements(2, 2), U.F0, U.DF, 4, array_frequency=-1.0)
    with pytest.raises(ValueError, match="hrt_sparse_array_channel: .*num_freqs"):
        t.sparse_array_channel(v, *U.elements(2, 2), U.F0, U.DF, 0)
    with pytest.raises(ValueError, match=r"hrt_sparse_array_channel: .*2\^24"):     # (refused before any allocation)
        t.sparse_array_channel(v, *U.elements(64, 16), U.F0, U.DF, 129, num_times=128)
    with pytest.raises(ValueError, match="hrt_sparse_array_channel: .*1025 RX"):
        t.sparse_array_channel(v, np.zeros((1025, 3), np.float32), np.zeros((1, 3), np.float32), U.F0, U.DF, 4)
