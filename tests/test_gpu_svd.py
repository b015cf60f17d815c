"""The per-point SVD on planted tensors (Tracer.svd -> hrt_channel_svd; csrc/hrt_svd.hip), no trace: matrices that need
no rotation at tolerance 0, one-hot plantings that pin every index, every lane-group size and both orientations under
the derived bounds, independence of a point from its neighbours and its tensor, non-finite input, the `want`
combinations.  Outputs are pre-filled with NaN bytes between guard bytes.  The cases and their design:
tests/svd_util.py, tests/test_svd_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import svd_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # svd reads only its tensor: nothing is traced
    yield t
    t.close()


def _run(tr, H, want=3):
    """hrt_channel_svd on the numpy tensor H into NaN bytes between guards -> (views of the numpy copy, the input as
    the device holds it after the call)"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    spec = abi.svd_spec(nrx, ntx, nr, nt, T, K_, want=want)
    need = abi.svd_regions(spec)[4]
    assert need == U.out_bytes(nrx, ntx, nr, nt, T, K_, want)
    d_H = torch.from_numpy(np.array(H, np.complex64)).to(tr.device)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    if want == 3:
        r = tr.svd(d_H, out=big[GUARD:GUARD + need])
        assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    else:
        abi.run_channel_svd(tr.L, tr.device.index, spec, d_H.data_ptr(), big.data_ptr() + GUARD,
                            torch.cuda.current_stream(tr.device).cuda_stream)
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    return abi.svd_views(host[GUARD:GUARD + need], spec), d_H.cpu().numpy()


def _batch(r):
    """device-layout views -> [B, ..] arrays in point order"""
    return (U.to_batch_sigma(r["sigma"]), None if r["u"] is None else U.to_batch(r["u"]),
            None if r["v"] is None else U.to_batch(r["v"]), r["sweeps"].ravel())


# ---------------------------------------------------------------- tolerance 0

def test_exact_plantings_at_tolerance_zero(tr):
    for name, mats, (s, u, v) in U.exact_cases():
        B = mats.shape[0]
        H = U.tensor(mats, (2, 2), 1, B // 8)
        assert H.shape[0] * H.shape[1] * 2 * H.shape[6] == B
        r, _ = _run(tr, H)
        gs, gu, gv, sw = _batch(r)
        assert not sw.any(), name
        assert np.array_equal(gs, s), (name, np.argwhere(gs != s)[:4])
        assert np.array_equal(gu, u), (name, np.argwhere(gu != u)[:4])
        assert np.array_equal(gv, v), (name, np.argwhere(gv != v)[:4])


def test_one_hot_plantings_pin_every_index(tr):
    shape = (2, 2, 3, 2, 2, 2, 3)
    val = np.complex64(-2j)
    count = 0
    for at in np.ndindex(*shape):
        H = np.zeros(shape, np.complex64)
        H[at] = val
        r, _ = _run(tr, H)
        rx, tx, i, j, pol, m, k = at
        sig = np.zeros((2, 2, 2, 2, 2, 3), np.float32)
        sig[rx, tx, 0, pol, m, k] = 2.0
        u = np.zeros((2, 2, 3, 2, 2, 2, 3), np.complex64)
        u[rx, tx, i, 0, pol, m, k] = -1j
        v = np.zeros((2, 2, 2, 2, 2, 2, 3), np.complex64)
        v[:, :, 0, 0], v[:, :, 1, 1] = 1, 1                               # H = 0: the identity on the short side
        v[rx, tx, :, :, pol, m, k] = np.eye(2)[[j, 1 - j]].T              # column j first, the zero column after it
        assert np.array_equal(r["sigma"], sig), at
        assert np.array_equal(r["u"], u), at
        assert np.array_equal(r["v"], v), at
        assert not r["sweeps"].any()
        count += 1
    assert count == 288


# ---------------------------------------------------------------- every shape under the derived bounds

_RESULTS = {}


def _shape_results(tr, shape):
    """the device results of every grid of one shape, computed once -> {grid: (H, batch results)}"""
    if shape not in _RESULTS:
        mats, _ = U.master_cases(*shape)
        out = {}
        for links, T, K_ in U.GRIDS:
            H = U.tensor(mats, links, T, K_)
            r, after = _run(tr, H)
            assert np.array_equal(after.view(np.float32), H.view(np.float32)), "the input was written"
            out[links, T, K_] = _batch(r)
        _RESULTS[shape] = out
    return _RESULTS[shape]


@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_under_the_derived_bounds(tr, shape):
    mats, kinds = U.master_cases(*shape)
    g = U.form(*shape)
    per_wg = U.THREADS // g
    counts = [links[0] * links[1] * 2 * T * K_ for links, T, K_ in U.GRIDS]
    assert counts[:4] == [8 * 1, 8 * 63, 8 * 64, 8 * 65] and any(c % per_wg for c in counts), (counts, per_wg)
    for (links, T, K_), (s, u, v, sw) in _shape_results(tr, shape).items():
        b = s.shape[0]
        assert b == links[0] * links[1] * 2 * T * K_
        worst = U.check(mats[:b], s, u, v, sw, relative=kinds[:b] != 3)
        print("shape %s g %d, %d points: sweeps <= %d, measures in u: %s"
              % (shape, g, b, int(sw.max()), " ".join("%.2f" % w for w in worst)))
        assert (sw < U.MAX_SWEEPS).all()
        r1 = kinds[:b] == 1
        if min(shape) >= 2 and r1.any():
            long_ = u if shape[0] >= shape[1] else v
            assert not long_[r1][:, :, 1:].any()                          # rank one: n - 1 exactly zero columns
            assert np.allclose(s[r1, 0], np.sqrt(shape[0] * shape[1]), rtol=1e-6)


@pytest.mark.parametrize("shape", [(4, 4), (8, 4), (8, 8), (16, 8), (16, 16), (32, 16), (64, 16), (16, 64), (5, 3)],
                         ids=lambda s: "%dx%d" % s)
def test_a_point_depends_on_its_own_matrix_only(tr, shape):
    """the tensors of one shape are prefixes of one list of matrices: a matrix gives the same bytes in every tensor
    (another size, another link split, other neighbours in its workgroup), also moved to another point position and
    beside non-finite neighbours; two calls give the same bytes"""
    mats, _ = U.master_cases(*shape)
    res = _shape_results(tr, shape)
    full = res[U.GRIDS[3]]
    for key, r in res.items():
        b = r[0].shape[0]
        assert U.same(r, [x[:b] for x in full]), key
    links, T, K_ = U.GRIDS[1]
    b = links[0] * links[1] * 2 * T * K_
    moved = np.roll(mats[:b], 5, axis=0)
    r, _ = _run(tr, U.tensor(moved, links, T, K_))
    assert U.same(_batch(r), [np.roll(x[:b], 5, axis=0) for x in full])
    again, _ = _run(tr, U.tensor(moved, links, T, K_))
    assert U.same([r[k] for k in ("sigma", "u", "v", "sweeps")], [again[k] for k in ("sigma", "u", "v", "sweeps")])
    # a NaN in one matrix and an Inf in another: the call returns, those points are flagged or NaN, every other byte
    # is the clean run's
    dirty = np.array(mats[:b])
    dirty[3, 0, 0] = np.nan
    dirty[b - 2, shape[0] - 1, shape[1] - 1] = np.inf
    r, _ = _run(tr, U.tensor(dirty, links, T, K_))
    s, u, v, sw = _batch(r)
    for p in (3, b - 2):
        assert sw[p] == U.NOT_CONVERGED or np.isnan(s[p]).any()
    keep = np.ones(b, bool)
    keep[[3, b - 2]] = False
    assert U.same([x[keep] for x in (s, u, v, sw)], [x[:b][keep] for x in full])


# ---------------------------------------------------------------- want, out and the wrapper's refusals

@pytest.mark.parametrize("shape", [(5, 3), (3, 5), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_want_combinations(tr, shape):
    mats, _ = U.master_cases(*shape)
    links, T, K_ = (1, 3), 3, 5
    H = U.tensor(mats, links, T, K_)
    full, _ = _run(tr, H, 3)
    for want in (0, 1, 2):
        r, after = _run(tr, H, want)                    # (the guards behind the shorter buffer are checked in _run)
        assert np.array_equal(after.view(np.float32), H.view(np.float32))
        assert (r["u"] is None) == (not want & 1) and (r["v"] is None) == (not want & 2)
        for k in ("sigma", "u", "v", "sweeps"):
            if r[k] is not None:
                assert np.array_equal(r[k].view(np.uint8), full[k].view(np.uint8)), (want, k)
    r = tr.svd(tr.torch.from_numpy(H).to(tr.device), vectors=False)
    assert r["u"] is None and r["v"] is None
    assert np.array_equal(r["sigma"].cpu().numpy(), full["sigma"])
    assert r["sweeps"].dtype == tr.torch.int32 and np.array_equal(r["sweeps"].cpu().numpy().view(np.uint32), full["sweeps"])


def test_wrapper_refuses_what_it_cannot_pass(tr):
    torch = tr.torch
    H = torch.zeros((1, 1, 4, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    with pytest.raises(ValueError, match="complex64"):
        tr.svd(H.to(torch.complex128))
    with pytest.raises(ValueError, match="complex64"):
        tr.svd(H.cpu())
    with pytest.raises(ValueError, match="expected"):
        tr.svd(H[0])
    with pytest.raises(ValueError, match="expected"):
        tr.svd(H.reshape(1, 1, 4, 2, 1, 2, 3))
    with pytest.raises(ValueError, match="out must be"):
        tr.svd(H, out=torch.zeros(7, dtype=torch.uint8, device=tr.device))
    with pytest.raises(ValueError, match="the smaller 1 .. 16"):
        tr.svd(torch.zeros((1, 1, 17, 17, 2, 1, 1), dtype=torch.complex64, device=tr.device))
    with pytest.raises(ValueError, match="the larger 1 .. 64"):
        tr.svd(torch.zeros((1, 1, 65, 2, 2, 1, 1), dtype=torch.complex64, device=tr.device))
    with pytest.raises(ValueError, match="must be > 0"):
        tr.svd(torch.zeros((1, 1, 4, 2, 2, 0, 3), dtype=torch.complex64, device=tr.device))
    # a non-contiguous view is decomposed as the tensor it shows
    mats, _ = U.master_cases(4, 4)
    Hn = U.tensor(mats, (1, 2), 2, 3)
    base = torch.from_numpy(np.ascontiguousarray(np.swapaxes(Hn, 5, 6))).to(tr.device)
    a = tr.svd(base.transpose(5, 6))
    b = tr.svd(torch.from_numpy(Hn).to(tr.device))
    assert torch.equal(a["buffer"], b["buffer"])
    z = tr.svd(H)                                        # H = 0
    assert not z["sigma"].any() and not z["u"].any() and not z["sweeps"].any()
    assert torch.equal(z["v"][0, 0, :, :, 1, 0, 2].real, torch.eye(2, device=tr.device))
