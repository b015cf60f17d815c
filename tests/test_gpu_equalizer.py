"""The per-point equalizers on planted tensors (Tracer.equalizer -> hrt_channel_equalizer; csrc/hrt_equalizer.hip), no
trace: plantings whose every intermediate is a power of two at tolerance 0, one-column plantings that pin every output
index, every lane-group size under the derived bounds, singular and non-finite points, independence of a point from
its neighbours and its tensor, the buffer rules.  Outputs are pre-filled with NaN bytes between guard bytes.  The cases
and their design: tests/equalizer_util.py, tests/test_equalizer_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import equalizer_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256
KIND_NAME = {U.ZF: "zf", U.LMMSE: "lmmse"}


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # equalizer reads only its tensor: nothing is traced
    yield t
    t.close()


def _run(tr, H, noise, kind, weights=True):
    """hrt_channel_equalizer on the numpy tensor H into NaN bytes between guards -> (views of the numpy copy, the input
    as the device holds it after the call)"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    spec = abi.equalizer_spec(nrx, ntx, nr, nt, T, K_, noise, kind, weights)
    need = abi.equalizer_regions(spec)[3]
    assert need == U.out_bytes(nrx, ntx, nr, nt, T, K_, int(spec.flags))
    d_H = torch.from_numpy(np.array(H, np.complex64)).to(tr.device)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    r = tr.equalizer(d_H, noise, KIND_NAME[kind], weights, out=big[GUARD:GUARD + need])
    assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    return abi.equalizer_views(host[GUARD:GUARD + need], spec), d_H.cpu().numpy()


def _batch(r):
    """device-layout views -> [B, ..] arrays in point order"""
    return (None if r["W"] is None else U.to_batch(r["W"]), U.to_batch_vec(r["sinr"]), r["status"].ravel())


# ---------------------------------------------------------------- tolerance 0

def test_exact_plantings_at_tolerance_zero(tr):
    for name, kind, n0, mats, W, S, st in U.exact_cases():
        B = mats.shape[0]
        H = U.tensor(mats, (1, 2), 1, B // 4)
        assert H.shape[0] * H.shape[1] * 2 * H.shape[6] == B
        r, _ = _run(tr, H, n0, kind)
        gw, gs, gst = _batch(r)
        assert np.array_equal(gst, st), name
        assert np.array_equal(gs, S), (name, np.argwhere(gs != S)[:4])
        assert np.array_equal(gw, W), (name, np.argwhere(gw != W)[:4])


@pytest.mark.parametrize("case", U.ONE_COLUMN, ids=lambda c: "%dx%d" % c[:2])
def test_one_column_plantings_pin_every_index(tr, case):
    nr, nt, K_ = case
    H, n0, W, S = U.one_column_case(nr, nt, K=K_)
    r, _ = _run(tr, H, n0, U.LMMSE)
    assert not r["status"].any()
    assert np.array_equal(r["sinr"], S), np.argwhere(r["sinr"] != S)[:4]
    assert np.array_equal(r["W"], W), np.argwhere(r["W"] != W)[:4]
    hit = np.zeros((nt, nr), bool)
    hit[np.nonzero(np.abs(U.to_batch(W)).sum(0))] = True
    assert hit.all() and (np.abs(W) > 0).sum() == 3 * S.size // nt


# ---------------------------------------------------------------- every shape under the derived bounds

_RESULTS = {}


def _shape_results(tr, shape, kind):
    """the device results of every grid of one shape and kind, computed once -> {grid: batch results}"""
    if (shape, kind) not in _RESULTS:
        mats, _ = U.master_cases(*shape)
        out = {}
        for links, T, K_ in U.grids(*shape):
            H = U.tensor(mats, links, T, K_)
            r, after = _run(tr, H, U.NOISE, kind)
            assert np.array_equal(after.view(np.float32), H.view(np.float32)), "the input was written"
            out[links, T, K_] = _batch(r)
        _RESULTS[shape, kind] = out
    return _RESULTS[shape, kind]


@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_under_the_derived_bounds(tr, shape):
    mats, kinds = U.master_cases(*shape)
    g = U.form(*shape)
    per_wg = U.THREADS // g
    counts = [links[0] * links[1] * 2 * T * K_ for links, T, K_ in U.grids(*shape)]
    assert counts[0] == 2 and per_wg + 2 in counts and (per_wg == 2 or per_wg - 2 in counts)
    assert any(c % per_wg for c in counts), (counts, per_wg)
    for kind in U.kinds_of(*shape):
        emu = None
        for (links, T, K_), (W, s, st) in _shape_results(tr, shape, kind).items():
            b = s.shape[0]
            assert b == links[0] * links[1] * 2 * T * K_
            bd = U.bounded(kinds[:b], kind)
            if bd.any():
                worst = U.check(mats[:b][bd], U.NOISE, kind, W[bd], s[bd], st[bd])
                if b == max(counts):
                    emu = U.emulate_batch(mats[:b], U.NOISE, kind)
                    print("shape %s g %d %s, %d points: measures %s; bits equal to the emulation's: W %s sinr %s"
                          % (shape, g, KIND_NAME[kind], b, " ".join("%.3g" % w for w in worst),
                             np.array_equal(emu[0], W), np.array_equal(emu[1], s)))
            # the rank-deficient family under ZF: singular, exact zeros
            assert (st[~bd] == U.SINGULAR).all() and not W[~bd].any() and not s[~bd].any()
        assert emu is not None


@pytest.mark.parametrize("shape", [(4, 4), (5, 4), (9, 7), (16, 16), (17, 16), (64, 16), (3, 16)],
                         ids=lambda s: "%dx%d" % s)
def test_a_point_depends_on_its_own_matrix_only(tr, shape):
    """the tensors of one shape are prefixes of one list of matrices: a matrix gives the same bytes in every tensor
    (another size, another link split, other neighbours in its workgroup), also moved to another point position and
    beside non-finite neighbours, which are flagged alone; two calls give the same bytes"""
    mats, _ = U.master_cases(*shape)
    for kind in U.kinds_of(*shape):
        res = _shape_results(tr, shape, kind)
        key_full = U.grids(*shape)[-1]
        full = res[key_full]
        for key, r in res.items():
            b = r[1].shape[0]
            assert U.same(r, [x[:b] for x in full]), key
        links, T, K_ = key_full
        b = links[0] * links[1] * 2 * T * K_
        moved = np.roll(mats[:b], 5, axis=0)
        r, _ = _run(tr, U.tensor(moved, links, T, K_), U.NOISE, kind)
        assert U.same(_batch(r), [np.roll(x[:b], 5, axis=0) for x in full])
        again, _ = _run(tr, U.tensor(moved, links, T, K_), U.NOISE, kind)
        assert U.same([r[k] for k in ("W", "sinr", "status")], [again[k] for k in ("W", "sinr", "status")])
        # a NaN in one matrix and an Inf in another: those points are flagged and zero, every other byte is the clean
        # run's
        dirty = np.array(mats[:b])
        dirty[3, 0, 0] = np.nan
        dirty[b - 2, shape[0] - 1, shape[1] - 1] = np.inf
        r, _ = _run(tr, U.tensor(dirty, links, T, K_), U.NOISE, kind)
        W, s, st = _batch(r)
        for p in (3, b - 2):
            assert st[p] == U.NONFINITE and not W[p].any() and not s[p].any()
        keep = np.ones(b, bool)
        keep[[3, b - 2]] = False
        assert U.same([x[keep] for x in (W, s, st)], [x[:b][keep] for x in full])


# ---------------------------------------------------------------- singular points

@pytest.mark.parametrize("shape", U.REPEATED_SHAPES, ids=lambda s: "%dx%d" % s)
def test_repeated_column_is_singular_under_zf_and_regular_under_lmmse(tr, shape):
    m, sing = U.repeated_cases(*shape)
    H = U.tensor(m, (1, 3), 1, 4)
    W, s, st = _batch(_run(tr, H, U.REPEATED_NOISE, U.ZF)[0])
    assert np.array_equal(st, np.where(sing, U.SINGULAR, 0))
    assert not W[sing].any() and not s[sing].any() and W[~sing].any(axis=(1, 2)).all() and (s[~sing] > 0).all()
    W, s, st = _batch(_run(tr, H, U.REPEATED_NOISE, U.LMMSE)[0])
    assert not st.any()
    assert not W[4].any() and not s[4].any()                 # H = 0 is regular: W = 0, sinr = 0
    reg = np.arange(24) != 4
    U.check(m[reg], U.REPEATED_NOISE, U.LMMSE, W[reg], s[reg], st[reg])   # (these are in the emulation's list)


# ---------------------------------------------------------------- weights, out and the wrapper's refusals

@pytest.mark.parametrize("shape", [(5, 3), (3, 16), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_without_weights_the_same_sinr_bits(tr, shape):
    mats, _ = U.master_cases(*shape)
    H = U.tensor(mats, (1, 3), 3, 5)
    for kind in U.kinds_of(*shape):
        full, _ = _run(tr, H, U.NOISE, kind)
        r, after = _run(tr, H, U.NOISE, kind, weights=False)   # (the guards behind the shorter buffer: checked in _run)
        assert np.array_equal(after.view(np.float32), H.view(np.float32))
        assert r["W"] is None and full["W"] is not None
        for k in ("sinr", "status"):
            assert np.array_equal(r[k].view(np.uint8), full[k].view(np.uint8)), (kind, k)
        assert not np.isnan(full["W"].view(np.float32)).any() and not np.isnan(full["sinr"]).any()   # poison overwritten
        d = tr.equalizer(tr.torch.from_numpy(H).to(tr.device), U.NOISE, KIND_NAME[kind], weights=False)
        assert d["W"] is None and d["status"].dtype == tr.torch.int32
        assert np.array_equal(d["sinr"].cpu().numpy(), full["sinr"])
        d = tr.equalizer(tr.torch.from_numpy(H).to(tr.device), U.NOISE, kind)       # (the constant as the kind)
        assert np.array_equal(d["buffer"].cpu().numpy(), full["buffer"])


def test_wrapper_refuses_what_it_cannot_pass(tr):
    torch = tr.torch
    H = torch.zeros((1, 1, 4, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    with pytest.raises(ValueError, match="complex64"):
        tr.equalizer(H.to(torch.complex128), 1.0)
    with pytest.raises(ValueError, match="complex64"):
        tr.equalizer(H.cpu(), 1.0)
    with pytest.raises(ValueError, match="expected"):
        tr.equalizer(H[0], 1.0)
    with pytest.raises(ValueError, match="out must be"):
        tr.equalizer(H, 1.0, out=torch.zeros(7, dtype=torch.uint8, device=tr.device))
    with pytest.raises(ValueError, match="kind"):
        tr.equalizer(H, 1.0, "mmse")
    with pytest.raises(ValueError, match="neither"):
        tr.equalizer(H, 1.0, 5)
    for noise in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise"):
            tr.equalizer(H, noise, "zf")
    with pytest.raises(ValueError, match="nr >= nt"):
        tr.equalizer(torch.zeros((1, 1, 2, 4, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0, "zf")
    with pytest.raises(ValueError, match="nt 1 .. 16"):
        tr.equalizer(torch.zeros((1, 1, 17, 17, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0)
    with pytest.raises(ValueError, match="nr 1 .. 64"):
        tr.equalizer(torch.zeros((1, 1, 65, 2, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0)
    with pytest.raises(ValueError, match="must be > 0"):
        tr.equalizer(torch.zeros((1, 1, 4, 2, 2, 0, 3), dtype=torch.complex64, device=tr.device), 1.0)
    # a non-contiguous view is equalised as the tensor it shows
    mats, _ = U.master_cases(4, 4)
    Hn = U.tensor(mats, (1, 2), 2, 3)
    base = torch.from_numpy(np.ascontiguousarray(np.swapaxes(Hn, 5, 6))).to(tr.device)
    a = tr.equalizer(base.transpose(5, 6), 0.5)
    b = tr.equalizer(torch.from_numpy(Hn).to(tr.device), 0.5)
    assert torch.equal(a["buffer"], b["buffer"])
    z = tr.equalizer(H, 0.25)                                            # H = 0 under LMMSE: regular
    assert not z["W"].any() and not z["sinr"].any() and not z["status"].any()
    z = tr.equalizer(H, 0.25, "zf")
    assert not z["W"].any() and not z["sinr"].any() and (z["status"] == abi.EQ_SINGULAR).all()
