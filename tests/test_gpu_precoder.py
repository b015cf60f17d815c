"""The per-point precoders on planted tensors (Tracer.precoder -> hrt_channel_precoder; csrc/hrt_precoder.hip), no trace:
plantings whose every intermediate is exact at tolerance 0, one-row plantings that pin every output index, every
lane-group size, kind and norm under the derived bounds, the heavily regularised set, singular and non-finite points,
independence of a point from its neighbours and its tensor, the buffer rules.  Outputs are pre-filled with NaN bytes
between guard bytes.  The cases and their design: tests/precoder_util.py, tests/test_precoder_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import precoder_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # precoder reads only its tensor: nothing is traced
    yield t
    t.close()


def _run(tr, H, noise, kind, norm, power=U.POWER, alpha=None, weights=True):
    """hrt_channel_precoder on the numpy tensor H into NaN bytes between guards -> (views of the numpy copy, the input
    as the device holds it after the call)"""
    torch = tr.torch
    nrx, ntx, nr, nt, _, T, K_ = H.shape
    spec = abi.precoder_spec(nrx, ntx, nr, nt, T, K_, noise, kind, power, alpha, norm, weights)
    need = abi.precoder_regions(spec)[3]
    assert need == U.out_bytes(nrx, ntx, nr, nt, T, K_, int(spec.flags))
    d_H = torch.from_numpy(np.array(H, np.complex64)).to(tr.device)
    big = torch.full((need + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=tr.device)
    big[GUARD:GUARD + need] = 0xFF
    r = tr.precoder(d_H, noise, U.KIND_NAME[kind], power, alpha, U.NORM_NAME[norm], weights,
                    out=big[GUARD:GUARD + need])
    assert r["buffer"].data_ptr() == big.data_ptr() + GUARD
    torch.cuda.synchronize(tr.device)
    host = big.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + need:] == 0xA5).all(), "written beyond the buffer"
    return abi.precoder_views(host[GUARD:GUARD + need], spec), d_H.cpu().numpy()


def _batch(r):
    """device-layout views -> [B, ..] arrays in point order"""
    return (None if r["P"] is None else U.to_batch(r["P"]), U.to_batch_vec(r["sinr"]), r["status"].ravel())


# ---------------------------------------------------------------- tolerance 0

def test_exact_plantings_at_tolerance_zero(tr):
    for name, kind, norm, n0, power, alpha, mats, P, S, st in U.exact_cases():
        B = mats.shape[0]
        H = U.tensor(mats, (1, 2), 1, B // 4)
        assert H.shape[0] * H.shape[1] * 2 * H.shape[6] == B
        r, _ = _run(tr, H, n0, kind, norm, power, alpha)
        gp, gs, gst = _batch(r)
        assert np.array_equal(gst, st), name
        assert np.array_equal(gs, S), (name, np.argwhere(gs != S)[:4])
        assert np.array_equal(gp, P), (name, np.argwhere(gp != P)[:4])


@pytest.mark.parametrize("case", U.ONE_ROW, ids=lambda c: "%s-%dx%d" % (U.KIND_NAME[c[0]], c[1], c[2]))
def test_one_row_plantings_pin_every_index(tr, case):
    kind, nr, nt, K_ = case
    H, n0, power, alpha, P, S = U.one_row_case(kind, nr, nt, K=K_)
    r, _ = _run(tr, H, n0, kind, U.TOTAL, power, alpha)
    assert not r["status"].any()
    assert np.array_equal(r["sinr"], S), np.argwhere(r["sinr"] != S)[:4]
    assert np.array_equal(r["P"], P), np.argwhere(r["P"] != P)[:4]
    hit = np.abs(U.to_batch(P)).sum(0) > 0
    assert hit.all() and (S > 0).sum() == S.size // nr


# ---------------------------------------------------------------- every shape under the derived bounds

_RESULTS = {}


def _shape_results(tr, shape, kind, norm):
    """the device results of every grid of one shape, kind and norm, computed once -> {grid: batch results}"""
    key = (shape, kind, norm)
    if key not in _RESULTS:
        mats, _ = U.master_cases(*shape)
        out = {}
        for links, T, K_ in U.grids(*shape):
            H = U.tensor(mats, links, T, K_)
            r, after = _run(tr, H, U.NOISE, kind, norm)
            assert np.array_equal(after.view(np.float32), H.view(np.float32)), "the input was written"
            out[links, T, K_] = _batch(r)
        _RESULTS[key] = out
    return _RESULTS[key]


@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "%dx%d" % s)
def test_shapes_under_the_derived_bounds(tr, shape):
    mats, kinds = U.master_cases(*shape)
    g = U.form(*shape)
    per_wg = U.THREADS // g
    counts = [links[0] * links[1] * 2 * T * K_ for links, T, K_ in U.grids(*shape)]
    assert counts[0] == 2 and per_wg + 2 in counts and (per_wg == 2 or per_wg - 2 in counts)
    assert any(c % per_wg for c in counts), (counts, per_wg)
    for kind in U.kinds_of(*shape):
        alpha = U.default_alpha(shape[0]) if kind == U.RZF else 0.0
        for norm in U.NORMS:
            emu = None
            for (links, T, K_), (P, s, st) in _shape_results(tr, shape, kind, norm).items():
                b = s.shape[0]
                assert b == links[0] * links[1] * 2 * T * K_
                bd = U.bounded(kinds[:b], kind)
                if bd.any():
                    worst = U.check(mats[:b][bd], U.NOISE, kind, norm, U.POWER, alpha, P[bd], s[bd], st[bd])
                    if b == max(counts):
                        emu = U.emulate_batch(mats[:b], U.NOISE, kind, norm)
                        print("shape %s g %d %s %s, %d points: measures %s; bits equal to the emulation's: P %s sinr %s"
                              % (shape, g, U.KIND_NAME[kind], U.NORM_NAME[norm], b, " ".join("%.3g" % w for w in worst),
                                 np.array_equal(emu[0], P), np.array_equal(emu[1], s)))
                # the rank-deficient family under ZF: singular, exact zeros
                assert (st[~bd] == U.SINGULAR).all() and not P[~bd].any() and not s[~bd].any()
            assert emu is not None


@pytest.mark.parametrize("shape", U.HEAVY_SHAPES, ids=lambda s: "%dx%d" % s)
def test_heavily_regularised_set_under_the_bounds(tr, shape):
    """alpha = 2^8 E|H|_F^2: E = H P of the stored P holds the bounds where the identity I - alpha T T^H would not
    (tests/test_precoder_design.py)"""
    mats, alpha = U.heavy_cases(*shape)
    H = U.tensor(mats, (1, 3), 1, 4)
    for norm in U.NORMS:
        P, s, st = _batch(_run(tr, H, U.NOISE, U.RZF, norm, U.POWER, alpha)[0])
        worst = U.check(mats, U.NOISE, U.RZF, norm, U.POWER, alpha, P, s, st)
        emu = U.emulate_batch(mats, U.NOISE, U.RZF, norm, U.POWER, alpha)
        print("heavy %s %s: measures %s; bits equal to the emulation's: P %s sinr %s"
              % (shape, U.NORM_NAME[norm], " ".join("%.3g" % w for w in worst), np.array_equal(emu[0], P),
                 np.array_equal(emu[1], s)))
        assert (s > 0).all()


@pytest.mark.parametrize("shape", [(4, 4), (4, 5), (7, 9), (16, 16), (16, 17), (16, 64), (16, 3)],
                         ids=lambda s: "%dx%d" % s)
def test_a_point_depends_on_its_own_matrix_only(tr, shape):
    """the tensors of one shape are prefixes of one list of matrices: a matrix gives the same bytes in every tensor
    (another size, another link split, other neighbours in its workgroup), also moved to another point position and
    beside non-finite neighbours, which are flagged alone; two calls give the same bytes"""
    mats, _ = U.master_cases(*shape)
    for kind in U.kinds_of(*shape):
        for norm in U.NORMS if kind == U.RZF else (U.TOTAL,):
            res = _shape_results(tr, shape, kind, norm)
            key_full = U.grids(*shape)[-1]
            full = res[key_full]
            for key, r in res.items():
                b = r[1].shape[0]
                assert U.same(r, [x[:b] for x in full]), key
            links, T, K_ = key_full
            b = links[0] * links[1] * 2 * T * K_
            moved = np.roll(mats[:b], 5, axis=0)
            r, _ = _run(tr, U.tensor(moved, links, T, K_), U.NOISE, kind, norm)
            assert U.same(_batch(r), [np.roll(x[:b], 5, axis=0) for x in full])
            again, _ = _run(tr, U.tensor(moved, links, T, K_), U.NOISE, kind, norm)
            assert U.same([r[k] for k in ("P", "sinr", "status")], [again[k] for k in ("P", "sinr", "status")])
            # a NaN in one matrix and an Inf in another: those points are flagged and zero, every other byte is the
            # clean run's
            dirty = np.array(mats[:b])
            dirty[3, 0, 0] = np.nan
            dirty[b - 2, shape[0] - 1, shape[1] - 1] = np.inf
            r, _ = _run(tr, U.tensor(dirty, links, T, K_), U.NOISE, kind, norm)
            P, s, st = _batch(r)
            for p in (3, b - 2):
                assert st[p] == U.NONFINITE and not P[p].any() and not s[p].any()
            keep = np.ones(b, bool)
            keep[[3, b - 2]] = False
            assert U.same([x[keep] for x in (P, s, st)], [x[:b][keep] for x in full])


# ---------------------------------------------------------------- singular points

@pytest.mark.parametrize("shape", [(4, 4), (7, 9), (16, 17), (16, 64)], ids=lambda s: "%dx%d" % s)
def test_zero_and_repeated_rows_are_flagged_as_the_reference_flags_them(tr, shape):
    """24 standard normal matrices; in the odd ones the last row repeats the first (SINGULAR under ZF, regular
    otherwise), matrix 4 is H = 0 (SINGULAR under every kind), in matrix 6 row 1 is zero (a user without a channel:
    SINGULAR under ZF and under STREAM, regular under MRT and RZF with TOTAL, where its stream gets no power)"""
    nr, nt = shape
    mats, kinds = U.master_cases(nr, nt)
    m = np.array(mats[kinds == 0][:24])
    m[1::2, nr - 1] = m[1::2, 0]
    m[4] = 0
    m[6, 1] = 0
    H = U.tensor(m, (1, 3), 1, 4)
    for kind in U.kinds_of(nr, nt):
        for norm in U.NORMS:
            P, s, st = _batch(_run(tr, H, 1.0, kind, norm)[0])
            want = np.zeros(24, np.uint32)
            want[4] = U.SINGULAR
            if kind == U.ZF:
                want[1::2] = U.SINGULAR
            if kind == U.ZF or norm == U.STREAM:
                want[6] = U.SINGULAR
            assert np.array_equal(st, want), (kind, norm, st)
            assert np.array_equal(U.reference_batch(m, 1.0, kind, norm)[2], want)
            flagged = want != 0
            assert not P[flagged].any() and not s[flagged].any()
            assert P[~flagged].any(axis=(1, 2)).all() and np.isfinite(s).all()
            if not want[6]:
                assert s[6, 1] == 0 and not P[6][:, 1].any() and (s[6, [0] + list(range(2, nr))] > 0).all()


# ---------------------------------------------------------------- weights, out and the wrapper's refusals

@pytest.mark.parametrize("shape", [(3, 5), (16, 3), (16, 16)], ids=lambda s: "%dx%d" % s)
def test_without_weights_the_same_sinr_bits(tr, shape):
    mats, _ = U.master_cases(*shape)
    H = U.tensor(mats, (1, 3), 3, 5)
    for kind in U.kinds_of(*shape):
        for norm in U.NORMS:
            full, _ = _run(tr, H, U.NOISE, kind, norm)
            r, after = _run(tr, H, U.NOISE, kind, norm, weights=False)   # (the guards behind the shorter buffer: _run)
            assert np.array_equal(after.view(np.float32), H.view(np.float32))
            assert r["P"] is None and full["P"] is not None
            for k in ("sinr", "status"):
                assert np.array_equal(r[k].view(np.uint8), full[k].view(np.uint8)), (kind, norm, k)
            # the poison is overwritten
            assert not np.isnan(full["P"].view(np.float32)).any() and not np.isnan(full["sinr"]).any()
        d = tr.precoder(tr.torch.from_numpy(H).to(tr.device), U.NOISE, U.KIND_NAME[kind], weights=False)
        assert d["P"] is None and d["status"].dtype == tr.torch.int32
        d = tr.precoder(tr.torch.from_numpy(H).to(tr.device), U.NOISE, kind, normalize=U.STREAM)   # (the constants)
        assert np.array_equal(d["buffer"].cpu().numpy(), full["buffer"])
    # regularization=None is the default Nr N0 / Ptot
    a = tr.precoder(tr.torch.from_numpy(H).to(tr.device), U.NOISE, "rzf", 2.0)
    b = tr.precoder(tr.torch.from_numpy(H).to(tr.device), U.NOISE, "rzf", 2.0, shape[0] * U.NOISE / 2.0)
    assert tr.torch.equal(a["buffer"], b["buffer"])
    # the power constraints hold
    P = a["P"].cpu().numpy().astype(np.complex128)
    assert np.allclose((np.abs(P) ** 2).sum((2, 3)), 2.0, rtol=1e-5)
    P = tr.precoder(tr.torch.from_numpy(H).to(tr.device), U.NOISE, "rzf", 2.0, normalize="stream")["P"].cpu().numpy()
    assert np.allclose((np.abs(P.astype(np.complex128)) ** 2).sum(2), 2.0 / shape[0], rtol=1e-5)


def test_wrapper_refuses_what_it_cannot_pass(tr):
    torch = tr.torch
    H = torch.zeros((1, 1, 2, 4, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    with pytest.raises(ValueError, match="complex64"):
        tr.precoder(H.to(torch.complex128), 1.0)
    with pytest.raises(ValueError, match="complex64"):
        tr.precoder(H.cpu(), 1.0)
    with pytest.raises(ValueError, match="expected"):
        tr.precoder(H[0], 1.0)
    with pytest.raises(ValueError, match="out must be"):
        tr.precoder(H, 1.0, out=torch.zeros(7, dtype=torch.uint8, device=tr.device))
    with pytest.raises(ValueError, match="kind"):
        tr.precoder(H, 1.0, "mmse")
    with pytest.raises(ValueError, match="normalize"):
        tr.precoder(H, 1.0, normalize="antenna")
    with pytest.raises(ValueError, match="none of"):
        tr.precoder(H, 1.0, 5)
    with pytest.raises(ValueError, match="neither"):
        tr.precoder(H, 1.0, normalize=5)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="noise"):
            tr.precoder(H, bad, "zf")
        with pytest.raises(ValueError, match="power"):
            tr.precoder(H, 1.0, "mrt", bad)
        with pytest.raises(ValueError, match="regularization"):
            tr.precoder(H, 1.0, "rzf", 1.0, bad)
    with pytest.raises(ValueError, match="nr <= nt"):
        tr.precoder(torch.zeros((1, 1, 4, 2, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0, "zf")
    with pytest.raises(ValueError, match="nr 1 .. 16"):
        tr.precoder(torch.zeros((1, 1, 17, 17, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0)
    with pytest.raises(ValueError, match="nt 1 .. 64"):
        tr.precoder(torch.zeros((1, 1, 2, 65, 2, 1, 1), dtype=torch.complex64, device=tr.device), 1.0)
    with pytest.raises(ValueError, match="must be > 0"):
        tr.precoder(torch.zeros((1, 1, 2, 4, 2, 0, 3), dtype=torch.complex64, device=tr.device), 1.0)
    # a non-contiguous view is precoded as the tensor it shows
    mats, _ = U.master_cases(4, 4)
    Hn = U.tensor(mats, (1, 2), 2, 3)
    base = torch.from_numpy(np.ascontiguousarray(np.swapaxes(Hn, 5, 6))).to(tr.device)
    a = tr.precoder(base.transpose(5, 6), 0.5)
    b = tr.precoder(torch.from_numpy(Hn).to(tr.device), 0.5)
    assert torch.equal(a["buffer"], b["buffer"])
    for kind in ("mrt", "zf", "rzf"):                                    # H = 0: singular for every kind
        for norm in ("total", "stream"):
            z = tr.precoder(H, 0.25, kind, normalize=norm)
            assert not z["P"].any() and not z["sinr"].any() and (z["status"] == abi.PC_SINGULAR).all()
