"""Received signals on planted tensors (Tracer.apply_taps -> hrt_propagate; csrc/hrt_propagate.hip), no trace: the
device result against the definition at tolerance 0 on an integer planting over a covering set of shapes, one-hot
pairs that pin every index map, standard-normal tensors under the derived float32 bound at every output element,
poison and determinism.  The cases and their design: tests/propagate_util.py, tests/test_propagate_design.py."""
import numpy as np
import pytest

from hermespy_rt_amd import propagate as pg

from . import configs as K
from . import propagate_util as U
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tr():
    t = _tracer(K.small(K.C1, 64))   # apply_taps reads only its two tensors: nothing is traced
    yield t
    t.close()


def _dev(tr, a):
    return tr.torch.from_numpy(np.ascontiguousarray(a)).to(tr.device)


def _apply(tr, h, x, l_min, S, n_out, **kw):
    y = tr.apply_taps(_dev(tr, h), _dev(tr, x), l_min, S, n_out, **kw)
    return y.cpu().numpy()


def test_exact_planting_at_tolerance_zero(tr):
    cases = U.exact_cases()
    print("exact cases:", len(cases))
    bad = []
    for c in cases:
        h, x = U.plant_integers(c)
        ref = U.reference(c, h, x)
        y = _apply(tr, h, x, c["l_min"], c["S"], c["n_out"])
        assert y.shape == ref.shape and y.dtype == np.complex64
        if not np.array_equal(y, ref.astype(np.complex64)):
            bad.append((c["choice"], int((y != ref).sum())))
    assert not bad, bad


def test_taps_and_signal_without_element_axes(tr):
    """taps() output [nrx, ntx, 2, M, L] and a signal [ntx, N] are the case Nr = Nt = 1"""
    c = dict(nrx=2, nr=1, ntx=3, nt=1, L=5, N=17, n_out=21, l_min=0, S=None, M=1)
    h, x = U.plant_integers(c)
    ref = U.reference(c, h, x)
    y = tr.apply_taps(_dev(tr, h[:, :, 0, 0]), _dev(tr, x[:, 0])).cpu().numpy()
    assert np.array_equal(y, ref.astype(np.complex64))
    assert y.shape == (2, 1, 2, pg.default_num_out(17, 5, 0))


def test_one_hot_pairs(tr):
    s = U.ONE_HOT_SHAPE
    for S, i in U.one_hot_cases():
        h, x = U.one_hot_tensors(i)
        y = _apply(tr, h, x, 0, S, s["n_out"])
        want = np.zeros((s["nrx"], s["nr"], 2, s["n_out"]), np.complex64)
        at = U.one_hot_expected(S, i)
        if at is not None:
            want[at] = 1
        assert np.array_equal(y, want), (S, i, np.argwhere(y != want)[:4])


@pytest.mark.parametrize("which", [U.MFMA, U.GENERAL])
def test_real_valued_within_the_derived_bound(tr, which):
    s = U.REAL_SHAPE
    S, M = U.REAL_BLOCKS[which]
    assert U.form(M, S) == which
    assert 2 * s["nrx"] * s["nr"] == 24 and s["ntx"] * s["nt"] * s["L"] == 2 * 3 * 37 and s["n_out"] == 200
    h, x = U.plant_normal(s, M, 5)
    ref = pg.apply_taps_reference(h, x, s["l_min"], S, s["n_out"])
    bound = pg.error_bound(h, x, s["l_min"], S, s["n_out"])
    assert (bound > 0).all()   # no element is compared against zero
    y = _apply(tr, h, x, s["l_min"], S, s["n_out"]).astype(np.complex128)
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    print("%s: largest error / bound %.4f, largest error %.3g" % (which, (err / bound).max(), err.max()))
    assert (err <= bound).all(), np.argwhere(err > bound)[:4]


def _poison_case():
    return dict(nrx=1, nr=3, ntx=2, nt=1, L=5, N=40, n_out=40, l_min=0, S=16, M=4)   # blocks 0 .. 2 used, 3 unused


@pytest.mark.parametrize("S", [16, 15])   # MFMA form, general form
def test_poison(tr, S):
    torch = tr.torch
    c = dict(_poison_case(), S=S)
    assert (c["n_out"] - 1) // S == 2 and U.form(c["M"], S) == (U.MFMA if S == 16 else U.GENERAL)
    h, x = U.plant_integers(c)
    ref = U.reference(c, h, x).astype(np.complex64)
    # NaN in the output buffer is overwritten
    out = torch.full((c["nrx"], c["nr"], 2, c["n_out"]), float("nan"), dtype=torch.complex64, device=tr.device)
    got = tr.apply_taps(_dev(tr, h), _dev(tr, x), 0, S, c["n_out"], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(out.cpu().numpy(), ref)
    # NaN in the taps of a block no sample uses does not reach y
    hp = h.copy()
    hp[:, :, :, :, :, 3] = np.nan
    assert np.array_equal(_apply(tr, hp, x, 0, S, c["n_out"]), ref)
    # accumulate twice = 2 x (exact on integers)
    tr.apply_taps(_dev(tr, h), _dev(tr, x), 0, S, c["n_out"], out=out, accumulate=True)
    assert np.array_equal(out.cpu().numpy(), 2 * ref)
    # a view passed as `out` is written in place, its neighbours are not
    big = torch.full((3, c["nrx"], c["nr"], 2, c["n_out"]), 7.0, dtype=torch.complex64, device=tr.device)
    tr.apply_taps(_dev(tr, h), _dev(tr, x), 0, S, c["n_out"], out=big[1])
    b = big.cpu().numpy()
    assert np.array_equal(b[1], ref) and (b[0] == 7).all() and (b[2] == 7).all()


def test_all_zero_outputs_are_written(tr):
    """windows shifted off the signal: the sum is empty everywhere and y = 0 + 0j is written, not skipped"""
    torch = tr.torch
    for S, M in ((16, 2), (5, 4)):
        for l_min in (-(40 + 5), 40 + 40):
            c = dict(nrx=1, nr=2, ntx=1, nt=2, L=5, N=40, n_out=44, l_min=l_min, S=S, M=M)
            h, x = U.plant_integers(c)
            out = torch.full((1, 2, 2, 44), float("nan"), dtype=torch.complex64, device=tr.device)
            tr.apply_taps(_dev(tr, h), _dev(tr, x), l_min, S, 44, out=out)
            assert not out.cpu().numpy().any()


def test_two_calls_give_the_same_bits(tr):
    s = U.REAL_SHAPE
    for which in (U.MFMA, U.GENERAL):
        S, M = U.REAL_BLOCKS[which]
        h, x = U.plant_normal(s, M, 9)
        a = _apply(tr, h, x, 0, S, s["n_out"])
        b = _apply(tr, h, x, 0, S, s["n_out"])
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_two_forms_agree_on_the_exact_planting(tr):
    """one block in use (n_out <= 16): S = 16 runs the MFMA form, S = 17 the general form, on the same taps"""
    c = dict(nrx=3, nr=3, ntx=2, nt=3, L=17, N=15, n_out=16, l_min=-3, S=16, M=2)
    assert U.form(2, 16) == U.MFMA and U.form(2, 17) == U.GENERAL
    h, x = U.plant_integers(c)
    a = _apply(tr, h, x, c["l_min"], 16, c["n_out"])
    b = _apply(tr, h, x, c["l_min"], 17, c["n_out"])
    assert np.array_equal(a, b) and np.array_equal(a, U.reference(c, h, x).astype(np.complex64)) and a.any()


def test_long_windows_cross_the_staged_tap_chunks(tr):
    """L beyond one LDS window of taps (HRT_PG_LC), odd, over two workgroups of columns"""
    c = dict(nrx=1, nr=1, ntx=1, nt=2, L=2 * U.LC + 3, N=300, n_out=U.COLS + 70, l_min=-7, S=None, M=1)
    h, x = U.plant_integers(c)
    assert np.array_equal(_apply(tr, h, x, c["l_min"], None, c["n_out"]), U.reference(c, h, x).astype(np.complex64))


def test_invalid_arguments_raise_value_error(tr):
    torch = tr.torch
    h = torch.zeros((1, 1, 1, 1, 2, 2, 4), dtype=torch.complex64, device=tr.device)
    x = torch.zeros((1, 1, 8), dtype=torch.complex64, device=tr.device)
    with pytest.raises(ValueError, match="samples_per_block=None"):
        tr.apply_taps(h, x)
    with pytest.raises(ValueError, match="must be > 0"):
        tr.apply_taps(h, x, samples_per_block=0)
    with pytest.raises(ValueError, match="must be > 0"):
        tr.apply_taps(h, x, samples_per_block=4, num_out=0)
    with pytest.raises(ValueError, match="tap indices"):
        tr.apply_taps(h, x, l_min=(1 << 24) + 1, samples_per_block=4)
    with pytest.raises(ValueError, match="TX ports"):
        tr.apply_taps(h, torch.zeros((2, 1, 8), dtype=torch.complex64, device=tr.device), samples_per_block=4)
    with pytest.raises(ValueError, match="complex64"):
        tr.apply_taps(h, x.to(torch.complex128), samples_per_block=4)
    with pytest.raises(ValueError, match="accumulate=True needs"):
        tr.apply_taps(h, x, samples_per_block=4, accumulate=True)
    with pytest.raises(ValueError, match="out must be"):
        tr.apply_taps(h, x, samples_per_block=4, out=torch.zeros((1, 1, 2, 5), dtype=torch.complex64,
                                                                 device=tr.device))
