"""Host side of the beamformed channel (hermespy_rt_amd/beams.py) and the references the GPU tests compare against
(tests/beam_util.py), on synthetic term lists: no device needed.

The last tests are about the GPU tests themselves: the references computed with a wrong convention (combiner not
conjugated, precoder conjugated, beam axes swapped) must differ from the right one by far more than the bound the GPU
tests allow, or those tests could not see such a kernel."""
import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_util as BU
from . import planted as PL

FA = 3.5e9
LAM = PL.C0 / FA


def _setup():
    T = PL.synthetic_terms(2, 2, 50)
    rng = np.random.default_rng(3)
    rxe = rng.uniform(-2 * LAM, 2 * LAM, (4, 3)).astype(np.float32)
    txe = rng.uniform(-2 * LAM, 2 * LAM, (6, 3)).astype(np.float32)
    wr, wt = BU.random_weights(3, 4, 1), BU.random_weights(5, 6, 2)   # Br != Bt
    f = PL.FC + np.arange(5) * 30e3
    t = np.arange(2) * PL.DT
    return T, rxe, txe, wr, wt, f, t


@pytest.mark.parametrize("n", [1, 2, 7, 16, 64])
def test_dft_codebook_is_unitary(n):
    W = beams.dft_codebook(n)
    assert W.shape == (n, n)
    assert np.abs(W @ W.conj().T - np.eye(n)).max() <= 1e-12
    assert np.abs(W.conj().T @ W - np.eye(n)).max() <= 1e-12


def test_dft_codebook_refuses_no_elements():
    with pytest.raises(ValueError):
        beams.dft_codebook(0)


def test_steering_is_the_array_factor_of_a_path():
    rng = np.random.default_rng(0)
    el = rng.uniform(-1, 1, (5, 3))
    u = rng.normal(size=(3, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s = beams.steering(el, u, FA)
    assert s.shape == (3, 5)
    want = np.exp(2j * np.pi * FA * (u @ el.T) / PL.C0)
    assert np.abs(s - want).max() <= 1e-9
    one = beams.steering(el, u[1], FA)
    assert one.shape == (5,) and np.abs(one - s[1]).max() <= 1e-12
    # matched combiner: conj(s) . s = n
    assert abs(np.vdot(s[0], s[0]) - 5) <= 1e-12


def test_apply_is_the_beam_sum_of_the_definition():
    T, rxe, txe, wr, wt, f, t = _setup()
    H = PL.array_direct(T, 2, 2, rxe, txe, FA, f, t)
    got = beams.apply(H, wr, wt)
    want, = BU.beam_direct(T, 2, 2, rxe, txe, [(wr, wt)], FA, f, t)
    assert got.shape == want.shape == (2, 2, 3, 5, 2, 2, 5)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_apply_refuses_mismatched_weights():
    H = np.zeros((1, 1, 2, 3, 2, 1, 4), np.complex64)
    with pytest.raises(ValueError):
        beams.apply(H, np.zeros((2, 3)), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        beams.apply(H, np.zeros(2), np.zeros((2, 3)))


def test_identity_codebooks_give_the_array_channel():
    T, rxe, txe, _, _, f, t = _setup()
    H = PL.array_direct(T, 2, 2, rxe, txe, FA, f, t)
    want, = BU.beam_direct(T, 2, 2, rxe, txe, [(np.eye(4), np.eye(6))], FA, f, t)
    assert np.abs(H - want).max() <= 1e-12 * np.abs(H).max()


def _swapped(B):
    """what a kernel whose row index is b * Br + a instead of a * Bt + b writes into the [Br, Bt] layout"""
    return np.ascontiguousarray(np.swapaxes(B, 2, 3)).reshape(B.shape)


@pytest.mark.parametrize("fault", ["rx_unconjugated", "tx_conjugated", "axes_swapped"])
def test_the_gpu_bound_sees_a_wrong_convention(fault):
    T, rxe, txe, wr, wt, f, t = _setup()
    assert wr.shape[0] != wt.shape[0]
    right, = BU.beam_direct(T, 2, 2, rxe, txe, [(wr, wt)], FA, f, t)
    if fault == "rx_unconjugated":
        wrong, = BU.beam_direct(T, 2, 2, rxe, txe, [(wr, wt)], FA, f, t, conj_rx=False)
    elif fault == "tx_conjugated":
        wrong, = BU.beam_direct(T, 2, 2, rxe, txe, [(wr, wt)], FA, f, t, conj_tx=True)
    else:
        wrong = _swapped(right)
    S = BU.amplitude_sums(T, 2, 2)
    err = np.abs(wrong - right).reshape(*right.shape[:5], -1).max(axis=-1)
    ratio = err / BU.bound(S, wr, wt)
    print(fault, "max |wrong - right| / bound = %.3g" % ratio.max())
    assert ratio.max() > 100.0
    # and the check itself refuses it
    with pytest.raises(AssertionError):
        BU.check(wrong.astype(np.complex64), right, S, wr, wt, what=fault)
    BU.check(right.astype(np.complex64), right, S, wr, wt, what="right")
