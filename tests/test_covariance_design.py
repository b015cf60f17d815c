"""The design of the covariance tests, proven without a device (tests/covariance_util.py, hermespy_rt_amd.covariance):
the float64 reference against a brute-force contraction of single-term array channels, the exactness of the exact
planting under the device's steering rule, that every MFMA tile of every tested size carries an imaginary part, that
each wrong result a kernel could give (CU.MUTANTS) moves an entry of every link, and the host-side helpers built on the
matrices against plain numpy."""
import numpy as np
import pytest

from hermespy_rt_amd import beams
from hermespy_rt_amd import covariance as CV

from . import covariance_util as CU
from . import planted as PL

NRX, NTX = 2, 2


@pytest.fixture(scope="module")
def terms():
    """synthetic terms (a LoS term per link) with the exact planting's directions"""
    T = CU.exact_values(PL.synthetic_terms(NRX, NTX, 40, seed=3))
    assert not PL.design_errors(T), PL.design_errors(T)
    return T


def test_reference_is_the_contraction_of_single_term_array_channels():
    """R_rx = sum_p sum_j H_p[i, j] conj(H_p[i', j]) / Nt and R_tx = sum_p sum_i H_p[i, j] conj(H_p[i, j']) / Nr with
    H_p the array channel of term p alone (PL.array_direct): the cross terms of E[H H^H] vanish under independent
    uniform phases, so the expectation is the sum of the single-term products"""
    T = PL.synthetic_terms(NRX, NTX, 5, seed=1)
    lam = PL.C0 / 3.5e9
    rxe = (np.arange(3)[:, None] * np.array([[0.0, lam / 2, 0.0]])).astype(np.float32)
    txe = np.array([[0, 0, 0], [lam / 2, 0, lam / 3]], np.float32)
    fa = 3.5e9
    want_rx = np.zeros((NRX, NTX, 2, 3, 3), np.complex128)
    want_tx = np.zeros((NRX, NTX, 2, 2, 2), np.complex128)
    for k in range(T["rx"].size):
        H = PL.array_direct(PL.select(T, np.array([k])), NRX, NTX, rxe, txe, fa, [PL.FC], [0.0])[..., 0, 0]
        want_rx += np.einsum("rtijp,rtkjp->rtpik", H, H.conj()) / txe.shape[0]
        want_tx += np.einsum("rtijp,rtikp->rtpjk", H, H.conj()) / rxe.shape[0]
    for side, e, want in (("rx", rxe, want_rx), ("tx", txe, want_tx)):
        got = CU.reference(T, NRX, NTX, e, fa, side)
        assert np.abs(got - want).max() < 1e-9, side
        assert not CU.hermitian_errors(got), side
        # the trace is N sum_p p
        tr = np.trace(got, axis1=-2, axis2=-1)
        assert np.allclose(tr, e.shape[0] * CU.total_power(T, NRX, NTX), rtol=1e-12, atol=0), side


def _steering_f32(elements, u, fa):
    """the device's rule in numpy: the phase fa_c (r . u) in float64 from float32 operands, its fraction as float32
    half revolutions, then sin and cos of that many half turns (exact at multiples of 1/2: sincospi)"""
    r = np.asarray(elements, np.float32).astype(np.float64)
    u = np.asarray(u, np.float32).astype(np.float64)
    ph = (fa / PL.C0) * (u[:, None, 0] * r[None, :, 0] + u[:, None, 1] * r[None, :, 1] + u[:, None, 2] * r[None, :, 2])
    hr = (2.0 * (ph - np.rint(ph))).astype(np.float32)
    q = hr * np.float32(2)                       # quarter turns
    assert np.array_equal(q, np.rint(q)), "a phase is not a whole number of quarter revolutions"
    k = q.astype(np.int64) % 4
    cs = np.array([1, 0, -1, 0], np.float32)[k]
    sn = np.array([0, 1, 0, -1], np.float32)[k]
    return cs, sn


def test_exact_planting_is_exact_under_the_float_steering_rule(terms):
    assert CU.F_A / PL.C0 == 8.0
    e = CU.exact_elements(256)
    assert np.array_equal(e.astype(np.float64), np.rint(e.astype(np.float64) * 32) / 32)
    assert len({tuple(p) for p in e}) == 256
    cs, sn = _steering_f32(e, terms["urx"], CU.F_A)
    assert set(np.unique(cs)) <= {-1.0, 0.0, 1.0} and set(np.unique(sn)) <= {-1.0, 0.0, 1.0}
    assert np.array_equal(cs * cs + sn * sn, np.ones_like(cs))
    # ... and it is the reference's steering to the bit
    s = CV._steering(e, terms["urx"], CU.F_A)
    assert np.array_equal(s.real, cs) and np.array_equal(s.imag, sn)
    # every power is 1/4, 1 or 4 and every entry an exact multiple of 1/4 below 2^22
    p = CU.powers(terms)
    assert set(np.unique(p)) <= {0.25, 1.0, 4.0}
    R = CU.reference(terms, NRX, NTX, e, CU.F_A, "rx")
    for part in (R.real, R.imag):
        assert np.array_equal(part * 4, np.rint(part * 4)) and np.abs(part).max() < 2 ** 22
        assert np.array_equal(part.astype(np.float32).astype(np.float64), part)
    assert set(range(6)) == set(CU.axis_of(terms)), "not every axis direction is planted"


@pytest.mark.parametrize("n", CU.SIZES)
def test_elements_and_tiles_of_every_size(terms, n):
    """the elements are distinct lattice points, not mirror-symmetric in any axis, and the reference has an imaginary
    part in every 16 x 32 tile that holds an off-diagonal element (a tile that holds only diagonal elements, such as
    the last one of N = 33, is real by definition): a kernel that loses the Im rows of a tile fails at tolerance 0"""
    e = CU.exact_elements(n)
    assert len({tuple(p) for p in e}) == n and not CU.mirror_symmetric(e)
    R = CU.reference(terms, NRX, NTX, e, CU.F_A, "rx")
    off = ~np.eye(n, dtype=bool)
    for i0 in range(0, n, CU.TILE[0]):
        for k0 in range(0, n, CU.TILE[1]):
            t = (slice(i0, i0 + CU.TILE[0]), slice(k0, k0 + CU.TILE[1]))
            if not off[t].any():
                continue
            im = np.abs(R[(Ellipsis,) + t].imag).reshape(NRX, NTX, 2, -1).max(axis=-1)
            assert (im > 0).all(), (n, i0, k0)


# (a 1 x 1 matrix is sum_p p whatever the directions are: the mutants of CU.NEED_TWO_ELEMENTS start at N = 15)
@pytest.mark.parametrize("name,n", [(m, n) for m in sorted(CU.MUTANTS) for n in CU.SIZES
                                    if n > 1 or m not in CU.NEED_TWO_ELEMENTS])
def test_every_mutant_moves_an_entry_of_every_link(terms, name, n):
    e = CU.exact_elements(n)
    ref = CU.reference(terms, NRX, NTX, e, CU.F_A, "rx")
    bad = CU.mutant(name, terms, NRX, NTX, e, CU.F_A, "rx")
    moved = np.abs(bad - ref).reshape(NRX, NTX, -1).max(axis=-1)
    assert (moved > 0).all(), (name, n, moved)
    if name != "diagonal_not_real":   # (that one is caught by the diagonal's exact comparison, not by the tolerance)
        assert (moved >= 0.25).all(), (name, n, moved)
    with pytest.raises(AssertionError):
        CU.check(ref.astype(np.complex64), bad, 0.0, name)
    CU.check(ref.astype(np.complex64), ref, 0.0, name)


def test_record_mutations_move_the_reference(terms):
    e = CU.exact_elements(17)
    ref = CU.reference(terms, NRX, NTX, e, CU.F_A, "rx")
    for k in (1, terms["rx"].size - 1):
        for how in PL.MUTATIONS:
            bad = CU.reference(PL.mutate(terms, k, how), NRX, NTX, e, CU.F_A, "rx")
            assert np.abs(bad - ref).max() >= 0.25, (k, how)


# ------------------------------------------------------------------ hermespy_rt_amd.covariance against numpy
def _random_cov(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(n, 3 * n)) + 1j * rng.normal(size=(n, 3 * n))
    return a @ a.conj().T


def test_from_terms_and_correlation():
    rng = np.random.default_rng(5)
    u = rng.normal(size=(7, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    e = rng.uniform(-0.1, 0.1, (4, 3))
    p = rng.uniform(0.1, 2.0, (2, 7))
    s = beams.steering(e, u, 3.5e9)
    want = np.einsum("qp,pi,pk->qik", p, s, s.conj())
    R = CV.from_terms(p, u, e, 3.5e9)
    assert R.shape == (2, 4, 4) and np.abs(R - want).max() < 1e-12
    assert CV.from_terms(np.zeros((2, 0)), np.zeros((0, 3)), e, 3.5e9).shape == (2, 4, 4)
    with pytest.raises(ValueError):
        CV.from_terms(p[:, :3], u, e, 3.5e9)
    c = CV.correlation(R)
    d = np.sqrt(np.einsum("qii->qi", R).real)
    assert np.allclose(np.einsum("qii->qi", c), 1.0) and np.allclose(c, R / d[:, :, None] / d[:, None, :])
    assert np.array_equal(CV.correlation(np.zeros((3, 3))), np.zeros((3, 3)))


def test_kronecker_is_numpy_kron_with_the_column_vec():
    R_rx, R_tx = _random_cov(3, 1), _random_cov(2, 2)
    R_tx *= np.trace(R_rx).real / 3 / (np.trace(R_tx).real / 2)   # the traces of a link: N sum_p p
    K = CV.kronecker(R_rx, R_tx)
    assert np.allclose(K, np.kron(R_tx, R_rx) / np.trace(R_rx).real * 3)
    assert np.isclose(np.trace(K).real, 3 * 2 * np.trace(R_rx).real / 3)
    # vec stacks the columns: a rank-one H = a b^T (one path) has vec(H) = kron(b, a)
    a, b = np.array([1, 1j, -1]), np.array([1, -1j])
    one = CV.kronecker(np.outer(a, a.conj()), np.outer(b, b.conj()))
    v = np.outer(a, b).reshape(-1, order="F")
    assert np.allclose(one, np.outer(v, v.conj()))
    # batched, and a link without power
    B = CV.kronecker(np.stack([R_rx, np.zeros_like(R_rx)]), np.stack([R_tx, np.zeros_like(R_tx)]))
    assert B.shape == (2, 6, 6) and np.allclose(B[0], K) and not B[1].any()


def test_beam_power_and_eigen_beams():
    R = _random_cov(5, 3)
    W = beams.dft_codebook(5)
    want = np.array([w.conj() @ R @ w for w in W]).real
    assert np.allclose(CV.beam_power(R, W), want)
    assert np.allclose(CV.beam_power(R, W, "tx"), np.array([w @ R @ w.conj() for w in W]).real)
    assert np.allclose(CV.beam_power(np.stack([R, 2 * R]), W[:2]), np.stack([want[:2], 2 * want[:2]]))
    assert np.allclose(CV.beam_power(R, W[1]), want[1:2])
    # the long-term power of a beam is sum_p p |g(u_p)|^2 with beam_channel's gains
    rng = np.random.default_rng(9)
    u = rng.normal(size=(6, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    e = rng.uniform(-0.1, 0.1, (5, 3))
    p = rng.uniform(0.1, 2.0, 6)
    s = beams.steering(e, u, 3.5e9)
    Rp = CV.from_terms(p, u, e, 3.5e9)
    assert np.allclose(CV.beam_power(Rp, W), (p[None, :] * np.abs(W.conj() @ s.T) ** 2).sum(axis=1))
    assert np.allclose(CV.beam_power(Rp, W, "tx"), (p[None, :] * np.abs(W @ s.T) ** 2).sum(axis=1))
    lam = np.linalg.eigvalsh(R)[::-1]
    for side in ("rx", "tx"):
        V = CV.eigen_beams(R, 3, side)
        assert V.shape == (3, 5) and np.allclose(V @ V.conj().T, np.eye(3))
        assert np.allclose(CV.beam_power(R, V, side), lam[:3])
    V = CV.eigen_beams(R, 2)
    k = np.argmax(np.abs(V), axis=1)
    assert np.allclose(V[np.arange(2), k].imag, 0) and (V[np.arange(2), k].real > 0).all()
    for bad in (0, 6):
        with pytest.raises(ValueError):
            CV.eigen_beams(R, bad)
    with pytest.raises(ValueError):
        CV.beam_power(R, W[:, :4])
