"""The pure-numpy parts of tests/planted.py (no GPU): the planted values are what the design promises, the references
agree with each other, and every check rejects a reference changed in one record."""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import planted as PL


@pytest.fixture(scope="module")
def terms():
    return PL.synthetic_terms(2, 2, 300, seed=3)


def test_delays_are_integral_and_exact_in_float32():
    n = np.arange(PL.N_MAX)
    tau = PL.delay(n)
    assert tau.dtype == np.float32
    x = tau.astype(np.float64) * PL.FS
    assert np.array_equal(x, n.astype(np.float64))
    # f tau on the carrier is a whole number of revolutions, k df tau on the DFT grid a multiple of 1 / K
    assert np.array_equal(PL.FC * tau.astype(np.float64), 3.0 * n)
    assert np.array_equal((PL.FS / 1024) * tau.astype(np.float64) * 1024, n.astype(np.float64))


def test_dopplers_give_quarter_revolutions():
    t = np.arange(8) * PL.DT
    ph = np.asarray(PL.NUS)[:, None] * t[None, :]
    assert np.array_equal(ph * 4, np.rint(ph * 4))


def test_amplitudes_are_dyadic_units():
    h = PL.mix(np.arange(4096))
    a_te, a_tm = PL.amplitudes(h)
    assert set(np.round(np.abs(a_te) ** 2, 12)) == {1.0, 4.0}
    assert set(np.abs(a_tm) ** 2) == {0.25, 1.0}
    assert np.array_equal(a_tm, a_te * 0.5j)
    for a in (a_te, a_tm):   # exact in float32: re, im in {0, +-1/2, +-1, +-2}
        assert np.array_equal(a.astype(np.complex64).astype(np.complex128), a)
        assert set(np.concatenate([a.real, a.imag])) <= {0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0}
    # all four quarter turns and both magnitudes occur
    assert len(set(np.round(a_te, 6))) == 8


def test_synthetic_terms_meet_the_design(terms):
    assert PL.design_errors(terms) == []
    link = PL.link_of(terms, 2)
    for lk in range(4):
        n = terms["n"][link == lk]
        assert np.unique(n).size == n.size   # distinct within a link


def test_design_errors_name_what_is_wrong(terms):
    U = {k: v.copy() for k, v in terms.items()}
    U["n"][5] = U["n"][6]
    U["tau"][5] = U["tau"][6]
    assert "n not distinct within a link" in PL.design_errors(U)
    U = {k: v.copy() for k, v in terms.items()}
    U["tau"][3] += 0.25 / PL.FS
    assert "fs tau is not the integer n" in PL.design_errors(U)
    U = {k: v.copy() for k, v in terms.items()}
    U["a_te"][7] *= 1.5
    assert any("a_te" in e for e in PL.design_errors(U))


def test_channel_histogram_is_the_inverse_dft_of_the_direct_sum(terms):
    nk = 1 << int(np.ceil(np.log2(terms["n"].max() + 1)))
    t = np.arange(3) * PL.DT
    H = PL.channel_direct(terms, 2, 2, PL.FC + np.arange(nk) * (PL.FS / nk), t)
    h = PL.channel_hist(terms, 2, 2, nk, t)
    assert np.abs(np.fft.ifft(H, axis=-1) - h).max() < 1e-9
    PL.check_channel_hist(H.astype(np.complex64), terms, 2, 2, nk, t)


def test_taps_histogram_is_the_sinc_sum(terms):
    t = np.arange(2) * PL.DT + 3 * PL.DT
    for nl, l_min in ((40, 0), (100, -30), (17, 250)):
        h = PL.taps_planted(terms, 2, 2, nl, l_min, t)
        assert np.array_equal(h, PL.taps_direct(terms, 2, 2, PL.FS, PL.FC, nl, l_min, t))
    # off the integer grid the sinc sum is the plain formula
    T = {k: v.copy() for k, v in terms.items()}
    T["tau"] = T["tau"] + 0.3 / PL.FS
    h = PL.taps_direct(PL.select(T, np.arange(5)), 1, 1, PL.FS, 0.0, 8, -2, np.zeros(1))
    l = np.arange(-2, 6)
    want = sum(T["a_te"][k] * np.sinc(l - T["tau"][k] * PL.FS) for k in range(5))
    assert np.abs(h[0, 0, 0, 0] - want).max() < 1e-12


def _controls(T, check):
    """check(T) passes; check(T') fails for every one-record change of PL.control_records x PL.MUTATIONS"""
    check(T)
    for name, k in PL.control_records(T):
        for how in PL.MUTATIONS:
            with pytest.raises(AssertionError):
                check(PL.mutate(T, k, how))


def test_channel_hist_check_rejects_one_record(terms):
    nk, t = 1024, np.arange(2) * PL.DT
    got = np.fft.fft(PL.channel_hist(terms, 2, 2, nk, t), axis=-1).astype(np.complex64)
    _controls(terms, lambda U: PL.check_channel_hist(got, U, 2, 2, nk, t))


def test_direct_sum_checks_reject_one_record(terms):
    f, t = 70e9 + np.arange(9) * -30e3, 0.01 + np.arange(2) * -1e-3
    got = PL.channel_direct(terms, 2, 2, f, t).astype(np.complex64)
    _controls(terms, lambda U: PL.check_close(got, PL.channel_direct(U, 2, 2, f, t), 0.05, "channel", U, 2))
    rxe = np.array([[0, 0, 0], [0, 0.002, 0]], np.float32)
    txe = np.array([[0.001, 0, 0]], np.float32)
    got = PL.array_direct(terms, 2, 2, rxe, txe, 70e9, f, t).astype(np.complex64)
    _controls(terms, lambda U: PL.check_close(got, PL.array_direct(U, 2, 2, rxe, txe, 70e9, f, t), 0.05, "array"))


def test_array_reference_reduces_to_the_channel(terms):
    f, t = PL.FC + np.arange(5) * 1e6, np.arange(2) * PL.DT
    A = PL.array_direct(terms, 2, 2, np.zeros((1, 3)), np.zeros((1, 3)), 3.5e9, f, t)
    assert np.abs(A[:, :, 0, 0] - PL.channel_direct(terms, 2, 2, f, t)).max() < 1e-9


def test_taps_check_rejects_one_record(terms):
    nl, t = int(terms["n"].max()) + 1, np.arange(3) * PL.DT
    got = PL.taps_planted(terms, 2, 2, nl, 0, t).astype(np.complex64)
    _controls(terms, lambda U: PL.check_taps_planted(got, U, 2, 2, nl, 0, t))


def test_power_check_rejects_one_record(terms):
    tau0, dtau, ld = -0.5 / PL.FS, 1.0 / PL.FS, int(terms["n"].max()) + 1
    M, pdp = PL.power_exact(terms, 2, 2, tau0, dtau, ld)
    m = np.zeros((2, 2, 2, abi.POWER_FIELDS))
    for f, v in M.items():
        m[..., f] = v
    got = {"moments": m, "pdp": pdp}
    # one term per delay bin: every bin is that term's p, the bins sum to P exactly
    assert np.count_nonzero(pdp) == 2 * terms["n"].size
    assert np.array_equal(pdp.sum(axis=-1), M[abi.POWER_P])
    _controls(terms, lambda U: PL.check_power_exact(got, U, 2, 2, tau0, dtau, ld))


def test_control_records_are_the_promised_ones(terms):
    (_, last), (_, edge) = PL.control_records(terms)
    s = ~terms["los"]
    assert terms["tx"][last] == terms["tx"][s].max()
    same = s & (terms["tx"] == terms["tx"][last])
    assert terms["bounce"][last] == terms["bounce"][same].max()
    assert terms["index"][last] == terms["index"][same & (terms["bounce"] == terms["bounce"][last])].max()
    assert terms["index"][edge] % 64 == 63 and not terms["los"][edge]


def test_failure_names_the_record(terms):
    """a kernel that loses one record: the failure names its (bounce, index)"""
    nk, t = 1024, np.zeros(1)
    k = int(np.nonzero(~terms["los"])[0][10])
    got = np.fft.fft(PL.channel_hist(PL.mutate(terms, k, "drop"), 2, 2, nk, t), axis=-1).astype(np.complex64)
    with pytest.raises(AssertionError, match=r"\(b %d, i %d\)" % (terms["bounce"][k], terms["index"][k])):
        PL.check_channel_hist(got, terms, 2, 2, nk, t)
