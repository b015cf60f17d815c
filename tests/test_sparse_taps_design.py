"""The design of the tests of the array taps of path lists (tests/sparse_taps_util.py), without a device: the planted
outputs are Gaussian integers, in float64 and under a float32 mirror of the kernel's U, sinc and MFMA-order stages; the
library's float64 reference (sparse.taps_reference) agrees with an independent per-path loop; and the planted cases
catch each wrong reading a kernel could make."""
import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import sparse_taps_util as U

# (nrx, ntx, K, kept per link, Nr, Nt, l_min, L, nt): the batch edge, the form switch (Nr Nt T = 12 / 13), a row block
# that begins inside a pair, tap windows left of, across and right of zero, links with different kept
CASES = [
    (1, 1, 1, 1, 1, 1, 0, 1, 1),
    (1, 1, 33, 33, 2, 3, -3, 17, 2),
    (1, 1, 33, 32, 3, 11, 5, 5, 1),
    (2, 3, 33, [[0, 1, 32], [33, 7, 31]], 2, 3, -40, 17, 3),
    (1, 2, 64, [[64, 31]], 13, 1, 2, 16, 1),
    (1, 1, 40, 40, 3, 8, -1, 9, 3),
]


def _case(c, salt=0):
    nrx, ntx, K, kept, nr, nt_, l_min, L, nt = c
    v = U.planted(nrx, ntx, K, kept, l_min, L, salt)
    re, te = U.elements(nr, nt_)
    return v, re, te, l_min, L, nt


def _is_gaussian_integer(h):
    return np.array_equal(h.real, np.rint(h.real)) and np.array_equal(h.imag, np.rint(h.imag))


def test_planted_list_has_the_delays_it_claims():
    l_min, L = -40, 17
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]], l_min, L)
    q = U.delays(v)
    assert np.array_equal(v["tau"], (q * U.TAU_STEP).astype(np.float32))
    assert {l_min - 1, l_min, l_min + L - 1, l_min + L} <= set(np.unique(q).tolist())     # both edges, one beyond each
    assert ((q >= l_min) & (q < l_min + L)).mean() > 0.3 and ((q < l_min) | (q >= l_min + L)).mean() > 0.2
    assert np.array_equal(v["eligible"], v["kept"] + 3)
    assert ((np.abs(v["a_te"]) > 0) | (np.abs(v["a_tm"]) > 0)).all()      # every slot, live or not, holds a term
    assert U.FS * U.TAU_STEP == 1.0 and U.FC * U.TAU_STEP == 0.25


def test_sinc_weights_of_integer_delays_are_one_and_signed_zeros():
    l = np.arange(-9, 12)
    for q in (-9, -1, 0, 3, 11, 12, -10, 1 << 20):
        w = U.sinc_weights_f32(U.FS, np.float32(q * U.TAU_STEP), l)
        assert w.dtype == np.float32 and np.array_equal(w, (l == q).astype(np.float32))     # (== : either zero)
    # off the lattice the mirror follows the float64 sinc within the bound of tests/sinc_util.py
    for x in (2.5, -0.25, 3.0 + 2.0 ** -12, 7.75):
        w = U.sinc_weights_f32(U.FS, np.float32(x * U.TAU_STEP), l)
        assert np.abs(w - np.sinc(l - x)).max() <= 10 * 2.0 ** -24


@pytest.mark.parametrize("case", range(len(CASES)))
def test_planted_outputs_are_gaussian_integers_in_float64(case):
    v, re, te, l_min, L, nt = _case(CASES[case])
    E = U.exact_reference(v, re, te, l_min, L, nt)
    assert _is_gaussian_integer(E) and np.abs(E).max() <= 4 * v["tau"].shape[2]
    h, S = sparse.taps_reference(v, re, te, U.F_A, U.FS, U.FC, l_min + np.arange(L), U.T0 + U.DT * np.arange(nt))
    # float64: the phases are whole quarter revolutions below 2^12, the sinc of a nonzero integer is below 4e-17
    assert np.abs(h - E).max() <= 1e-9 * max(float(S.max()), 1.0)
    assert np.array_equal(np.rint(h.real) + 1j * np.rint(h.imag), E)
    if v["kept"].max() >= 8:
        assert np.abs(E).max() >= 1


@pytest.mark.parametrize("case", range(len(CASES)))
def test_planted_outputs_are_exact_under_the_float32_mirror(case):
    v, re, te, l_min, L, nt = _case(CASES[case])
    M = U.mirror_f32(v, re, te, U.F_A, U.FS, U.FC, l_min, L, nt)
    U.check_exact(M, U.exact_reference(v, re, te, l_min, L, nt), "mirror")


def test_mirror_is_not_exact_off_the_planting():
    """the mirror rounds: off the lattice it differs from float64, so its exactness above is the planting's"""
    v, re, te, l_min, L, nt = _case(CASES[1])
    v["tau"][...] = v["tau"] * np.float32(1.37)
    h, S = sparse.taps_reference(v, re, te, U.F_A, U.FS, U.FC, l_min + np.arange(L), U.T0 + U.DT * np.arange(nt))
    M = U.mirror_f32(v, re, te, U.F_A, U.FS, U.FC, l_min, L, nt)
    err = np.abs(M - h).max()
    assert 0 < err <= 1e-5 * S.max()


def test_reference_against_the_per_path_loop():
    rng = np.random.default_rng(7)
    nrx, ntx, K = 2, 2, 5
    n = 14
    link = rng.integers(0, 3, n)                      # link 3 stays empty
    u = rng.normal(size=(2, n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    v = sparse.cluster_list(nrx, ntx, K, link, rng.normal(size=n) + 1j * rng.normal(size=n),
                            rng.normal(size=n) + 1j * rng.normal(size=n), rng.uniform(0, 1e-6, n),
                            rng.uniform(-200, 200, n), u[0], u[1])
    assert v["kept"][1, 1] == 0 and (v["eligible"] > v["kept"]).any()
    re, te = rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, (2, 3)).astype(np.float32)
    fs, fc, l, t = 30.72e6, 3.5e9, np.arange(-3, 40), 1e-3 * np.arange(3)
    h, S = sparse.taps_reference(v, re, te, 3.5e9, fs, fc, l, t)
    W = U.loop_reference(v, re, te, 3.5e9, fs, fc, l, t)
    assert h.shape == (2, 2, 3, 2, 2, 3, 43) and np.abs(h - W).max() <= 1e-9 * S.max() and np.abs(h).max() > 0
    assert not h[1, 1].any()
    live = np.arange(K) < v["kept"][..., None].astype(np.int64)
    assert np.allclose(S[..., 0], np.where(live, np.abs(v["a_te"]), 0).sum(-1))
    assert np.allclose(S[..., 1], np.where(live, np.abs(v["a_tm"]), 0).sum(-1))
    # slots at or beyond kept are not read
    w = U.copy(v)
    w["a_te"][~live] = np.nan
    w["tau"][~live] = np.nan
    h2, _ = sparse.taps_reference(w, re, te, 3.5e9, fs, fc, l, t)
    assert np.array_equal(h, h2)
    # its DTFT inside the band is sparse.reference at f_c + f (the sinc is the band-limited interpolation kernel): a
    # wide window, so the truncated tails stay below 1e-2 S
    lw = np.arange(-2000, 2040)
    hw, _ = sparse.taps_reference(v, re, te, 3.5e9, fs, fc, lw, t)
    f = np.array([-0.2, 0.0, 0.3]) * fs
    D = np.einsum("...l,lk->...k", hw, np.exp(-2j * np.pi * lw[:, None] * f[None, :] / fs))
    H, _ = sparse.reference(v, re, te, 3.5e9, fc + f, t)
    assert np.abs(D - H).max() <= 1e-2 * S.max()


def test_exact_reference_against_the_per_path_loop():
    v, re, te, l_min, L, nt = _case(CASES[3])
    W = U.loop_reference(v, re, te, U.F_A, U.FS, U.FC, l_min + np.arange(L), U.T0 + U.DT * np.arange(nt))
    E = U.exact_reference(v, re, te, l_min, L, nt)
    assert np.abs(W - E).max() <= 1e-7


@pytest.mark.parametrize("name", U.MUTANTS)
def test_planted_cases_catch_each_wrong_reading(name):
    """every wrong reading gives a different Gaussian integer somewhere on the planted cases, so the exact comparison on
    the device catches it"""
    caught = 0
    for c in CASES[1:]:
        v, re, te, l_min, L, nt = _case(c)
        E = U.exact_reference(v, re, te, l_min, L, nt)
        W = U.mutant(name, v, re, te, l_min, L, nt)
        assert _is_gaussian_integer(W) and W.shape == E.shape
        if not np.array_equal(E, W):
            with pytest.raises(AssertionError):
                U.check_exact(W.astype(np.complex64), E)
            caught += 1
    assert caught >= 2, name


def test_one_hot_lists_hit_every_index_once():
    """one live slot with one nonzero component at tap q: the output is nonzero on that link, polarisation and tap only,
    there of modulus 1 at every (pair, m)"""
    nrx, ntx, l_min, L, nt = 1, 3, -2, 5, 2
    re, te = U.elements(2, 3)
    for link in range(3):
        for comp in range(4):
            for k in range(L):
                v = U.one_hot(nrx, ntx, link, comp, l_min + k, salt=link)
                assert int(v["kept"].sum()) == 1
                E = U.exact_reference(v, re, te, l_min, L, nt)
                assert np.array_equal(np.abs(E[0, link, :, :, comp // 2, :, k]), np.ones((2, 3, nt)))
                E[0, link, :, :, comp // 2, :, k] = 0
                assert not E.any()
