"""The design of the tests of the array channel of path lists (tests/sparse_util.py), without a device: the planted
outputs are Gaussian integers, in float64 and under a float32 mirror of the kernel's U, V and S stages; the library's
float64 reference agrees with an independent per-path loop; and the planted cases catch each wrong reading a kernel
could make."""
import numpy as np
import pytest

from hermespy_rt_amd import abi, dominant, sparse

from . import sparse_util as U

# (nrx, ntx, K, kept per link, Nr, Nt, nk, nt): batch edge, pair tile edge, inner length edge, links with different kept
CASES = [
    (1, 1, 1, 1, 1, 1, 1, 1),
    (1, 1, 33, 33, 2, 3, 17, 2),
    (1, 1, 33, 32, 3, 11, 5, 1),
    (2, 3, 33, [[0, 1, 32], [33, 7, 31]], 2, 3, 17, 3),
    (1, 2, 64, [[64, 31]], 17, 1, 16, 2),
]


def _case(c, salt=0):
    nrx, ntx, K, kept, nr, nt_, nk, nt = c
    v = U.planted(nrx, ntx, K, kept, salt)
    re, te = U.elements(nr, nt_)
    return v, re, te, nk, nt


def _is_gaussian_integer(H):
    return np.array_equal(H.real, np.rint(H.real)) and np.array_equal(H.imag, np.rint(H.imag))


def test_planted_list_has_the_layout_and_the_values_it_claims():
    v = U.planted(2, 3, 33, [[0, 1, 32], [33, 7, 31]])
    assert v["buffer"].size == 2 * 3 * (16 + 72 * 33)
    assert np.array_equal(v["eligible"], v["kept"] + 3)
    for k in ("a_te", "a_tm"):
        assert set(np.unique(v[k].real)) | set(np.unique(v[k].imag)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert ((np.abs(v["a_te"]) > 0) | (np.abs(v["a_tm"]) > 0)).all()      # every slot, live or not, holds a term
    assert np.array_equal(np.abs(v["u_rx"]).sum(-1), np.ones((2, 3, 33))) and set(np.unique(v["u_rx"])) <= {-1, 0, 1}
    assert (v["bounce"][:, :, 1] == -1).all() and np.array_equal(v["u_rx"][:, :, 1], -v["u_tx"][:, :, 1])
    n = v["tau"] / np.float32(U.TAU_STEP)
    assert np.array_equal(n, np.rint(n)) and n.max() == 7 and n.min() == 0
    assert set(np.unique(v["freq_shift"])) == set(U.NUS)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_planted_outputs_are_gaussian_integers_in_float64(case):
    v, re, te, nk, nt = _case(CASES[case])
    f, t = U.grid(nk, nt)
    E = U.exact_reference(v, re, te, nk, nt)
    assert _is_gaussian_integer(E) and np.abs(E).max() <= 4 * v["tau"].shape[2]
    H, S = sparse.reference(v, re, te, U.F_A, f, t)
    # float64 exp of a whole number of quarter revolutions up to 2^15: within 2^15 * 2^-52 * 2 pi per term
    assert np.abs(H - E).max() <= 1e-9 * max(float(S.max()), 1.0)
    assert np.array_equal(np.rint(H.real) + 1j * np.rint(H.imag), E)
    if np.abs(E).max() > 0:
        assert np.abs(E).max() >= 1


@pytest.mark.parametrize("case", range(len(CASES)))
def test_planted_outputs_are_exact_under_the_float32_mirror(case):
    v, re, te, nk, nt = _case(CASES[case])
    M = U.mirror_f32(v, re, te, U.F_A, nk, nt)
    U.check_exact(M, U.exact_reference(v, re, te, nk, nt), "mirror")


def test_mirror_is_not_exact_off_the_planting():
    """the mirror rounds: off the lattice it differs from float64, so its exactness above is the planting's"""
    v, re, te, nk, nt = _case(CASES[1])
    v["tau"][...] = v["tau"] * np.float32(1.37)
    f, t = U.grid(nk, nt)
    H, S = sparse.reference(v, re, te, U.F_A, f, t)
    M = U.mirror_f32(v, re, te, U.F_A, nk, nt)
    err = np.abs(M - H).max()
    assert 0 < err <= 1e-5 * S.max()


def test_reference_against_the_per_path_loop():
    rng = np.random.default_rng(5)
    nrx, ntx, K = 2, 2, 5
    n = 14
    link = rng.integers(0, 3, n)                      # link 3 stays empty
    u = rng.normal(size=(2, n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    v = sparse.cluster_list(nrx, ntx, K, link, rng.normal(size=n) + 1j * rng.normal(size=n),
                            rng.normal(size=n) + 1j * rng.normal(size=n), rng.uniform(0, 1e-6, n),
                            rng.uniform(-200, 200, n), u[0], u[1])
    assert int(v["kept"].sum()) == sum(min(int((link == l).sum()), K) for l in range(4)) and v["kept"][1, 1] == 0
    assert (v["eligible"] > v["kept"]).any()
    re, te = rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, (2, 3)).astype(np.float32)
    f, t = 3.5e9 + 30e3 * np.arange(4), 1e-3 * np.arange(3)
    H, S = sparse.reference(v, re, te, 3.5e9, f, t)
    L = U.loop_reference(v, re, te, 3.5e9, f, t)
    assert H.shape == (2, 2, 3, 2, 2, 3, 4) and np.abs(H - L).max() <= 1e-9 * S.max() and np.abs(H).max() > 0
    assert not H[1, 1].any()
    live = np.arange(K) < v["kept"][..., None].astype(np.int64)
    assert np.allclose(S[..., 0], np.where(live, np.abs(v["a_te"]), 0).sum(-1))
    assert np.allclose(S[..., 1], np.where(live, np.abs(v["a_tm"]), 0).sum(-1))
    # slots at or beyond kept are not read
    w = U.copy(v)
    w["a_te"][~live] = np.nan
    w["tau"][~live] = np.nan
    H2, _ = sparse.reference(w, re, te, 3.5e9, f, t)
    assert np.array_equal(H, H2)
    # one element at the origin: the SISO channel of the list
    z = np.zeros((1, 3), np.float32)
    H1, _ = sparse.reference(v, z, z, 3.5e9, f, t)
    amp = np.stack([v["a_te"], v["a_tm"]], -1).astype(np.complex128)
    W = np.exp(2j * np.pi * (v["freq_shift"].astype(np.float64)[..., None, None] * t[:, None]
                             - f[None, :] * v["tau"].astype(np.float64)[..., None, None]))
    siso = np.einsum("rtpq,rtpmk,rtp->rtqmk", amp, W, live.astype(np.float64))
    assert np.abs(H1[:, :, 0, 0] - siso).max() <= 1e-9 * S.max()


def test_exact_reference_against_the_per_path_loop():
    v, re, te, nk, nt = _case(CASES[3])
    f, t = U.grid(nk, nt)
    L = U.loop_reference(v, re, te, U.F_A, f, t)
    E = U.exact_reference(v, re, te, nk, nt)
    assert np.abs(L - E).max() <= 1e-7      # cmath.exp of phases up to 2^15 revolutions


@pytest.mark.parametrize("name", U.MUTANTS)
def test_planted_cases_catch_each_wrong_reading(name):
    """every wrong reading gives a different Gaussian integer somewhere on the planted cases, so the exact comparison on
    the device catches it"""
    caught = 0
    for c in CASES[1:]:
        v, re, te, nk, nt = _case(c)
        E = U.exact_reference(v, re, te, nk, nt)
        W = U.mutant(name, v, re, te, nk, nt)
        assert _is_gaussian_integer(W)
        if not np.array_equal(E, W):
            with pytest.raises(AssertionError):
                U.check_exact(W.astype(np.complex64), E)
            caught += 1
    assert caught >= 2, name


def test_one_hot_lists_hit_every_index_once():
    """one live slot with one nonzero component: the output is nonzero on that link and polarisation only, there of
    modulus 1 at every (pair, m, k), with a phase pattern that differs between any two index positions of the pair,
    time and frequency axes"""
    nrx, ntx, nk, nt = 1, 3, 17, 2
    re, te = U.elements(2, 3)
    for link in range(3):
        for comp in range(4):
            v = U.one_hot(nrx, ntx, link, comp, salt=link)
            assert int(v["kept"].sum()) == 1
            E = U.exact_reference(v, re, te, nk, nt)
            assert np.array_equal(np.abs(E[0, link, :, :, comp // 2]), np.ones((2, 3, nt, nk)))
            E[0, link, :, :, comp // 2] = 0
            assert not E.any()


def test_dropped_power_and_cluster_list():
    v = sparse.cluster_list(1, 2, 2, [0, 0, 0, 1], [1, 2, 3, 1], [0, 0, 0, 1j], np.zeros(4), np.zeros(4),
                            np.tile([1.0, 0, 0], (4, 1)), np.tile([-1.0, 0, 0], (4, 1)))
    assert v["kept"].tolist() == [[2, 1]] and v["eligible"].tolist() == [[3, 1]]
    assert v["power"][0, 0].tolist() == [9.0, 4.0] and v["power"][0, 1, 0] == 2.0
    moments = np.zeros((1, 2, 2, abi.POWER_FIELDS))
    moments[0, 0, 0, abi.POWER_P] = 14.0
    moments[0, 1, 0, abi.POWER_P] = 1.0
    moments[0, 1, 1, abi.POWER_P] = 1.0
    d = sparse.dropped_power(v, moments)
    assert d.tolist() == [[1.0, 0.0]]
    assert np.allclose(dominant.captured_fraction(v, moments), [[13.0 / 14.0, 1.0]])
