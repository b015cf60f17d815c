"""The design of the tests of the beam channel of path lists (tests/sparse_beam_util.py), without a device: for every
planted case the outputs are Gaussian integers whose intermediates stay below 2^24 in modulus, in float64 (the governing
quantity n max|a| ||W_rx[a]||_1 ||W_tx[b]||_1) and under a float32 mirror of the kernel's gain, G and accumulation
stages; the library's float64 reference agrees with an independent per-path loop and with beams.apply of the array
channel's reference; no live case expects an all-zero tensor; and the cases catch each wrong reading a kernel could
make."""
import numpy as np
import pytest

from hermespy_rt_amd import beams, sparse

from . import sparse_beam_util as U


def _is_gaussian_integer(B):
    return np.array_equal(B.real, np.rint(B.real)) and np.array_equal(B.imag, np.rint(B.imag))


def test_planted_codebooks_are_gaussian_integers_without_symmetry():
    wr, wt = U.codebook(5, 33, 0), U.codebook(5, 33, 1)
    for W in (wr, wt):
        assert set(np.unique(W.real)) <= {-2.0, -1.0, 0.0, 1.0, 2.0} and set(np.unique(W.imag)) <= {-2.0, -1.0, 1.0, 2.0}
        assert (W.imag != 0).all()                                    # the conjugate matters at every weight
        assert len({W[a].tobytes() for a in range(5)}) == 5           # no two beams alike
        assert not np.array_equal(W, W[:, ::-1]) and not np.array_equal(W, np.conj(W))
    assert not np.array_equal(wr, wt) and not np.array_equal(wr, np.conj(wt))
    assert not np.array_equal(wr[:, :5], wr[:, :5].T)
    S = U.codebook(4, 64, 1, fill=3, salt=2)
    assert ((S != 0).sum(axis=1) == 3).all() and (S.imag[S != 0] != 0).all()
    assert len({tuple(np.flatnonzero(S[a])) for a in range(4)}) == 4   # other positions in every beam
    H = U.one_hot_codebook(3, 4, 2, 1, 1 - 2j)
    assert H[2, 1] == 1 - 2j and (H != 0).sum() == 1


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_every_case_is_exact_in_float64_and_under_the_float32_mirror(name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    nk, nt = c["nk"], c["nt_"]
    # the governing quantity bounds every intermediate: tile sums and gains by ||W||_1, G by their product, the
    # accumulators by n max|a| times it
    assert U.governing(v, wr, wt) < U.LIMIT, (name, U.governing(v, wr, wt))
    assert float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max()) < U.LIMIT
    E = U.exact_reference(v, re, te, wr, wt, nk, nt)
    assert _is_gaussian_integer(E) and np.abs(E).max() <= U.governing(v, wr, wt) + 0.5
    live = np.minimum(v["kept"], np.uint64(c["K"])) > 0
    for rx, tx in np.argwhere(live):                                   # no live link expects an all-zero tensor
        assert E[rx, tx].any(), (name, rx, tx)
    assert not E[~live].any()
    M, peak = U.mirror_f32(v, re, te, wr, wt, U.F_A, nk, nt)
    assert peak < U.LIMIT, (name, peak)
    U.check_exact(M, E, name)


@pytest.mark.parametrize("name", ["K33", "links5", "pairs3x11", "rx33"])
def test_float64_reference_gives_the_exact_values(name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    f, t = U.grid(c["nk"], c["nt_"])
    E = U.exact_reference(v, re, te, wr, wt, c["nk"], c["nt_"])
    B, S = sparse.beam_reference(v, re, te, wr, wt, U.F_A, f, t)
    # float64 exp of a whole number of quarter revolutions up to 2^15: within 2^15 * 2^-52 * 2 pi per term
    scale = float(S.max()) * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max())
    assert np.abs(B - E).max() <= 1e-9 * max(scale, 1.0)
    assert np.array_equal(np.rint(B.real) + 1j * np.rint(B.imag), E)


def test_mirror_is_not_exact_off_the_planting():
    """the mirror rounds: off the lattice it differs from float64, so its exactness above is the planting's"""
    c = U.CASES["K33"]
    v, re, te, wr, wt = U.build(c)
    v["tau"][...] = v["tau"] * np.float32(1.37)
    re = (re * np.float32(1.013)).astype(np.float32)
    f, t = U.grid(c["nk"], c["nt_"])
    B, S = sparse.beam_reference(v, re, te, wr, wt, U.F_A, f, t)
    M, _ = U.mirror_f32(v, re, te, wr, wt, U.F_A, c["nk"], c["nt_"])
    scale = float(S.max()) * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max())
    err = np.abs(M - B).max()
    assert 0 < err <= 1e-5 * scale


def test_reference_against_the_per_path_loop_and_the_contracted_array_channel():
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
    wr = (rng.normal(size=(2, 3)) + 1j * rng.normal(size=(2, 3))).astype(np.complex64)
    wt = (rng.normal(size=(4, 2)) + 1j * rng.normal(size=(4, 2))).astype(np.complex64)
    f, t = 3.5e9 + 30e3 * np.arange(4), 1e-3 * np.arange(3)
    B, S = sparse.beam_reference(v, re, te, wr, wt, 3.5e9, f, t)
    scale = S.max() * np.abs(wr).sum(axis=1).max() * np.abs(wt).sum(axis=1).max()
    L = U.loop_reference(v, re, te, wr, wt, 3.5e9, f, t)
    assert B.shape == (2, 2, 2, 4, 2, 3, 4) and np.abs(B - L).max() <= 1e-9 * scale and np.abs(B).max() > 0
    assert not B[1, 1].any()
    H, S2 = sparse.reference(v, re, te, 3.5e9, f, t)
    assert np.array_equal(S, S2)
    assert np.abs(B - beams.apply(H, wr, wt)).max() <= 1e-12 * scale
    # slots at or beyond kept are not read
    live = np.arange(K) < v["kept"][..., None].astype(np.int64)
    w = U.copy(v)
    w["a_te"][~live] = np.nan
    w["u_tx"][~live] = np.nan
    B2, _ = sparse.beam_reference(w, re, te, wr, wt, 3.5e9, f, t)
    assert np.array_equal(B, B2)
    # beams.gains: the gains of the list's directions, as the reference forms them
    rx, tx = 0, 0
    k = int(v["kept"][rx, tx])
    g_rx = beams.gains(re, wr, v["u_rx"][rx, tx, :k], 3.5e9, conj=True)
    g_tx = beams.gains(te, wt, v["u_tx"][rx, tx, :k], 3.5e9)
    assert g_rx.shape == (2, k) and g_tx.shape == (4, k)
    amp = np.stack([v["a_te"][rx, tx, :k], v["a_tm"][rx, tx, :k]], axis=1).astype(np.complex128)
    W = np.exp(2j * np.pi * (v["freq_shift"][rx, tx, :k, None, None].astype(np.float64) * t[None, :, None]
                             - f[None, None, :] * v["tau"][rx, tx, :k, None, None].astype(np.float64)))
    assert np.abs(np.einsum("ap,bp,pq,pmk->abqmk", g_rx, g_tx, amp, W) - B[rx, tx]).max() <= 1e-9 * scale
    # one beam as a 1-D codebook, one direction as a 3-vector
    assert beams.gains(re, wr[1], v["u_rx"][rx, tx, 0], 3.5e9, conj=True).shape == (1, 1)
    assert np.allclose(beams.gains(re, wr[1], v["u_rx"][rx, tx, 0], 3.5e9, conj=True)[0, 0], g_rx[1, 0])
    with pytest.raises(ValueError, match="do not match 3 elements"):
        beams.gains(re, wt, v["u_rx"][rx, tx, :k], 3.5e9)


def test_exact_reference_against_the_per_path_loop():
    c = U.case(ntx=2, K=5, kept=[[5, 3]], nr=2, nt=3, br=2, bt=3, nk=5, nt_=2, salt=1)
    v, re, te, wr, wt = U.build(c)
    f, t = U.grid(5, 2)
    L = U.loop_reference(v, re, te, wr, wt, U.F_A, f, t)
    E = U.exact_reference(v, re, te, wr, wt, 5, 2)
    assert np.abs(L - E).max() <= 1e-6      # cmath.exp of phases up to 2^15 revolutions, weights up to |2 + 2j|


@pytest.mark.parametrize("name", U.MUTANTS)
def test_planted_cases_catch_each_wrong_reading(name):
    """every wrong reading gives a different Gaussian integer somewhere on the planted cases, so the exact comparison on
    the device catches it"""
    caught = []
    for cn in U.MUTANT_CASES:
        c = U.CASES[cn]
        v, re, te, wr, wt = U.build(c)
        E = U.exact_reference(v, re, te, wr, wt, c["nk"], c["nt_"])
        W = U.mutant(name, v, re, te, wr, wt, c["nk"], c["nt_"])
        assert _is_gaussian_integer(W)
        if not np.array_equal(E, W):
            with pytest.raises(AssertionError):
                U.check_exact(W.astype(np.complex64), E)
            caught.append(cn)
    assert len(caught) >= 2, (name, caught)


def test_one_hot_lists_and_codebooks_hit_every_index_once():
    """one live slot with one nonzero component and one-hot codebooks: the output is nonzero on that link, beam pair and
    polarisation only, there of the weights' modulus at every (m, k)"""
    nk, nt = 17, 2
    re, te = U.elements(2, 3)
    for link in range(3):
        v = U.one_hot(1, 3, link, link % 4, salt=link)
        for a in range(2):
            for b in range(3):
                wr, wt = U.one_hot_codebook(2, 2, a, (a + link) % 2, 1 + 2j), U.one_hot_codebook(3, 3, b, (b + link) % 3, 2 - 1j)
                E = U.exact_reference(v, re, te, wr, wt, nk, nt)
                assert np.array_equal(np.abs(E[0, link, a, b, (link % 4) // 2]), np.full((nt, nk), 5.0))
                E[0, link, a, b, (link % 4) // 2] = 0
                assert not E.any()
