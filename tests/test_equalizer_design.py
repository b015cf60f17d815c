"""The design of the per-point equalizers (csrc/hrt_equalizer.{h,hip}, include/hermespy_rt.h hrt_equalizer_spec), checked
without a GPU: the form rule's mirror against the C header, the LDS layout bank by bank, the float64 reference against
numpy's pinv / solve and against the SVD, the LMMSE identity, the wrong readings of the definition that the plantings
catch, the float32 emulation against the plantings to the bit, and the emulation's worst error over the GPU tests' case
list, which fixes their tolerance constants (tests/equalizer_util.py)."""
import math
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import equalize, mimo

from . import equalizer_util as U


def test_form_rule_mirror_matches_the_c_header(tmp_path):
    prog = tmp_path / "form.c"
    prog.write_text('#include <stdio.h>\n#include "hrt_equalizer.h"\n'
                    "int main(void){for (unsigned nt = 0; nt <= 17; ++nt) for (unsigned nr = 0; nr <= 65; ++nr) "
                    'printf("%u %u %u\\n", nr, nt, hrt_equalizer_form(nr, nt)); '
                    'printf("%u %u %u %u %u\\n", HRT_EQ_THREADS, HRT_EQ_WORDS, HRT_EQ_MAX_NT, HRT_EQ_MAX_NR, '
                    "HRT_EQ_MAX_POINTS); return 0;}\n")
    exe = tmp_path / "form"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(U.REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o",
                           str(exe)])
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert lines[-1] == [U.THREADS, U.WORDS, U.MAX_NT, U.MAX_NR, U.MAX_POINTS]
    assert len(lines) - 1 == 18 * 66
    inside = 0
    for nr, nt, g in lines[:-1]:
        assert g == U.form(nr, nt), (nr, nt)
        if 1 <= nt <= 16 and 1 <= nr <= 64:
            inside += 1
            assert g in (1, 2, 4, 8, 16, 32, 64)
            mk, nk = -(-nr // g), -(-nt // g)
            assert 2 * nt * (mk + nk) <= U.WORDS                          # fits, and the next smaller g does not
            assert g == 1 or 2 * nt * (-(-nr // (g // 2)) + -(-nt // (g // 2))) > U.WORDS
        else:
            assert g == 0
    assert inside == 16 * 64
    assert U.WORDS * U.THREADS * 4 == 64 * 1024                           # static LDS of a workgroup
    # the shapes of the GPU tests sit on both sides of every switch of g
    gs = {s: U.form(*s) for s in U.SHAPES}
    for lo, hi in (((4, 4), (5, 4)), ((6, 5), (7, 5)), ((8, 7), (9, 7)), ((8, 9), (9, 9)), ((16, 11), (17, 11)),
                   ((32, 11), (33, 11)), ((16, 16), (17, 16))):
        assert gs[hi] == 2 * gs[lo], (lo, hi)
    assert sorted(set(gs.values())) == [1, 2, 4, 8, 16, 32, 64]
    for g in (2, 4, 8, 16, 32, 64):      # ... and the upper one is the smallest shape (Nr >= Nt) of its g
        best = min(((nr * nt, nt), (nr, nt)) for nt in range(1, 17) for nr in range(nt, 65) if U.form(nr, nt) == g)[1]
        assert best in U.SHAPES, (g, best)


@pytest.mark.parametrize("shape", U.SHAPES + U.PLANT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_lds_layout_has_no_bank_conflict_and_one_owner_per_word(shape):
    """every entry of both blocks: the 64 lanes of each wave touch 64 consecutive words (64 distinct banks of 4 bytes),
    every word has one owner, and the words stay inside the workgroup's array"""
    nr, nt = shape
    g = U.form(nr, nt)
    mk, nk = -(-nr // g), -(-nt // g)
    tid = np.arange(U.THREADS)
    seen = np.zeros(U.WORDS * U.THREADS, np.int64)
    for region, rows in ((0, mk), (1, nk)):
        for k in range(rows):
            for c in range(nt):
                for part in range(2):
                    w = U.lds_word(g, nt, mk, region, k, c, part, tid)
                    assert w.max() < U.WORDS * U.THREADS
                    for wave in w.reshape(-1, 64):
                        assert np.array_equal(wave - wave[0], np.arange(64))
                        assert len(set(wave % 64)) == 64
                    seen[w] += 1
    assert seen.max() == 1
    # the rows of a matrix: each has one (thread, k), inside the point's lane group
    for slot in (0, U.THREADS // g - 1):
        for rows, per in ((nr, mk), (nt, nk)):
            own = [U.owner(g, r, slot) for r in range(rows)]
            assert len(set(own)) == rows
            assert all(slot * g <= t < (slot + 1) * g and k < per for t, k in own)


def _random(rng, B, nr, nt):
    return (rng.standard_normal((B, nr, nt)) + 1j * rng.standard_normal((B, nr, nt))).astype(np.complex64)


@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (8, 3), (3, 8), (64, 16), (3, 16)], ids=lambda s: "%dx%d" % s)
def test_reference_against_numpy_and_the_svd(shape):
    nr, nt = shape
    rng = np.random.RandomState(5)
    mats = _random(rng, 12, nr, nt)
    A = mats.astype(np.complex128)
    AH = np.conj(np.swapaxes(A, 1, 2))
    for kind in U.kinds_of(nr, nt):
        n0 = 0.37
        W, sinr, status, cond = U.reference_batch(mats, n0, kind)
        assert not status.any()
        lam = n0 if kind == U.LMMSE else 0.0
        G = np.linalg.inv(AH @ A + lam * np.eye(nt))
        want = np.linalg.solve(AH @ A + lam * np.eye(nt), AH)
        assert np.allclose(W, want, rtol=1e-9, atol=1e-12)
        if kind == U.ZF:
            assert np.allclose(W, np.linalg.pinv(A), rtol=1e-9, atol=1e-12)
        rho = 1.0 / (n0 * np.real(np.diagonal(G, axis1=1, axis2=2))) - (kind == U.LMMSE)
        assert np.allclose(sinr, rho, rtol=1e-9, atol=1e-12)
        # the same SINR from the SVD (the cross-check between the two families)
        H = U.from_batch(np.concatenate([mats, mats]), (1, 1, 2, 1, 12))
        r = mimo.svd_reference(H)
        s2 = equalize.sinr_from_svd(r["sigma"], r["v"], n0, "lmmse" if kind == U.LMMSE else "zf")
        assert np.allclose(U.to_batch_vec(s2)[:12], rho, rtol=1e-8, atol=1e-10)
        if kind == U.LMMSE:      # sinr_i = d_i / (1 - d_i), d = diag(W H)
            d = np.real(np.einsum("bij,bji->bi", W, A))
            assert np.allclose(sinr, d / (1.0 - d), rtol=1e-8, atol=1e-10)
    if nr < nt:
        with pytest.raises(ValueError, match="Nr >= Nt"):
            U.reference_batch(mats, 1.0, U.ZF)


def test_reference_rules_for_singular_and_non_finite_points():
    rng = np.random.RandomState(6)
    mats = _random(rng, 6, 5, 3)
    mats[1, :, 2] = mats[1, :, 0]                    # a repeated column
    mats[2] = 0                                      # H = 0
    mats[3, 4, 1] = np.nan
    mats[4, 0, 0] = np.inf
    W, sinr, status, _ = U.reference_batch(mats, 1.0, U.ZF)
    assert list(status) == [0, U.SINGULAR, U.SINGULAR, U.NONFINITE, U.NONFINITE, 0]
    assert not W[1:5].any() and not sinr[1:5].any() and W[0].any() and sinr[5].all()
    W, sinr, status, _ = U.reference_batch(mats, 1.0, U.LMMSE)
    assert list(status) == [0, 0, 0, U.NONFINITE, U.NONFINITE, 0]
    assert W[1].any() and not W[2].any() and not sinr[2].any()
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="noise"):
            U.reference_batch(mats, bad, U.LMMSE)
    with pytest.raises(ValueError, match="kind"):
        equalize.equalizer_reference(np.zeros((1, 1, 2, 2, 2, 1, 1)), 1.0, "mmse")


def test_what_is_read_from_the_sinr():
    s = np.array([[1.0, 3.0, 7.0], [2.0, 2.0, 2.0]])
    assert np.allclose(equalize.rate(s, axis=1), [1 + 2 + 3, 3 * math.log2(3)])
    e = equalize.effective_sinr(s, 2.0, axis=1)
    assert np.allclose(e[1], 2.0) and 1.0 < e[0] < s[0].mean()
    assert np.allclose(e[0], -2.0 * math.log(np.exp(-s[0] / 2.0).mean()))
    assert np.isfinite(equalize.effective_sinr(np.array([1e6, 2e6]), 1.0)).all()
    with pytest.raises(ValueError):
        equalize.effective_sinr(s, 0.0)
    H = np.arange(2 * 3 * 4 * 2 * 2 * 1 * 2).reshape(2, 3, 4, 2, 2, 1, 2)
    up = equalize.stack_users(H, "tx")
    assert up.shape == (2, 1, 4, 6, 2, 1, 2) and np.array_equal(up[1, 0, :, 2 * 2 + 1], H[1, 2, :, 1])
    down = equalize.stack_users(H, "rx")
    assert down.shape == (1, 3, 8, 2, 2, 1, 2) and np.array_equal(down[0, 2, 1 * 4 + 3], H[1, 2, 3])
    with pytest.raises(ValueError):
        equalize.stack_users(H, "both")


def test_emulation_reproduces_the_plantings_to_the_bit():
    names = set()
    for name, kind, n0, H, W, S, st in U.exact_cases():
        for weights in (True, False):
            w, s, status = U.emulate_batch(H, n0, kind, weights)
            assert np.array_equal(status, st), name
            assert np.array_equal(s, S), (name, np.argwhere(s != S)[:4])
            assert (w is None) if not weights else np.array_equal(w, W), name
        names.add(name.split(" ")[0] + " " + name.split(" ")[1])
    assert names == {"zf permutation", "zf coupled", "lmmse triple", "lmmse wide", "lmmse zero"}
    for nr, nt, K in U.ONE_COLUMN:
        H, n0, W, S = U.one_column_case(nr, nt, K=K)
        assert H.shape[0] * H.shape[1] * 2 * H.shape[5] * H.shape[6] >= nr * nt
        r = U.emulate(H, n0, U.LMMSE)
        assert np.array_equal(r["W"], W) and np.array_equal(r["sinr"], S) and not r["status"].any()


@pytest.mark.parametrize("wrong", U.READINGS)
def test_plantings_catch_a_wrong_reading(wrong):
    """the exact expectations of the plantings agree with the definition read rightly, and at least one planting
    differs from each wrong reading by far more than float32 rounding"""
    caught = []
    for name, kind, n0, H, W, S, st in U.exact_cases():
        if name.startswith("lmmse zero") or (name.startswith("lmmse wide") and wrong == "lambda_left_out_for_lmmse"):
            continue      # (H = 0 tells nothing; without lambda a wide H has no inverse at all: caught trivially)
        Wr, Sr = U.reading(H, n0, kind)
        assert np.allclose(Wr, W, rtol=1e-6, atol=1e-9) and np.allclose(Sr, S, rtol=1e-6, atol=1e-9), name
        Ww, Sw = U.reading(H, n0, kind, wrong)
        if not (np.allclose(Ww, W, rtol=1e-3, atol=1e-6) and np.allclose(Sw, S, rtol=1e-3, atol=1e-6)):
            caught.append(name)
    assert caught, wrong
    print(wrong, "caught by", len(caught), "plantings, e.g.", caught[0])


def test_emulation_fixes_the_tolerance_constants():
    """the worst of the three measures over the GPU tests' case list, emulated: the constants are 4 x these.  The
    rank-deficient family (two columns differing by the factor 1 + 2^-12) is SINGULAR under ZF, in the emulation and
    in float64 alike."""
    worst = np.zeros(3)
    for nr, nt in U.SHAPES:
        mats, kinds = U.master_cases(nr, nt)
        assert mats.shape[0] >= max(l[0] * l[1] * 2 * T * K for l, T, K in U.grids(nr, nt))
        for kind in U.kinds_of(nr, nt):
            W, sinr, status = U.emulate_batch(mats, U.NOISE, kind)
            bd = U.bounded(kinds, kind)
            assert not status[bd].any()
            if not bd.all():
                assert (status[~bd] == U.SINGULAR).all() and not W[~bd].any() and not sinr[~bd].any()
                assert (U.reference_batch(mats[~bd], U.NOISE, kind)[2] == U.SINGULAR).all()
            m = [x.max() for x in U.measures(mats[bd], U.NOISE, kind, W[bd], sinr[bd])]
            worst = np.maximum(worst, m)
    for nr, nt in U.REPEATED_SHAPES:      # the repeated columns of the GPU tests, regular under LMMSE
        m, sing = U.repeated_cases(nr, nt)
        W, sinr, status = U.emulate_batch(m, U.REPEATED_NOISE, U.LMMSE)
        assert not status.any() and not W[4].any() and not sinr[4].any()
        reg = np.arange(24) != 4
        worst = np.maximum(worst, [x.max() for x in U.measures(m[reg], U.REPEATED_NOISE, U.LMMSE, W[reg], sinr[reg])])
        W, sinr, status = U.emulate_batch(m, U.REPEATED_NOISE, U.ZF)
        assert np.array_equal(status, np.where(sing, U.SINGULAR, 0)) and not W[sing].any() and not sinr[sing].any()
        assert np.array_equal(U.reference_batch(m, U.REPEATED_NOISE, U.ZF)[2], status)
    print("emulation's worst measures (u kappa, u kappa, u):", " ".join("%.4g" % w for w in worst))
    tol = (U.TOL_W, U.TOL_SINR, U.TOL_RESIDUAL)
    for w, e, t in zip(worst, U.EMULATION_WORST, tol):
        assert 0.97 * e <= w <= e, (w, e)                                 # (LAPACK builds differ in the last digits)
        assert 4.0 * e <= t <= 4.0 * e * 1.001, (e, t)
