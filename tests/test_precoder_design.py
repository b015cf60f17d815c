"""The design of the per-point precoders (csrc/hrt_precoder.{h,hip}, include/hermespy_rt.h hrt_precoder_spec), checked
without a GPU: the form rule against hrt_equalizer_form with the sides swapped, the LDS layout bank by bank, the float64
reference against a direct numpy.linalg formula, sinr_of against an explicit loop, the float32 emulation against the
plantings and against float64 to the bit, the emulation's worst error over the GPU tests' case list, which fixes their
tolerance constants (tests/precoder_util.py), and the wrong readings of the definition that the case list separates."""
import math
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import equalize, precode

from . import precoder_util as U


def test_form_rule_is_the_equalizers_with_the_sides_swapped(tmp_path):
    prog = tmp_path / "form.c"
    prog.write_text('#include <stdio.h>\n#include "hrt_precoder.h"\n'
                    "int main(void){for (unsigned nr = 0; nr <= 17; ++nr) for (unsigned nt = 0; nt <= 65; ++nt) "
                    'printf("%u %u %u %u\\n", nr, nt, hrt_precoder_form(nr, nt), hrt_equalizer_form(nt, nr)); '
                    'printf("%u %u %u %u %u\\n", HRT_PC_THREADS, HRT_PC_WORDS, HRT_PC_MAX_NR, HRT_PC_MAX_NT, '
                    "HRT_PC_MAX_POINTS); return 0;}\n")
    exe = tmp_path / "form"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(U.REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o",
                           str(exe)])
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert lines[-1] == [U.THREADS, U.WORDS, U.MAX_NR, U.MAX_NT, U.MAX_POINTS]
    assert len(lines) - 1 == 18 * 66
    inside = 0
    for nr, nt, g, g_eq in lines[:-1]:
        assert g == g_eq == U.form(nr, nt) == U.EU.form(nt, nr), (nr, nt)
        if 1 <= nr <= 16 and 1 <= nt <= 64:
            inside += 1
            assert g in (1, 2, 4, 8, 16, 32, 64)
            mk, nk = -(-nt // g), -(-nr // g)
            assert 2 * nr * (mk + nk) <= U.WORDS                          # fits, and the next smaller g does not
            assert g == 1 or 2 * nr * (-(-nt // (g // 2)) + -(-nr // (g // 2))) > U.WORDS
            assert 2 * nr <= 2 * nr * nk                                  # T's region holds the partial sums of a row of E
        else:
            assert g == 0
    assert inside == 16 * 64
    assert U.WORDS * U.THREADS * 4 == 64 * 1024                           # static LDS of a workgroup
    # the shapes of the GPU tests sit on both sides of every switch of g
    gs = {s: U.form(*s) for s in U.SHAPES}
    for lo, hi in (((4, 4), (4, 5)), ((5, 6), (5, 7)), ((7, 8), (7, 9)), ((9, 8), (9, 9)), ((11, 16), (11, 17)),
                   ((11, 32), (11, 33)), ((16, 16), (16, 17))):
        assert gs[hi] == 2 * gs[lo], (lo, hi)
    assert sorted(set(gs.values())) == [1, 2, 4, 8, 16, 32, 64]
    assert {(1, 1), (16, 16), (16, 17), (16, 64), (16, 3), (9, 8)} <= set(U.SHAPES)
    assert [s for s in U.SHAPES if U.ZF not in U.kinds_of(*s)] == [(9, 8), (16, 3)]
    for nr, nt in U.SHAPES:
        assert [l[0] * l[1] * 2 * T * K for l, T, K in U.grids(nr, nt)][-1] == U.MASTER


@pytest.mark.parametrize("shape", sorted(set(U.SHAPES + U.PLANT_SHAPES)), ids=lambda s: "%dx%d" % s)
def test_lds_layout_has_no_bank_conflict_and_one_owner_per_word(shape):
    """every entry of both blocks: the 64 lanes of each wave touch 64 consecutive words (64 distinct banks of 4 bytes),
    every word has one owner, and the words stay inside the workgroup's array; so do the partial sums of E"""
    nr, nt = shape
    g = U.form(nr, nt)
    mk, nk = -(-nt // g), -(-nr // g)
    tid = np.arange(U.THREADS)
    seen = np.zeros(U.WORDS * U.THREADS, np.int64)
    for region, rows in ((0, mk), (1, nk)):
        for k in range(rows):
            for c in range(nr):
                for part in range(2):
                    w = U.lds_word(g, nr, mk, region, k, c, part, tid)
                    assert w.max() < U.WORDS * U.THREADS
                    for wave in w.reshape(-1, 64):
                        assert np.array_equal(wave - wave[0], np.arange(64))
                        assert len(set(wave % 64)) == 64
                    seen[w] += 1
    assert seen.max() == 1
    # the accumulators of E[i][j]: word j 2 + part of T's region, T's own entry (0, j, part)
    for j in range(nr):
        for part in range(2):
            assert np.array_equal(mk * nr * 2 * U.THREADS + (j * 2 + part) * U.THREADS + tid,
                                  U.lds_word(g, nr, mk, 1, 0, j, part, tid))
    # the rows of a matrix: each has one (thread, k), inside the point's lane group
    for slot in (0, U.THREADS // g - 1):
        for rows, per in ((nt, mk), (nr, nk)):
            own = [U.owner(g, r, slot) for r in range(rows)]
            assert len(set(own)) == rows
            assert all(slot * g <= t < (slot + 1) * g and k < per for t, k in own)


def _random(rng, B, nr, nt):
    return (rng.standard_normal((B, nr, nt)) + 1j * rng.standard_normal((B, nr, nt))).astype(np.complex64)


@pytest.mark.parametrize("shape", [(1, 1), (4, 4), (3, 8), (8, 3), (16, 64), (16, 3)], ids=lambda s: "%dx%d" % s)
def test_reference_against_a_direct_formula(shape):
    nr, nt = shape
    rng = np.random.RandomState(5)
    mats = _random(rng, 12, nr, nt)
    A = mats.astype(np.complex128)
    AH = np.conj(np.swapaxes(A, 1, 2))
    n0, power, alpha = 0.37, 2.5, 0.8
    for kind in U.kinds_of(nr, nt):
        P0 = AH if kind == U.MRT else AH @ np.linalg.inv(A @ AH + (alpha if kind == U.RZF else 0.0) * np.eye(nr))
        if kind == U.RZF:      # the push-through identity: H^H (H H^H + a I)^-1 = (H^H H + a I)^-1 H^H
            assert np.allclose(P0, np.linalg.solve(AH @ A + alpha * np.eye(nt), AH), rtol=1e-9, atol=1e-12)
        if kind == U.ZF:
            assert np.allclose(P0, np.linalg.pinv(A), rtol=1e-9, atol=1e-12)
        for norm in U.NORMS:
            P, sinr, status, cond = U.reference_batch(mats, n0, kind, norm, power, alpha)
            assert not status.any()
            c = (np.abs(P0) ** 2).sum(1)
            want = P0 * (np.sqrt(power / nr / c)[:, None, :] if norm == U.STREAM else
                         np.sqrt(power / c.sum(1))[:, None, None])
            assert np.allclose(P, want, rtol=1e-9, atol=1e-12)
            # the power constraint
            if norm == U.TOTAL:
                assert np.allclose((np.abs(P) ** 2).sum((1, 2)), power)
            else:
                assert np.allclose((np.abs(P) ** 2).sum(1), power / nr)
            E = A @ want
            for b in range(12):
                for i in range(nr):
                    itf = sum(abs(E[b, i, j]) ** 2 for j in range(nr) if j != i)
                    assert math.isclose(sinr[b, i], abs(E[b, i, i]) ** 2 / (itf + n0), rel_tol=1e-9)
            if kind == U.ZF:      # no interference: E is diagonal
                off = E * (1 - np.eye(nr))
                assert np.abs(off).max() <= 1e-9 * np.abs(E).max()
            if kind == U.MRT:
                assert (cond == 1).all()
            else:
                aug = np.concatenate([AH, np.broadcast_to(np.sqrt(alpha) * np.eye(nr), (12, nr, nr))], 1) \
                    if kind == U.RZF else AH
                assert np.allclose(cond, np.linalg.cond(aug), rtol=1e-9)
    # the default regularization
    a = precode.default_regularization(nr, n0, power)
    assert a == nr * n0 / power
    P1 = U.reference_batch(mats, n0, U.RZF, U.TOTAL, power, None)[0]
    P2 = U.reference_batch(mats, n0, U.RZF, U.TOTAL, power, a)[0]
    assert np.array_equal(P1, P2)
    if nr > nt:
        with pytest.raises(ValueError, match="Nr <= Nt"):
            U.reference_batch(mats, 1.0, U.ZF, U.TOTAL)


def test_reference_rules_for_singular_and_non_finite_points():
    rng = np.random.RandomState(6)
    mats = _random(rng, 7, 3, 5)
    mats[1, 2] = mats[1, 0]                          # a repeated row
    mats[2] = 0                                      # H = 0
    mats[3, 1, 4] = np.nan
    mats[4, 0, 0] = np.inf
    mats[5, 1] = 0                                   # one user without a channel
    P, sinr, status, _ = U.reference_batch(mats, 1.0, U.ZF, U.TOTAL)
    assert list(status) == [0, U.SINGULAR, U.SINGULAR, U.NONFINITE, U.NONFINITE, U.SINGULAR, 0]
    assert not P[1:6].any() and not sinr[1:6].any() and P[0].any() and sinr[6].all()
    for kind in (U.MRT, U.RZF):
        P, sinr, status, _ = U.reference_batch(mats, 1.0, kind, U.TOTAL)
        assert list(status) == [0, 0, U.SINGULAR, U.NONFINITE, U.NONFINITE, 0, 0]
        assert P[1].any() and not P[2].any() and not sinr[2].any()
        assert sinr[5, 1] == 0 and sinr[5, 0] > 0 and not P[5][:, 1].any()     # the zero row: no power, no rate
        P, sinr, status, _ = U.reference_batch(mats, 1.0, kind, U.STREAM)
        assert list(status) == [0, 0, U.SINGULAR, U.NONFINITE, U.NONFINITE, U.SINGULAR, 0]
        assert not P[5].any() and not sinr[5].any()
        # ... and the emulation has the same rules
        for norm in U.NORMS:
            e = U.emulate_batch(mats, 1.0, kind, norm)
            r = U.reference_batch(mats, 1.0, kind, norm)
            assert np.array_equal(e[2], r[2])
            assert not e[0][e[2] != 0].any() and not e[1][e[2] != 0].any()
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="noise"):
            U.reference_batch(mats, bad, U.RZF, U.TOTAL)
        with pytest.raises(ValueError, match="power"):
            U.reference_batch(mats, 1.0, U.RZF, U.TOTAL, power=bad)
        with pytest.raises(ValueError, match="regularization"):
            U.reference_batch(mats, 1.0, U.RZF, U.TOTAL, alpha=bad)
    with pytest.raises(ValueError, match="kind"):
        precode.precoder_reference(np.zeros((1, 1, 2, 2, 2, 1, 1)), 1.0, "mmse")
    with pytest.raises(ValueError, match="normalize"):
        precode.precoder_reference(np.zeros((1, 1, 2, 2, 2, 1, 1)), 1.0, "rzf", normalize="antenna")


def test_sinr_of_against_an_explicit_loop_and_what_is_read_from_it():
    rng = np.random.RandomState(7)
    shape = (2, 3, 3, 5, 2, 2, 4)
    H = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    Pshape = (2, 3, 5, 3, 2, 2, 4)
    P = rng.standard_normal(Pshape) + 1j * rng.standard_normal(Pshape)
    got = precode.sinr_of(H, P, 0.3)
    assert got.shape == (2, 3, 3, 2, 2, 4)
    for idx in np.ndindex(2, 3, 2, 2, 4):
        a, b, p, m, k = idx
        E = H[a, b, :, :, p, m, k] @ P[a, b, :, :, p, m, k]
        for i in range(3):
            itf = sum(abs(E[i, j]) ** 2 for j in range(3) if j != i)
            assert math.isclose(got[a, b, i, p, m, k], abs(E[i, i]) ** 2 / (itf + 0.3), rel_tol=1e-12)
    # the reference's own sinr is sinr_of its own P; a stale P (of another H) scores lower under ZF
    r = precode.precoder_reference(H, 0.3, "zf")
    assert np.allclose(precode.sinr_of(H, r["P"], 0.3), r["sinr"], rtol=1e-9)
    H2 = H + 0.3 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))
    assert precode.sinr_of(H2, r["P"], 0.3).mean() < r["sinr"].mean()
    assert np.allclose(precode.sum_rate(r["sinr"]), equalize.rate(r["sinr"], 2))
    assert precode.sum_rate(r["sinr"]).shape == (2, 3, 2, 2, 4)
    with pytest.raises(ValueError, match="sinr_of"):
        precode.sinr_of(H, H, 0.3)
    with pytest.raises(ValueError, match="noise"):
        precode.sinr_of(H, P, 0.0)
    # the multi-user downlink matrix: the users stacked along Nr
    down = equalize.stack_users(H, "rx")
    assert down.shape == (1, 3, 6, 5, 2, 2, 4) and np.array_equal(down[0, 2, 1 * 3 + 2], H[1, 2, 2])
    assert precode.precoder_reference(down, 0.3)["sinr"].shape == (1, 3, 6, 2, 2, 4)


def _rounded(x64, like):
    """a float64 result rounded to float32, the rounding noise of the float64 factorisation around an exact zero
    (below 2^-40 of the largest entry) flushed first"""
    x64 = np.asarray(x64)
    big = np.abs(x64).max() if x64.size else 0.0
    return np.where(np.abs(x64) < 2.0 ** -40 * big, 0, x64).astype(like.dtype)


def test_emulation_reproduces_the_plantings_and_float64_to_the_bit():
    names = set()
    for name, kind, norm, n0, power, alpha, H, P, S, st in U.exact_cases():
        p, s, status = U.emulate_batch(H, n0, kind, norm, power, alpha)
        assert np.array_equal(status, st), name
        assert np.array_equal(s, S), (name, np.argwhere(s != S)[:4])
        assert np.array_equal(p, P), (name, np.argwhere(p != P)[:4])
        Pr, sr, str_, _ = U.reference_batch(H, n0, kind, norm, power, alpha if kind == U.RZF else None)
        assert np.array_equal(str_, st), name
        assert np.array_equal(_rounded(Pr, p), p) and np.array_equal(_rounded(sr, s), s), name
        names.add(" ".join(name.split(" ")[:2]))
    assert names == {"zf permutation", "zf coupled", "rzf triple", "mrt integers"} | {
        "zero " + k for k in ("mrt", "zf", "rzf")}
    for kind, nr, nt, K in U.ONE_ROW:
        H, n0, power, alpha, P, S = U.one_row_case(kind, nr, nt, K=K)
        assert H.shape[0] * H.shape[1] * 2 * H.shape[5] * H.shape[6] >= nr * nt
        r = U.emulate(H, n0, kind, U.TOTAL, power, alpha)
        assert np.array_equal(r["P"], P) and np.array_equal(r["sinr"], S) and not r["status"].any()
        hit = np.abs(U.to_batch(P)).sum(0) > 0
        assert hit.shape == (nt, nr) and hit.all() and (U.to_batch_vec(S) > 0).any(0).all()


def _emulated_configurations():
    """configurations() with the emulation's results; the factorisation is shared by the two norms"""
    last = None
    for name, mats, kind, norm, n0, power, alpha in U.configurations():
        key = name.rsplit(" ", 1)[0]
        if last is None or last[0] != key:
            last = (key, U.emulate_p0(mats, kind, alpha))
        yield (name, mats, kind, norm, n0, power, alpha) + U.emulate_finish(mats, last[1], n0, norm, power)


def test_emulation_fixes_the_tolerance_constants():
    """the worst of the two measures over the GPU tests' case list, emulated: the constants are 4 x these.  The
    rank-deficient family (two rows differing by the factor 1 + 2^-12) is SINGULAR under ZF, in the emulation and in
    float64 alike."""
    worst = np.zeros(2)
    seen = set()
    for name, mats, kind, norm, n0, power, alpha, P, sinr, status in _emulated_configurations():
        assert not status.any(), name
        worst = np.maximum(worst, [x.max() for x in U.measures(mats, n0, kind, norm, power, alpha, P, sinr)])
        seen.add(name)
    assert len(seen) == sum(2 * len(U.kinds_of(*s)) for s in U.SHAPES) + 2 * len(U.HEAVY_SHAPES)
    for nr, nt in U.SHAPES:
        mats, kinds = U.master_cases(nr, nt)
        assert mats.shape == (U.MASTER, nr, nt)
        rest = ~U.bounded(kinds, U.ZF)
        if nr >= 2 and U.ZF in U.kinds_of(nr, nt):
            assert rest.sum() == U.MASTER // 4
            for norm in U.NORMS:
                P, sinr, status = U.emulate_batch(mats[rest], U.NOISE, U.ZF, norm)
                assert (status == U.SINGULAR).all() and not P.any() and not sinr.any()
                assert (U.reference_batch(mats[rest], U.NOISE, U.ZF, norm)[2] == U.SINGULAR).all()
        for kind in (U.MRT, U.RZF):
            assert U.bounded(kinds, kind).all()
    print("emulation's worst measures (u kappa):", " ".join("%.4g" % w for w in worst))
    for w, e, t in zip(worst, U.EMULATION_WORST, (U.TOL_P, U.TOL_SINR)):
        assert 0.97 * e <= w <= e, (w, e)                                 # (LAPACK builds differ in the last digits)
        assert 4.0 * e <= t <= 4.0 * e * 1.001, (e, t)


READING_SHAPES = ((4, 4), (5, 7), (9, 8), (11, 16))


def _reading_configurations(wrong):
    """the standard-normal matrices of the case list a reading is held against: the bounded cases' constants, or, for
    the identity-based E, the heavily regularised set"""
    if wrong == "e_from_identity_in_float":
        for nr, nt in U.HEAVY_SHAPES:
            mats, alpha = U.heavy_cases(nr, nt)
            for norm in U.NORMS:
                yield mats, U.RZF, norm, alpha
        return
    for nr, nt in READING_SHAPES:
        mats, kinds = U.master_cases(nr, nt)
        for kind in U.kinds_of(nr, nt):
            for norm in U.NORMS:
                yield mats[kinds == 0][:24], kind, norm, U.default_alpha(nr) if kind == U.RZF else 0.0


@pytest.mark.parametrize("wrong", U.READINGS)
def test_case_list_separates_a_wrong_reading(wrong):
    """the definition read rightly (through the Gram matrix, in float64) agrees with the reference to 10^-3 of the
    bounds; read wrongly, the typical (median) matrix of every configuration the reading applies to misses a bound by
    more than a factor of 100.  The last reading is no misreading but a method: E from the identity of the
    factorisation, with only its one subtraction rounded to float32 (a kernel would add T's own error).  In every
    configuration of the heavily regularised set the typical matrix misses a bound with it: the medians are 1.2 to 2.6
    bounds, single matrices 0.8 to 6 (the bounds are 4 x the worst of all shapes; this cancellation costs 2^8 / Nr)."""
    applied = 0
    for mats, kind, norm, alpha in _reading_configurations(wrong):
        args = (mats, U.NOISE, kind, norm, U.POWER, alpha)
        right = U.reading(*args)
        m = U.measures(*args, *right)
        assert m[0].max() <= 1e-3 * U.TOL_P and m[1].max() <= 1e-3 * U.TOL_SINR
        got = U.reading(*args, wrong)
        if got is None:
            continue
        applied += 1
        m = U.measures(*args, *got)
        ratio = np.maximum(m[0] / U.TOL_P, m[1] / U.TOL_SINR)
        if wrong == "e_from_identity_in_float":
            assert np.median(ratio) > 1.2, (wrong, mats.shape, kind, norm, np.median(ratio))
            continue
        assert np.median(ratio) > 100, (wrong, mats.shape, kind, norm, np.median(ratio))
    assert applied, wrong
