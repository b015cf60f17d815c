"""Design of the SVD tests (tests/svd_util.py, hermespy_rt_amd.mimo), no GPU: the float32 emulation of the kernel's
rotation sequence against float64 numpy, the sweep cap and the tolerance constant it sets, the form rule and the LDS
layout of csrc/hrt_svd.h, the exact plantings, eight wrong results the checks catch, and mimo.py against brute force."""
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import mimo

from . import svd_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_EMU = {}


def emulated(nr, nt):
    """the emulation of one shape's whole case list, computed once -> (mats, kinds, sigma, u, v, sweeps)"""
    if (nr, nt) not in _EMU:
        mats, kinds = U.master_cases(nr, nt)
        _EMU[nr, nt] = (mats, kinds) + U.emulate_batch(mats)
    return _EMU[nr, nt]


# ---------------------------------------------------------------- the form rule and the layout

def test_form_matches_the_header_and_covers_every_group(tmp_path):
    pairs = [(nr, nt) for nr in range(0, 67) for nt in range(0, 19)] + [(nt, nr) for nr in (33, 64, 65) for nt in (1, 16, 17)]
    prog = tmp_path / "f.c"
    prog.write_text('#include <stdio.h>\n#include "hrt_svd.h"\nint main(void){\n' +
                    "".join('printf("%%u ", hrt_svd_form(%du, %du));\n' % p for p in pairs) +
                    'printf("\\n%u %u %u %u %u %u\\n", HRT_SVD_THREADS, HRT_SVD_WORDS, HRT_SVD_MAX_SHORT, HRT_SVD_MAX_LONG, '
                    "HRT_SVD_MAX_POINTS, HRT_SVD_MAX_SWEEPS);return 0;}\n")
    exe = tmp_path / "f"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    assert [int(v) for v in out[0].split()] == [U.form(*p) for p in pairs]
    assert [int(v) for v in out[1].split()] == [U.THREADS, U.WORDS, U.MAX_SHORT, U.MAX_LONG, U.MAX_POINTS, U.MAX_SWEEPS]
    # one shape per g, and the shapes of the GPU tests reach every g in both orientations
    table = {(4, 4): 1, (8, 4): 2, (8, 8): 4, (16, 8): 8, (16, 16): 16, (32, 16): 32, (64, 16): 64}
    for (m, n), g in table.items():
        assert U.form(m, n) == g and U.form(n, m) == g
    assert {U.form(*s) for s in U.SHAPES} == {1, 2, 4, 8, 16, 32, 64}
    assert any(nr < nt for nr, nt in U.SHAPES) and any(max(s) % U.form(*s) for s in U.SHAPES)


def test_lds_fits_and_every_word_has_one_owner():
    """a workgroup's matrices fill at most 64 KB, and no two (thread, entry) pairs share a word"""
    for nr in range(1, U.MAX_LONG + 1):
        for nt in range(1, U.MAX_SHORT + 1):
            g = U.form(nr, nt)
            m, n = max(nr, nt), min(nr, nt)
            mk, nk = -(-m // g), -(-n // g)
            assert g and (g == 1 or 2 * n * (-(-m // (g // 2)) + -(-n // (g // 2))) > U.WORDS)   # the smallest g
            words = 2 * n * (mk + nk)
            assert words <= U.WORDS and words * U.THREADS * 4 <= 64 << 10
    for nr, nt in ((5, 3), (17, 16), (64, 16)):
        g = U.form(nr, nt)
        m, n = max(nr, nt), min(nr, nt)
        mk, nk = -(-m // g), -(-n // g)
        seen = set()
        for region, rows in ((0, mk), (1, nk)):
            for k in range(rows):
                for c in range(n):
                    for part in range(2):
                        for tid in (0, 1, 63, 64, 255):
                            w = U.lds_word(g, n, mk, region, k, c, part, tid)
                            assert w not in seen and 0 <= w < U.WORDS * U.THREADS
                            seen.add(w)
        # the stage-in's writer finds the owner's word: row r of slot s belongs to thread s g + r % g, entry r // g
        for slot in (0, U.THREADS // g - 1):
            for r in range(m):
                tid, k = U.owner(g, r, slot)
                assert tid // g == slot and tid % g == r % g and k * g + tid % g == r and tid < U.THREADS


def test_sweep_reads_are_free_of_bank_conflicts():
    """ds_read_b32 / ds_write_b32 serve a wave in two halves of 32 lanes over 32 banks: for every entry of A and of V
    the 32 lanes of a half touch 32 different banks (the 64 lanes of a wave touch 64 consecutive words)"""
    for nr, nt in U.SHAPES:
        g = U.form(nr, nt)
        m, n = max(nr, nt), min(nr, nt)
        mk, nk = -(-m // g), -(-n // g)
        for region, rows in ((0, mk), (1, nk)):
            for k in range(rows):
                for c in range(n):
                    for part in range(2):
                        for wave in range(U.THREADS // 64):
                            words = [U.lds_word(g, n, mk, region, k, c, part, 64 * wave + lane) for lane in range(64)]
                            assert words == list(range(words[0], words[0] + 64))
                            banks = [w % 32 for w in words]
                            assert len(set(banks[:32])) == 32 and len(set(banks[32:])) == 32


# ---------------------------------------------------------------- the emulation, the cap and the constant

@pytest.mark.parametrize("shape", U.SHAPES, ids=lambda s: "%dx%d" % s)
def test_emulation_stays_within_a_quarter_of_the_constant(shape):
    mats, kinds, s, u, v, sw = emulated(*shape)
    worst = U.check(mats, s, u, v, sw, const=U.TOL_CONST / 4.0, relative=kinds != 3)
    print("shape %s g %d: sweeps <= %d, measures in u:" % (shape, U.form(*shape), int(sw.max())),
          " ".join("%.2f" % w for w in worst))
    # the cap: twice the worst sweep count, and at least 16
    assert U.MAX_SWEEPS >= 16 and U.MAX_SWEEPS >= 2 * int(sw.max())
    # the kinds are there, and do what they are for
    n = min(shape)
    if n >= 2:
        r1 = kinds == 1
        assert r1.any() and (mimo.rank(s[r1], *shape, axis=1) == 1).all()
        assert np.allclose(s[r1, 0], np.sqrt(shape[0] * shape[1]), rtol=1e-6)
        assert not (u if shape[0] >= shape[1] else v)[r1][:, :, 1:].any()       # n - 1 null columns: exact zeros
        assert (kinds == 2).any()
    if n >= 3:
        p = kinds == 3
        assert p.any() and np.abs(s[p, :3] - np.array([1, 2.0 ** -10, 2.0 ** -20])).max() <= U.TOL_CONST / 4 * U.unit_roundoff(*shape)


def test_the_constant_and_the_cap_are_the_emulations():
    """TOL_CONST is 4 x the worst measure over all shapes (rounded up by less than 1 %), MAX_SWEEPS as derived"""
    worst, sweeps = 0.0, 0
    for shape in U.SHAPES:
        mats, kinds, s, u, v, sw = emulated(*shape)
        e = U.measures(mats, s, u, v)
        e = (e[0], np.where(kinds != 3, e[1], 0.0), e[2], e[3])
        worst = max(worst, max(float(x.max()) for x in e) / U.unit_roundoff(*shape))
        sweeps = max(sweeps, int(sw.max()))
    print("worst measure %.4f u, worst sweeps %d" % (worst, sweeps))
    assert 4 * worst <= U.TOL_CONST <= 4 * worst * 1.01
    assert U.MAX_SWEEPS == max(16, 2 * sweeps)
    design = open(os.path.join(REPO, "DESIGN.md")).read()
    assert "HRT_SVD_MAX_SWEEPS = %d" % U.MAX_SWEEPS in design and "%.1f u" % U.TOL_CONST in design


def test_emulation_is_independent_of_the_batch():
    mats, _ = U.master_cases(8, 8)
    a = U.emulate_batch(mats[:40])
    b = U.emulate_batch(mats[7:9])
    assert U.same([x[7:9] for x in a], b)


def test_exact_cases_need_no_rotation():
    names = []
    for name, H, (s, u, v) in U.exact_cases():
        es, eu, ev, sw = U.emulate_batch(H)
        assert not sw.any(), name
        assert np.array_equal(es, s) and np.array_equal(eu, u) and np.array_equal(ev, v), name
        rec = np.einsum("bid,bd,bjd->bij", u.astype(np.complex128), s.astype(np.float64), np.conj(v))
        assert np.array_equal(rec, H.astype(np.complex128)), name           # exact, not only close
        assert (s[:, :-1] >= s[:, 1:]).all()
        names.append(name)
    assert any("1x1" in n for n in names) and any("hadamard 16" in n for n in names)
    # ties, zero columns and H = 0 are among them
    _, H, (s, u, v) = U.exact_cases()[1]
    assert (s[:, 0] == s[:, -1]).any() and (s[:, -1] == 0).any() and not H[5].any() and not s[5].any()
    assert np.array_equal(v[5], np.eye(4)) and not u[5].any()


def test_non_finite_matrices_end_within_the_cap():
    mats = np.array(U.master_cases(4, 4)[0][:8])
    mats[2, 1, 3] = np.nan
    mats[5, 0, 0] = np.inf
    clean = U.emulate_batch(U.master_cases(4, 4)[0][:8])
    s, u, v, sw = U.emulate_batch(mats)
    assert sw[2] == U.NOT_CONVERGED and sw[5] == U.NOT_CONVERGED
    keep = np.array([0, 1, 3, 4, 6, 7])
    assert U.same([x[keep] for x in (s, u, v, sw)], [x[keep] for x in clean])


# ---------------------------------------------------------------- wrong results the checks catch

def _good(shape, count=64):
    mats, kinds = U.master_cases(*shape)
    mats, kinds = mats[:count], kinds[:count]
    return mats, kinds, U.emulate_batch(mats)


def _caught(mats, s, u, v, sw, relative=None):
    try:
        U.check(mats, s, u, v, sw, relative=relative)
    except AssertionError as e:
        return str(e) or "assert"
    return None


def mutant_unsorted_sigma():
    mats, kinds, (s, u, v, sw) = _good((5, 3))
    s, u, v = s[:, ::-1].copy(), u[:, :, ::-1].copy(), v[:, :, ::-1].copy()    # a consistent SVD, ascending
    return _caught(mats, s, u, v, sw, kinds != 3)


def mutant_unstable_ties():
    name, H, (s, u, v) = U.exact_cases()[1]
    got = U.emulate_batch(H, stable=False)
    assert _caught(H, *got) is None          # still an SVD ...
    return None if all(np.array_equal(a, b) for a, b in zip(got[:3], (s, u, v))) else "differs from the planting"


def mutant_no_null_rule():
    mats, kinds, _ = _good((5, 3))
    return _caught(mats, *U.emulate_batch(mats, null_rule=False), relative=kinds != 3)


def mutant_no_column_floor():
    mats, kinds, _ = _good((8, 8))
    return _caught(mats, *U.emulate_batch(mats, floor_clause=False), relative=kinds != 3)


def mutant_u_v_swapped_when_wide():
    mats, kinds, (s, u, v, sw) = _good((3, 5))
    wrong = _caught(mats, s, v, u, sw, kinds != 3)                      # the shapes give it away ...
    mats, kinds, (s, u, v, sw) = _good((3, 5))
    tall = U.emulate_batch(np.conj(np.swapaxes(mats, 1, 2)))            # ... and so do the values: H^H's (u, v) for H's
    sq = np.swapaxes(np.conj(mats), 1, 2)
    assert _caught(sq, *tall, relative=kinds != 3) is None
    mats4, kinds4, (s4, u4, v4, sw4) = _good((4, 4))
    return wrong and _caught(mats4, s4, v4, u4, sw4, kinds4 != 3)


def mutant_no_conjugate_on_v():
    mats, kinds, (s, u, v, sw) = _good((4, 4))
    return _caught(mats, s, u, np.conj(v), sw, kinds != 3)


def mutant_point_axes_transposed():
    mats, kinds = U.master_cases(3, 2)
    H = U.tensor(mats, (1, 1), 3, 3)
    r = U.emulate(H)
    bad = {k: np.ascontiguousarray(np.swapaxes(x, -1, -2)) for k, x in r.items()}
    ok = _caught(U.to_batch(H), U.to_batch_sigma(r["sigma"]), U.to_batch(r["u"]), U.to_batch(r["v"]), r["sweeps"].ravel())
    assert ok is None
    return _caught(U.to_batch(H), U.to_batch_sigma(bad["sigma"]), U.to_batch(bad["u"]), U.to_batch(bad["v"]),
                   bad["sweeps"].ravel())


def mutant_sigma_squared():
    mats, kinds, (s, u, v, sw) = _good((4, 4))
    return _caught(mats, s * s, u, v, sw, kinds != 3)


MUTANTS = [mutant_unsorted_sigma, mutant_unstable_ties, mutant_no_null_rule, mutant_no_column_floor,
           mutant_u_v_swapped_when_wide, mutant_no_conjugate_on_v, mutant_point_axes_transposed, mutant_sigma_squared]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda f: f.__name__[7:])
def test_checks_catch_the_wrong_result(mutant):
    why = mutant()
    print(mutant.__name__, "->", why)
    assert why


def test_checks_pass_the_right_result():
    for shape in ((5, 3), (3, 5), (4, 4)):
        mats, kinds, r = _good(shape)
        assert _caught(mats, *r, relative=kinds != 3) is None


def test_no_column_floor_fails_on_rank_one_as_the_definition_says():
    """the plain algorithm on rank-one 8 x 8 matrices rotates noise against noise: it is still rotating at the cap (or
    has formed a NaN), also at a cap of 40 sweeps; with the clause every one is finished within 8 sweeps"""
    mats, kinds = U.master_cases(8, 8)
    r1 = mats[kinds == 1][:16]
    for cap in (U.MAX_SWEEPS, 40):
        s, u, v, sw = U.emulate_batch(r1, floor_clause=False, max_sweeps=cap)
        assert (np.isnan(s).any(1) | (sw == U.NOT_CONVERGED)).all()
    s, u, v, sw = U.emulate_batch(r1)
    assert np.isfinite(s).all() and (sw <= 8).all()


# ---------------------------------------------------------------- hermespy_rt_amd.mimo against brute force

def _points(seed, nr, nt, shape=(2, 1, 2, 2, 3)):
    rng = np.random.RandomState(seed)
    full = shape[:2] + (nr, nt) + shape[2:]
    return (rng.standard_normal(full) + 1j * rng.standard_normal(full)).astype(np.complex64)


@pytest.mark.parametrize("nr,nt", [(4, 4), (5, 3), (2, 6), (1, 1)])
def test_svd_reference_layout(nr, nt):
    H = _points(1, nr, nt)
    r = mimo.svd_reference(H)
    n = min(nr, nt)
    assert r["sigma"].shape == (2, 1, n, 2, 2, 3) and r["u"].shape == (2, 1, nr, n, 2, 2, 3)
    assert r["v"].shape == (2, 1, nt, n, 2, 2, 3)
    rec = np.einsum("abidpmk,abdpmk,abjdpmk->abijpmk", r["u"], r["sigma"], np.conj(r["v"]))
    assert np.abs(rec - H).max() < 1e-12 * np.abs(H).max() * 1e6
    assert (np.diff(r["sigma"], axis=2) <= 0).all()
    one = np.linalg.svd(H[1, 0, :, :, 1, 0, 2].astype(np.complex128), compute_uv=False)
    assert np.allclose(r["sigma"][1, 0, :, 1, 0, 2], one, rtol=1e-13)
    with pytest.raises(ValueError):
        mimo.svd_reference(H[0])


def test_capacity_is_log_det():
    for nr, nt in ((4, 4), (5, 3), (2, 6)):
        H = _points(2, nr, nt)
        s = mimo.svd_reference(H)["sigma"]
        for snr in (0.1, 10.0, 1e3):
            c = mimo.capacity(s, snr, nt)
            assert c.shape == (2, 1, 2, 2, 3)
            A = np.moveaxis(H.astype(np.complex128), (2, 3), (-2, -1))
            det = np.linalg.det(np.eye(nr) + snr / nt * A @ np.conj(np.swapaxes(A, -1, -2)))
            assert np.allclose(c, np.log2(det.real), rtol=1e-10)
            assert np.allclose(mimo.capacity(s[1, 0, :, 1, 0, 2], snr, nt), c[1, 0, 1, 0, 2])


def _waterfill_bisection(g, snr):
    """capacity by a bisection on the water level mu: sum max(mu - 1 / g, 0) = snr"""
    g = g[g > 0]
    if not g.size:
        return 0.0
    lo, hi = 0.0, snr + (1.0 / g).max()
    for _ in range(200):
        mu = 0.5 * (lo + hi)
        if np.maximum(mu - 1.0 / g, 0).sum() > snr:
            hi = mu
        else:
            lo = mu
    p = np.maximum(0.5 * (lo + hi) - 1.0 / g, 0)
    return float(np.log2(1 + p * g).sum())


def test_waterfilling_is_the_bisection():
    rng = np.random.RandomState(5)
    for n in (1, 2, 5):
        s = np.abs(rng.standard_normal((3, 2, n, 2, 1, 4))) * 10.0 ** rng.uniform(-3, 1, (3, 2, n, 2, 1, 4))
        s[0, 0, -1:, 0] = 0.0
        s[1, 1, :, 1, 0, 0] = 0.0                       # a point without gain
        for snr in (1e-3, 1.0, 1e4):
            w = mimo.waterfilling(s, snr)
            assert w.shape == (3, 2, 2, 1, 4)
            flat = np.moveaxis(s, 2, -1).reshape(-1, n)
            ref = np.array([_waterfill_bisection(x * x, snr) for x in flat]).reshape(w.shape)
            assert np.allclose(w, ref, rtol=1e-9, atol=1e-12)
            assert (w >= mimo.capacity(s, snr, n) - 1e-12).all()     # at least the equal-power capacity over n streams
    assert mimo.waterfilling(np.zeros(3), 1.0) == 0.0


def test_condition_number_and_rank():
    s = np.array([4.0, 2.0, 0.5])
    assert mimo.condition_number(s) == 8.0 and mimo.rank(s, 3, 3) == 3
    assert np.isinf(mimo.condition_number(np.array([1.0, 0.0])))
    eps = 8 * 2.0 ** -23
    assert mimo.rank(np.array([1.0, eps, 0.0]), 8, 3) == 1 and mimo.rank(np.array([1.0, eps * 1.01, 0.0]), 3, 8) == 2
    assert mimo.rank(np.zeros(4), 4, 4) == 0
    t = np.zeros((1, 1, 3, 2, 1, 2))
    t[0, 0, :, 0, 0, 1] = (3, 1, 0)
    assert mimo.rank(t, 3, 3).tolist() == [[[[[0, 2]], [[0, 0]]]]]
    assert mimo.condition_number(t)[0, 0, 0, 0, 1] == np.inf


def test_precoder_and_combiner_diagonalise_the_point():
    from hermespy_rt_amd import beams
    H = _points(9, 5, 3)
    r = mimo.svd_reference(H)
    u, v, s = r["u"][1, 0, :, :, 1, 0, 2], r["v"][1, 0, :, :, 1, 0, 2], r["sigma"][1, 0, :, 1, 0, 2]
    wr, wt = mimo.combiner(u, 2), mimo.precoder(v, 2)
    assert wr.shape == (2, 5) and wt.shape == (2, 3)
    B = np.conj(wr) @ H[1, 0, :, :, 1, 0, 2].astype(np.complex128) @ wt.T     # conj(W_rx) H W_tx^T: beam_channel's rule
    assert np.allclose(B, np.diag(s[:2]), atol=1e-12)
    assert np.allclose(beams.apply(H.astype(np.complex128), wr, wt)[1, 0, :, :, 1, 0, 2], B, atol=1e-12)
    for bad in (0, 4):
        with pytest.raises(ValueError):
            mimo.precoder(v, bad)
    with pytest.raises(ValueError):
        mimo.combiner(r["u"], 1)
