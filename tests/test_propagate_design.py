"""Design of the received-signal tests (tests/propagate_util.py, hermespy_rt_amd.propagate), no GPU: the float64
reference against an independent formulation, the planted cases against eight wrong readings of the definition, the
error bound against float32 chains, the form rule and the LDS layout of csrc/hrt_propagate.h."""
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import propagate as pg

from . import propagate_util as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = U.exact_cases()


def test_cases_cover_the_axes():
    print("exact cases:", len(CASES))
    assert U.covered([c["choice"] for c in CASES])
    assert len(CASES) <= 150
    forms = {U.form(c["M"], 1 if c["S"] is None else c["S"]) for c in CASES}
    assert forms == {U.MFMA, U.GENERAL}
    # the MFMA-form cases with blocks: M S both below n_out (the clamp) and above it (unused blocks)
    blocked = [c for c in CASES if c["S"] is not None and c["S"] % 16 == 0]
    assert any(c["M"] * c["S"] < c["n_out"] for c in blocked) and any(c["M"] * c["S"] > c["n_out"] for c in blocked)
    assert any(c["N"] < c["L"] for c in CASES)
    # the shifted windows that leave nothing: an all-zero y, and cases with a non-zero one
    zero = [not reference_of(c).any() for c in CASES]
    assert any(zero) and not all(zero)


_REF = {}


def reference_of(case):
    k = id(case)
    if k not in _REF:
        h, x = U.plant_integers(case)
        _REF[k] = U.reference(case, h, x)
    return _REF[k]


def test_reference_agrees_with_convolution_and_evaluator():
    for c in CASES:
        h, x = U.plant_integers(c)
        ref = reference_of(c)
        assert ref.shape == (c["nrx"], c["nr"], 2, c["n_out"])
        assert np.array_equal(ref, U.convolve_reference(h, x, c["l_min"], c["S"], c["n_out"])), c
        assert np.array_equal(ref, U.evaluate(h, x, c["l_min"], c["S"], c["n_out"])), c
        assert np.array_equal(ref, np.round(ref)) and np.abs(ref.real).max(initial=0) < 1 << 24


def test_reference_takes_the_shapes_of_taps():
    rng = np.random.RandomState(3)
    h = rng.standard_normal((2, 3, 2, 1, 4)) + 1j * rng.standard_normal((2, 3, 2, 1, 4))   # taps(): 5-D
    x = rng.standard_normal((3, 9)) + 1j * rng.standard_normal((3, 9))
    y = pg.apply_taps_reference(h, x)
    assert y.shape == (2, 1, 2, pg.default_num_out(9, 4, 0))
    assert np.allclose(y, pg.apply_taps_reference(h[:, :, None, None], x[:, None]))
    assert np.allclose(y[1, 0, 1], sum(np.convolve(h[1, t, 1, 0], x[t]) for t in range(3)))
    with pytest.raises(ValueError):
        pg.apply_taps_reference(np.zeros((1, 1, 2, 2, 4)), np.zeros((1, 9)))   # M = 2 without samples_per_block
    with pytest.raises(ValueError):
        pg.apply_taps_reference(np.zeros((1, 2, 2, 1, 4)), np.zeros((1, 9)))   # ntx differs


@pytest.mark.parametrize("mutant", U.MUTANTS)
def test_planted_cases_catch_the_mutant(mutant):
    caught = 0
    for c in CASES:
        h, x = U.plant_integers(c)
        caught += not np.array_equal(reference_of(c), U.evaluate(h, x, c["l_min"], c["S"], c["n_out"], mutant))
    print(mutant, "caught by", caught, "of", len(CASES), "cases")
    assert caught >= 2


def test_one_hot_cases():
    cases = U.one_hot_cases()
    hits = 0
    for S, i in cases:
        h, x = U.one_hot_tensors(i)
        y = pg.apply_taps_reference(h, x, 0, S, U.ONE_HOT_SHAPE["n_out"])
        want = np.zeros_like(y)
        at = U.one_hot_expected(S, i)
        if at is not None:
            want[at] = 1
            hits += 1
        assert np.array_equal(y, want), (S, i)
    assert 8 <= hits <= len(cases) - 8
    for a in U.ONE_HOT_AXES:   # every axis at its first and its last index
        assert len({i[a] for _, i in cases}) == 2


def test_block_helpers():
    assert pg.num_blocks(100, None) == 1 and pg.num_blocks(100, 1) == 100 and pg.num_blocks(100, 16) == 7
    assert pg.num_blocks(96, 16) == 6 and pg.num_blocks(1, 48) == 1
    assert pg.block_times(1e6, None, 0.25) == (0.25, 0.0)
    assert pg.block_times(1e6, 1, 0.25) == (0.25, 1e-6)
    t0, dt = pg.block_times(2e6, 16, 1.0)
    assert t0 == 1.0 + 15 / 4e6 and dt == 16 / 2e6
    assert pg.default_num_out(40, 16, 0) == 55 and pg.default_num_out(40, 16, 5) == 60
    assert pg.default_num_out(40, 16, -3) == 55
    with pytest.raises(ValueError):
        pg.num_blocks(10, 0)


def _f32_chain(h, x, case, S, reverse):
    """y of one small case as a float32 multiply-add chain over (tx, j, l) (reverse: the opposite order), products
    rounded, then the sum rounded"""
    f = np.float32
    nrx, ntx, nr, nt, _, M, L = h.shape
    N, n_out, l_min = x.shape[2], case["n_out"], case["l_min"]
    y = np.zeros((nrx, nr, 2, n_out), np.complex64)
    terms = [(tx, j, l) for tx in range(ntx) for j in range(nt) for l in range(L)]
    if reverse:
        terms.reverse()
    for rx in range(nrx):
        for i in range(nr):
            for pol in range(2):
                for n in range(n_out):
                    m = min(n // S, M - 1)
                    re, im = f(0), f(0)
                    for tx, j, l in terms:
                        k = n - l_min - l
                        if not 0 <= k < N:
                            continue
                        hv, xv = h[rx, tx, i, j, pol, m, l], x[tx, j, k]
                        re = f(re + f(f(hv.real) * f(xv.real)))
                        re = f(re - f(f(hv.imag) * f(xv.imag)))
                        im = f(im + f(f(hv.real) * f(xv.imag)))
                        im = f(im + f(f(hv.imag) * f(xv.real)))
                    y[rx, i, pol, n] = complex(re, im)
    return y


def test_error_bound_holds_for_float32_chains_in_both_orders():
    shape = dict(nrx=1, nr=2, ntx=2, nt=2, L=9, N=24, n_out=30, l_min=-1)
    S, M = 7, 5
    h, x = U.plant_normal(shape, M, 11)
    ref = pg.apply_taps_reference(h, x, shape["l_min"], S, shape["n_out"])
    bound = pg.error_bound(h, x, shape["l_min"], S, shape["n_out"])
    assert bound.shape == ref.shape and (bound > 0).all()
    K = shape["ntx"] * shape["nt"] * shape["L"]
    gamma = 2 * K * 2.0 ** -24 / (1 - 2 * K * 2.0 ** -24)
    assert np.allclose(bound, gamma * pg.apply_taps_reference(np.abs(h), np.abs(x), shape["l_min"], S,
                                                              shape["n_out"]).real)
    worst = 0.0
    for reverse in (False, True):
        y = _f32_chain(h, x, shape, S, reverse)
        err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
        assert (err <= bound).all()
        worst = max(worst, float((err / bound).max()))
    print("largest float32-chain error / bound: %.3f" % worst)
    assert worst > 1e-3   # (the bound is not vacuous: float32 rounding is seen)


def test_form_rule_mirror_matches_the_header(tmp_path):
    pairs = [(m, s) for m in (1, 2, 3, 7) for s in (1, 5, 15, 16, 17, 32, 40, 48, 1024, 4095)]
    prog = tmp_path / "f.c"
    prog.write_text('#include <stdio.h>\n#include "hrt_propagate.h"\nint main(void){\n' +
                    "".join('printf("%%u ", hrt_propagate_form(%du, %du));\n' % p for p in pairs) +
                    'printf("\\n%u %u %u %u %u\\n", HRT_PG_MFMA, HRT_PG_COLS, HRT_PG_LC, HRT_PG_WTILES, HRT_PG_WINDOW);'
                    "return 0;}\n")
    exe = tmp_path / "f"
    subprocess.check_call(["gcc", "-std=gnu11", "-I", os.path.join(REPO, "include"), "-I",
                           os.path.join(REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    out = subprocess.check_output([str(exe)], text=True).split("\n")
    mfma, cols, lc, wtiles, window = (int(v) for v in out[1].split())
    got = [U.MFMA if int(v) == mfma else U.GENERAL for v in out[0].split()]
    assert got == [U.form(*p) for p in pairs]
    assert (cols, lc, wtiles) == (U.COLS, U.LC, U.WTILES) and window == cols + lc and lc % 2 == 0
    assert cols == 4 * wtiles * 16


def test_b_reads_are_free_of_bank_conflicts():
    """ds_read_b32 serves a wave in two halves of 32 lanes over 32 banks: in each half the lanes that do not share an
    address (a broadcast) must lie on different banks -- here all 32 lanes of a half read different banks"""
    for nl in range(0, U.COLS, 16):
        for lc in (1, 2, 17, U.LC):
            for d0 in range(0, lc, 2):
                banks = U.b_read_banks(nl, lc, d0)
                assert len(set(banks[:32])) == 32 and len(set(banks[32:])) == 32
