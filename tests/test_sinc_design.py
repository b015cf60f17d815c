"""The design of the per-weight sinc tests (tests/sinc_util.py), on the CPU: the float64 reference against mpmath, the
floor of a faithful float32 emulation of csrc/hrt_sinc.h (which fixes the bound B the device is held to in
tests/test_gpu_sinc_weights.py), the eight mutants of the emulation that the cases must catch, and the same floor for
the phase factor of a record (the bound P)."""
import math

import numpy as np
import pytest

from . import sinc_util as S

CASES = S.cases()


def _windows(windows):
    return np.concatenate([lo + np.arange(L, dtype=np.int64) for lo, L in windows])


def test_every_delay_is_in_its_class():
    assert S.design_errors(CASES) == []
    assert tuple(sorted({c for c, _, _, _ in CASES})) == S.CLASSES


def test_reference_against_mpmath():
    mpmath = pytest.importorskip("mpmath")
    worst = 0.0
    for cls, fs, tau, windows in CASES:
        l = _windows(windows)
        ref = S.sinc_ref(fs, tau, l)
        mp = S.sinc_mp(fs, tau, l, bits=200)
        for i in range(tau.size):
            for j in range(l.size):
                m = mp[i][j]
                if m == 0 or m == 1:
                    assert ref[i, j] == float(m), (cls, fs, tau[i], l[j], ref[i, j])
                    continue
                e = abs((mpmath.mpf(float(ref[i, j])) - m) / m)
                worst = max(worst, float(e))
                assert e <= 8 * 2.0 ** -53, (cls, fs, tau[i], l[j], ref[i, j], float(e) / 2.0 ** -53)
    print("sinc_ref against mpmath: at most %.2f x 2^-53 relative" % (worst / 2.0 ** -53))


def test_floor_of_the_faithful_emulation_and_the_bound():
    floor = {}
    for cls, fs, tau, windows in CASES:
        l = _windows(windows)
        e = S.check(S.sinc_emulate(fs, tau, l), fs, tau, l, S.B, what="emulation, class " + cls)
        floor[cls] = max(floor.get(cls, 0.0), e)
    print("floor of the emulation, units of 2^-24 |w|: " + ", ".join("%s %.2f" % kv for kv in sorted(floor.items())))
    assert math.ceil(max(floor.values())) == S.FLOOR_CEIL
    assert S.B == S.FLOOR_CEIL + 6


@pytest.mark.parametrize("mutation", S.MUTATIONS)
def test_a_mutant_of_the_emulation_fails(mutation):
    caught = set()
    for cls, fs, tau, windows in CASES:
        l = _windows(windows)
        try:
            S.check(S.sinc_emulate(fs, tau, l, **{mutation: True}), fs, tau, l, S.B)
        except AssertionError:
            caught.add(cls)
    print("%s: caught by the classes %s" % (mutation, "".join(sorted(caught))))
    assert caught, mutation
    want = {"switch_1e3": "c", "tie_away": "bf", "no_clamp": "j", "parity_of_k": "j", "c_remainder": "fgj",
            "x_float": "a", "rcp_12bit": "abcdfghij"}.get(mutation, "".join(S.CLASSES))
    assert set(want) <= caught, (mutation, sorted(caught))


def test_check_itself():
    cls, fs, tau, windows = CASES[0]
    l = _windows(windows)
    ref = S.sinc_ref(fs, tau, l)
    assert S.check(ref, fs, tau, l, 0.0) == 0.0
    for bad in (np.nan, np.inf):
        g = ref.copy()
        g[3, 5] = bad
        with pytest.raises(AssertionError):
            S.check(g, fs, tau, l, S.B)
    g = ref.copy()
    g[3, 5] *= 1 + (S.B + 1) * S.U
    with pytest.raises(AssertionError):
        S.check(g, fs, tau, l, S.B)
    g[3, 5] = ref[3, 5] * (1 + (S.B - 1) * S.U)
    assert S.B - 1.01 < S.check(g, fs, tau, l, S.B) < S.B
    # exact weights: 1 - 2^-24 for a 1 and a denormal for a 0 both fail; -0 for 0 passes
    cls, fs, tau, windows = [c for c in CASES if c[0] == "e"][0]
    l = _windows(windows)
    ref = S.sinc_ref(fs, tau, l)
    assert set(np.unique(ref)) == {0.0, 1.0}
    S.check(np.where(ref == 0, -0.0, ref), fs, tau, l, S.B)
    for at, bad in ((1.0, 1.0 - S.U), (0.0, 1e-45)):
        g = ref.copy()
        g[tuple(np.argwhere(ref == at)[0])] = bad
        with pytest.raises(AssertionError):
            S.check(g, fs, tau, l, S.B)


def test_floor_of_the_phase_factor_and_the_bound():
    fc = 3.5e9
    floor = {}
    for cls, fs, tau, windows in CASES:
        if cls not in S.PHASE_CLASSES:
            continue
        tau = S.by_link(tau, 64)   # (as tests/test_gpu_sinc_weights.py deals them to its 8 x 8 links)
        nu, t = S.phase_inputs(64)
        ref = S.phase_ref(nu, t, fc, tau)
        e = np.abs(S.phase_emulate(nu, t, fc, tau) - ref[None]).max() / S.U
        floor[cls] = max(floor.get(cls, 0.0), float(e))
    print("floor of the phase factor, units of 2^-24: " + ", ".join("%s %.2f" % kv for kv in sorted(floor.items())))
    assert math.ceil(max(floor.values()) + 0.5) == S.PHASE_FLOOR_CEIL
    assert S.P == S.PHASE_FLOOR_CEIL + 3
