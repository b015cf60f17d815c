"""The codebook selection's design on the CPU (csrc/hrt_codebook.h, csrc/hrt_codebook.hip; tests/codebook_util.py): the
tile rule and the LDS image built for the host, the log2 restatement against the C function bit for bit and against
float64, the float32 emulation on the exact plantings (equal to the rounded float64 reference, bit for bit), the
tolerance constants recomputed, the lead of the float64 reference over the case list, and the wrong readings of the
definition that the cases separate."""
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import codebook as CB

from . import codebook_util as U


def _build(tmp_path, body, name):
    prog = tmp_path / (name + ".c")
    prog.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "hrt_codebook.h"\n' + body)
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I",
                           os.path.join(U.REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    return str(exe)


def _shapes():
    """(Nt, L) of every test shape: the GPU tests' case lists"""
    s = {(c[3], c[4]) for c in U.INTEGER_CASES}
    for c in U.NORMAL_CASES:
        s.add((c[3], U.normal_case(c)[1].shape[2]))
    return sorted(s)


def test_tile_rule_built_for_the_host(tmp_path):
    exe = _build(tmp_path, "int main(void){for (unsigned nt = 0; nt <= 65; ++nt) for (unsigned l = 0; l <= 5; ++l) "
                 'printf("%u %u %u\\n", nt, l, hrt_codebook_tile(nt, l)); '
                 'printf("%u %u %u %u %u %u %u %u\\n", HRT_CS_THREADS, HRT_CS_WAVES, HRT_CS_LDS_BYTES, HRT_CS_MAX_NR, '
                 "HRT_CS_MAX_NT, HRT_CS_MAX_L, HRT_CS_MAX_C, HRT_CS_ROWS); return 0;}\n", "tile")
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([exe], text=True).splitlines()]
    assert lines[-1] == [U.THREADS, U.WAVES, U.LDS_BYTES, U.MAX_NR, U.MAX_NT, U.MAX_L, U.MAX_C, U.ROWS]
    assert len(lines) - 1 == 66 * 6
    seen = set()
    for nt, l, ct in lines[:-1]:
        assert ct == U.tile(nt, l)
        inside = 1 <= nt <= 64 and 1 <= l <= min(4, nt)
        assert (ct > 0) == inside
        if inside:
            assert ct in (32, 64) and ct * nt * l * 8 <= U.LDS_BYTES and (ct == 64 or 64 * nt * l * 8 > U.LDS_BYTES)
            seen.add(ct)
    assert seen == {32, 64}
    # the test shapes take both tile sizes, and C meets each at -1, +0, +1 and two tiles plus one
    for ct in (32, 64):
        cs = {c[5] for c in U.INTEGER_CASES if U.tile(c[3], c[4]) == ct}
        assert {ct - 1, ct, ct + 1, 2 * ct + 1} <= cs, (ct, cs)


@pytest.mark.parametrize("shape", _shapes(), ids=lambda s: "nt%d-l%d" % s)
def test_lds_image_has_one_owner_per_word_and_no_bank_conflicts(tmp_path, shape):
    nt, L = shape
    ct = U.tile(nt, L)
    exe = _build(tmp_path, "int main(int n, char **v){unsigned ct = atoi(v[1]), nt = atoi(v[2]), L = atoi(v[3]); "
                 "for (unsigned j = 0; j < ct; ++j) for (unsigned t = 0; t < nt; ++t) for (unsigned l = 0; l < L; ++l) "
                 'printf("%u\\n", hrt_codebook_slot(ct, L, j, t, l)); return 0;}\n', "slot")
    got = np.array(subprocess.check_output([exe, str(ct), str(nt), str(L)], text=True).split(), np.int64)
    want = np.array([U.slot(ct, L, j, t, l) for j in range(ct) for t in range(nt) for l in range(L)])
    assert np.array_equal(got, want)
    # one owner per word: the slots of all (entry, element) are a permutation of the image
    assert np.array_equal(np.sort(got), np.arange(ct * nt * L))
    assert ct * nt * L * 8 <= U.LDS_BYTES
    # staging: thread w of a pass of 256 writes slot w for entry w % ct, element w // ct -- the same map, in order
    w = np.arange(ct * nt * L)
    assert np.array_equal(U.slot(ct, L, w % ct, (w // ct) // L, (w // ct) % L), w)
    for first in range(0, ct * nt * L, 64):
        assert U.banks_b64(w[first:first + 64]) == 1
    # scoring: lane j of a wave reads element (t, l) of its entry, one float2 per lane
    for t in range(nt):
        for l in range(L):
            assert U.banks_b64([U.slot(ct, L, j, t, l) for j in range(ct)]) == 1


def test_log2_restatement_follows_the_c_function_bit_for_bit(tmp_path):
    exe = _build(tmp_path, "int main(int n, char **v){unsigned long a = strtoul(v[1], 0, 0), b = strtoul(v[2], 0, 0), "
                 "s = strtoul(v[3], 0, 0); for (unsigned long u = a; u < b; u += s) {uint32_t w = (uint32_t)u, r; float x, y; "
                 'memcpy(&x, &w, 4); y = hrt_cs_log2(x); memcpy(&r, &y, 4); printf("%u\\n", r);} return 0;}\n', "log2")
    for a, b, s in ((0x3F000000, 0x40800000, 1009), (0x00000000, 0xFFFFFFFF, 7_654_321), (0x3FB504F3 - 40, 0x3FB504F3 + 40, 1),
                    (0x3F800000 - 40, 0x3F800000 + 40, 1), (0x7F7FFFF0, 0x7F800010, 1), (0x007FFFF0, 0x00800010, 1)):
        got = np.array(subprocess.check_output([exe, str(a), str(b), str(s)], text=True).split(), np.uint64).astype(np.uint32)
        x = np.arange(a, b, s, dtype=np.uint64).astype(np.uint32).view(np.float32)
        emu = U.log2_f32(x).view(np.uint32)
        nan = np.isnan(got.view(np.float32))
        assert np.array_equal(nan, np.isnan(emu.view(np.float32)))
        assert np.array_equal(got[~nan], emu[~nan])
        normal = (x.view(np.uint32) >= 0x00800000) & (x.view(np.uint32) < 0x7F800000)
        assert np.array_equal(nan, ~normal)


def test_log2_restatement_against_float64():
    """Every 61st mantissa of four binades around 1 (275 000 values a binade), the exact powers of two, and both sides
    of the sqrt(2) split.  The bound: with p = log2 of the reduced mantissa, |p| <= 1/2, the quotient, the square, four
    Horner steps (two roundings each) and the product round 11 times on the way to p, the series' tail adds 2^-28 |p|,
    and the last sum rounds once: |error| <= 2^-24 (|result| + 12 |p|)."""
    u = np.arange(0x3F000000, 0x40800000, 61, dtype=np.uint32)
    x = u.view(np.float32)
    ref = np.log2(x.astype(np.float64))
    got = U.log2_f32(x).astype(np.float64)
    p = ref - np.floor(ref + 0.5)           # the reduced part: the exponent after the split is the nearest integer
    assert (np.abs(got - ref) <= 2.0 ** -24 * (np.abs(ref) + 12 * np.abs(p)) + 1e-300).all()
    # the powers of two are exact, every normal one
    k = np.arange(-126, 128)
    assert np.array_equal(U.log2_f32(np.ldexp(np.float32(1), k).astype(np.float32)), k.astype(np.float32))
    # monotone across the split of the mantissa at sqrt(2)
    s = np.arange(U.SQRT2_BITS - 64, U.SQRT2_BITS + 64, dtype=np.uint32).view(np.float32)
    assert (np.diff(U.log2_f32(s)) >= 0).all()
    # outside the normal positive floats: NaN
    bad = np.array([0.0, -0.0, -1.0, np.inf, -np.inf, np.nan, 1e-45, 1.1e-38], np.float32)
    assert np.isnan(U.log2_f32(bad)).all()


# ---------------------------------------------------------------- exact plantings

@pytest.mark.parametrize("case", U.INTEGER_CASES, ids=lambda c: c[0])
def test_gaussian_integer_plantings_are_exact_under_power(case):
    H, W, S = U.integer_case(case)
    K = H.shape[6]
    assert S & (S - 1) == 0 and K % S in (0, 1)
    ref = CB.select_reference(H, W, "power", None, S)
    assert ref["table"].max() * S < 2 ** 24 and np.array_equal(ref["table"] * S, np.round(ref["table"] * S))
    assert not ref["status"].any()
    assert U.same(U.emulate(H, W, U.POWER, None, S), U.rounded(ref)) is None


def test_integer_cases_cover_every_axis_value():
    cases = U.INTEGER_CASES
    assert {c[2] for c in cases} >= {1, 2, 3, 16} and {c[3] for c in cases} >= {1, 4, 33, 63, 64}
    assert {c[4] for c in cases} == {1, 2, 3, 4} and {c[5] for c in cases} >= {1, 2, 1023, 1024, 1025}
    assert {c[7] for c in cases} >= {1, 5, 64} and {c[6] for c in cases} >= {1, 3}
    assert any(c[1] == (2, 2) for c in cases)
    assert any(c[8] == 1 and c[7] > 1 for c in cases) and any(c[8] == 2 for c in cases)
    assert any(c[8] == c[7] and c[7] > 1 for c in cases) and any(c[7] % c[8] == 1 and c[8] > 1 for c in cases)
    differ = 0
    for c in cases:
        if c[5] > 1 and c[2] * c[3] <= 64:
            H, W, S = U.integer_case(c)
            idx = CB.select_reference(H, W, "power", None, S)["index"]
            differ += bool((idx[:, :, 0] != idx[:, :, 1]).any())
    assert differ >= 3          # both pols with different winners


def test_capacity_with_one_layer_and_power_of_two_determinants_is_exact():
    H, W, S, n0 = U.capacity_l1_case()
    ref = CB.select_reference(H, W, "capacity", n0, S)
    assert len(np.unique(ref["table"])) >= 6
    assert np.array_equal(ref["table"] * S, np.round(ref["table"] * S))
    assert U.same(U.emulate(H, W, U.CAPACITY, n0, S), U.rounded(ref)) is None


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 4, 2), (3, 33, 3), (16, 63, 4), (16, 64, 4)),
                         ids=lambda s: "%dx%d-l%d" % s)
def test_one_hot_plantings_pin_every_index(shape):
    nr, nt, L = shape
    H, W, want = U.one_hot_case(nr, nt, L)
    emu = U.emulate(H, W, U.POWER, None, 1)
    assert U.same(emu, U.rounded(CB.select_reference(H, W, "power", None, 1))) is None
    assert np.array_equal(emu["index"].ravel(), want) and (emu["metric"] == L * L).all()
    # every (row, layer) of effective, every (column) of H and every entry of the last layer is hit
    E = emu["effective"]
    assert (np.abs(E).sum((0, 1, 4, 5, 6))[:, L - 1] > 0).all() and np.abs(E).sum() == L * want.size
    assert set(want) == {t * L + L - 1 for t in range(nt)}


def test_planted_ties_return_the_lowest_index_and_zero_channel_index_zero():
    H, W, S, c = U.tie_case()
    for metric in (U.POWER, U.CAPACITY):
        emu = U.emulate(H, W, metric, 0.5, S)
        assert (emu["index"] == c).all()
        t = emu["table"]
        assert np.array_equal(t[:, :, c], t[:, :, 66]) and np.array_equal(t[:, :, c], t[:, :, 67])
        zero = U.emulate(np.zeros_like(H), W, metric, 0.5, S)
        assert not zero["index"].any() and not zero["status"].any() and not zero["table"].any()
        assert U.same(zero, U.rounded(CB.select_reference(np.zeros_like(H), W, metric, 0.5, S))) is None


def test_non_finite_subbands_are_flagged_alone():
    H, W, S = U.normal_case(U.NORMAL_CASES[0])
    clean = U.emulate(H, W, U.CAPACITY, U.NOISE, S)
    for value in (np.nan, np.inf, 1e30):
        Hb = H.copy()
        Hb[0, 0, 1, 2, 1, 0, S + 1] = value
        for metric in (U.POWER, U.CAPACITY):
            emu = U.emulate(Hb, W, metric, U.NOISE, S)
            ref = CB.select_reference(Hb, W, metric, U.NOISE, S)
            flagged = np.zeros(emu["status"].shape, bool)
            flagged[0, 0, 1, 0, 1] = True
            assert np.array_equal(emu["status"] != 0, flagged)
            assert (emu["index"][flagged] == U.NO_INDEX).all() and not emu["metric"][flagged].any()
            assert not emu["table"][0, 0, :, 1, 0, 1].any() and not emu["effective"][0, 0, :, :, 1, 0, S:2 * S].any()
            if value != 1e30:       # (a square beyond float is finite in float64: the reference does not flag it)
                assert np.array_equal(ref["status"], emu["status"])
            if metric == U.CAPACITY:
                keep = ~flagged
                assert np.array_equal(emu["index"][keep], clean["index"][keep])
                assert np.array_equal(emu["metric"][keep], clean["metric"][keep])


# ---------------------------------------------------------------- the tolerance and the lead

_NORMAL = {}


def _normal(case, metric):
    key = (case[0], metric)
    if key not in _NORMAL:
        H, W, S = U.normal_case(case)
        _NORMAL[key] = (H, W, S, U.emulate(H, W, metric, U.NOISE, S),
                        CB.select_reference(H, W, U.METRIC_NAME[metric], U.NOISE, S))
    return _NORMAL[key]


def test_tolerance_constants_are_four_times_the_emulations_worst():
    mu = eff = 0.0
    for case in U.NORMAL_CASES:
        for metric in (U.POWER, U.CAPACITY):
            H, W, S, emu, ref = _normal(case, metric)
            assert np.array_equal(emu["index"], ref["index"]), case[0]
            mu = max(mu, U.mu_error(emu["table"], ref["table"], case[2], case[3]))
            eff = max(eff, U.eff_error(emu["effective"], ref, H, W, emu["index"]))
    assert 0.95 * U.MU_WORST <= mu <= U.MU_WORST, mu
    assert 0.95 * U.EFF_WORST <= eff <= U.EFF_WORST, eff
    assert U.MU_BOUND == 4 * U.MU_WORST and U.EFF_BOUND == 4 * U.EFF_WORST


@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_reference_lead_exceeds_twice_the_bound_on_the_case_list(case):
    for metric in (U.POWER, U.CAPACITY):
        _, _, _, emu, ref = _normal(case, metric)
        assert U.lead_share(ref, case[2], case[3]) >= 0.95
        ok, second = U.index_check(emu["index"], ref, case[2], case[3])
        assert ok and second <= 0.05


def test_normal_cases_cover_both_codebook_kinds_and_both_tiles():
    kinds = {c[7][0] for c in U.NORMAL_CASES}
    assert kinds == {"dual", "random"}
    tiles = {U.tile(c[3], U.normal_case(c)[1].shape[2]) for c in U.NORMAL_CASES}
    assert tiles == {32, 64}
    assert any(c[5] % c[6] for c in U.NORMAL_CASES) and any(c[4] > 1 for c in U.NORMAL_CASES)
    assert any(c[1] == (2, 2) for c in U.NORMAL_CASES)
    for c in U.NORMAL_CASES:        # unit norm
        W = U.normal_case(c)[1]
        assert np.allclose((np.abs(W) ** 2).sum((1, 2)), 1.0, atol=1e-6)


# ---------------------------------------------------------------- wrong readings

def _differs(r, w, nr, nt):
    """whether a reading's result is told from the right one by the checks the GPU tests apply"""
    if w is None:
        return False
    if U.mu_error(w["table"], r["table"], nr, nt) > U.MU_BOUND:
        return True
    ok, second = U.index_check(w["index"], r, nr, nt)
    if not ok or second > 0.05:
        return True
    return not np.array_equal(w["index"], r["index"]) or \
        np.abs(w["effective"] - r["effective"]).max() > 1e-3 * np.abs(r["effective"]).max()


@pytest.mark.parametrize("wrong", U.WRONG_READINGS)
def test_wrong_readings_are_caught(wrong):
    caught = []
    for case in U.NORMAL_CASES:
        H, W, S = U.normal_case(case)
        for metric in ("power", "capacity"):
            if wrong in ("noise-multiplied", "trace", "power-under-capacity") and metric == "power":
                continue
            r = CB.select_reference(H, W, metric, U.NOISE, S)
            if _differs(r, U.reading(H, W, metric, U.NOISE, S, wrong), case[2], case[3]):
                caught.append((case[0], metric))
    if wrong == "highest-on-ties":      # only a planted tie tells it
        H, W, S, c = U.tie_case()
        r = CB.select_reference(H, W, "power", None, S)
        w = U.reading(H, W, "power", None, S, wrong)
        assert (r["index"] == c).all() and (w["index"] == 67).all()
        return
    if wrong == "pol-time-swapped":     # it shows only with several times
        assert caught and all(c[4] > 1 for c in U.NORMAL_CASES if (c[0], "power") in caught)
    assert caught, wrong
    if wrong == "trace":                # it is the definition at L = 1 and must be caught at L > 1
        assert all(U.normal_case(c)[1].shape[2] > 1 for c in U.NORMAL_CASES if (c[0], "capacity") in caught)
