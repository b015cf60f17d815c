"""The K-best tree-search detection's design on the CPU (csrc/hrt_kbest.h, csrc/hrt_kbest.hip; tests/kbest_util.py): the
form rule built for the host over every (Nr, Nt, K), the float32 emulation on the exact plantings (equal to the rounded
float64 reference, bit for bit), what the plantings cover, the wrong readings of the definition that they separate,
the pruned maximum-likelihood hypothesis, the exhaustive limits against hermespy_rt_amd.detect.ml_reference, the
fragile-point cap of the standard-normal cases and the tolerance constants recomputed."""
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import detect as DT

from . import kbest_util as U
from .detect_util import REPO


# ---------------------------------------------------------------- the form

def test_form_rule_built_for_the_host(tmp_path):
    prog = tmp_path / "form.c"
    prog.write_text('#include <stdio.h>\n#include "hrt_kbest.h"\n'
                    "int main(void){for (unsigned nr = 0; nr <= 65; ++nr) for (unsigned nt = 0; nt <= 17; ++nt) "
                    "for (unsigned k = 0; k <= 65; ++k) { unsigned g = hrt_kbest_form(nr, nt, k); "
                    'if (g || (k & (k - 1)) == 0) printf("%u %u %u %u\\n", nr, nt, k, g); } '
                    'printf("%u %u %u %u %u %u %u\\n", HRT_KB_THREADS, HRT_KB_WORDS, HRT_KB_MAX_NR, HRT_KB_MAX_NT, '
                    "HRT_KB_MAX_B, HRT_KB_MAX_BITS, HRT_KB_MAX_K); return 0;}\n")
    exe = tmp_path / "form"
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-I", os.path.join(REPO, "hermespy-rt_amd", "csrc"),
                           str(prog), "-o", str(exe)])
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert lines[-1] == [U.THREADS, U.WORDS, U.MAX_NR, U.MAX_NT, U.MAX_B, U.MAX_BITS, U.MAX_K]
    inside = 0
    for nr, nt, k, g in lines[:-1]:
        assert g == U.form(nr, nt, k), (nr, nt, k)
        ok = 1 <= nr <= 64 and 1 <= nt <= 16 and k in U.KS
        assert (g > 0) == ok, (nr, nt, k)
        if ok:
            inside += 1
            # a power of two from K to 64 whose share of LDS holds the matrix and the point's R and z, the smallest
            assert g >= k and 64 % g == 0
            words = lambda x: 2 * (nt + 1) * -(-nr // x) + -(-U.point_words(nt) // x)
            assert words(g) <= U.WORDS and (g == k or words(g // 2) > U.WORDS)
    assert inside == 64 * 16 * 7
    # the threads' words and the constellation fit the 64 KiB of a workgroup; the order fits its nibbles, the key its word
    assert U.THREADS * U.WORDS * 4 + 8 * 256 <= 65536 and U.MAX_NT <= 16 and U.MAX_BITS == 32
    assert U.form(4, 4, 16) == 16 and U.form(4, 4, 64) == 64 and U.form(8, 8, 32) == 32 and U.form(4, 4, 1) == 2


# ---------------------------------------------------------------- exact plantings

_PLANTED = {}


def _planted(case):
    if case[0] not in _PLANTED:
        name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
        H, Y, S, sent = U.planting(case)
        _PLANTED[case[0]] = (H, Y, S, sent, U.emulate(H, Y, S, n0, k, clip, srt),
                             U.reference(H, Y, S, n0, k, clip, srt))
    return _PLANTED[case[0]]


@pytest.mark.parametrize("case", U.PLANTINGS, ids=lambda c: c[0])
def test_plantings_are_exact(case):
    name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
    H, Y, S, sent, emu, ref = _planted(case)
    assert U.same(emu, U.rounded(ref)) is None
    # exact means exact: every metric is a multiple of 1 / 16 below 2^20
    assert (emu["metric"] * 16 == np.round(emu["metric"] * 16)).all() and emu["metric"].max() < 2.0 ** 20
    bare = U.emulate(H, Y, S, n0, k, clip, srt, llr=False)
    assert bare["llr"] is None and U.same(bare, emu, ("index", "status", "metric")) is None
    want = U.DEFICIENT if special == "null" or nr < nt else 0
    assert (emu["status"] == want).all()
    assert (np.abs(emu["llr"]) <= clip).all()
    if k == 1:                          # one leaf: every bit lacks its counter-hypothesis
        bits = np.moveaxis(DT.hard_bits(emu["index"], nt, B), (-2, -1), (2, 3))
        assert np.array_equal(emu["llr"], np.where(bits == 1, clip, -clip).astype(np.float32))


def test_plantings_cover_the_design():
    c = U.PLANTINGS
    assert {x[7] for x in c} >= {1, 2, 8, 64}
    g = {U.form(x[2], x[3], x[7]) for x in c}
    assert 64 in g and g & {1, 2, 4, 8, 16, 32}                         # both sides of the narrow/wide switch
    assert any(U.form(x[2], x[3], x[7]) > x[7] for x in c)              # a group wider than the list
    assert {x[3] for x in c} >= {1, 2, 4, 16} and {x[4] for x in c} >= {1, 2, 4, 8}
    assert {x[2] for x in c} >= {1, 4, 16, 64}
    assert any(x[3] * x[4] == 32 for x in c) and all(x[3] * x[4] <= 32 for x in c)
    assert {x[8] for x in c} == {True, False} and {x[9] for x in c} == {"perm", "had"}
    # a level with fewer than K candidates and a later one with more
    assert any((1 << x[4]) < x[7] < (1 << (x[3] * x[4])) for x in c)
    assert any(x[14] == "null" for x in c) and any(x[14] == "tie-norm" for x in c) and any(x[2] < x[3] for x in c)
    # a hypothesis beyond 2^31 (a key that is no int32)
    assert any(x[3] * x[4] == 32 and (_planted(x)[4]["index"] >= 1 << 31).any() for x in c)


def test_sorted_plantings_recover_the_planted_order_and_tie_norms_go_to_the_lower_stream():
    case = [x for x in U.PLANTINGS if x[14] == "tie-norm"][0]
    name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
    H, Y, S, sent, emu, ref = _planted(case)
    # the two tied columns have the same norm at their pick in every point ...
    n2 = (np.abs(U._points(H).astype(np.complex128)) ** 2).sum(-2).reshape(-1, nt)
    assert (np.sort(n2, -1)[:, 1] == np.sort(n2, -1)[:, 2]).all() and (ref["order_gap"] == 0).all()
    # ... and the reference (argmin, the first) and the emulation (a strict <) agree on who goes first
    assert U.same(emu, U.rounded(ref)) is None


@pytest.mark.parametrize("wrong", U.WRONG_READINGS)
def test_wrong_readings_are_caught(wrong):
    caught = []
    for case in U.PLANTINGS:
        name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
        if wrong == "sorted-descending" and not srt:
            continue
        H, Y, S, sent, emu, ref = _planted(case)
        if U.same(U.emulate(H, Y, S, n0, k, clip, srt, wrong=wrong), emu) is not None:
            caught.append(name)
    print(wrong, caught)
    assert caught
    if wrong == "ties-higher-key":      # the null level ties every child: the K-th place is a tie
        assert any("null" in n for n in caught)
    if wrong == "null-divided":
        assert all("null" in n or "wide" in n for n in caught)


def test_a_planting_prunes_the_ml_hypothesis():
    H, Y, S, n0, clip, k, srt = U.pruned_case()
    emu = U.emulate(H, Y, S, n0, k, clip, srt)
    assert U.same(emu, U.rounded(U.reference(H, Y, S, n0, k, clip, srt))) is None
    ml = DT.ml_reference(H, Y, S, n0)
    differs = emu["index"] != ml["index"]
    assert differs.any() and not differs.all()
    # where it differs the K-best leaf is the worse one, strictly; elsewhere the metrics are the same number
    assert (emu["metric"][differs] > ml["metric"][differs]).all()
    assert np.array_equal(emu["metric"][~differs], ml["metric"][~differs].astype(np.float32))
    # a list that holds every parent of the last level finds it again
    full = U.emulate(H, Y, S, n0, 16, clip, srt)
    assert np.array_equal(full["index"], ml["index"])


def test_exhaustive_limits_are_ml():
    # M^(Nt - 1) <= K: index and metric; M^Nt <= K: the LLRs too, clamped
    for case in U.PLANTINGS:
        name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
        if nt * B > 12 or (1 << ((nt - 1) * B)) > k or special or nr < nt:
            continue
        H, Y, S, sent, emu, ref = _planted(case)
        ml = DT.ml_reference(H, Y, S, n0)
        assert np.array_equal(emu["index"], ml["index"]), name
        assert np.array_equal(emu["metric"], ml["metric"].astype(np.float32)), name
        if (1 << (nt * B)) <= k:
            assert np.array_equal(emu["llr"], np.clip(ml["llr"], -clip, clip).astype(np.float32)), name
            print(name, "LLRs are ML's")
    names = [x[0] for x in U.PLANTINGS]
    assert "k64-3x3-b2-all" in names and "k64-2x2-b1-nr64" in names


def test_absent_counter_hypotheses_and_the_clamp():
    case = [x for x in U.PLANTINGS if x[0] == "k2-clamp-2x2-b2"][0]
    name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
    H, Y, S, sent, emu, ref = _planted(case)
    free = U.emulate(H, Y, S, n0, k, clip, srt, wrong="no-clamp")["llr"]
    cut = np.abs(free) > clip
    assert cut.any()                                            # a quotient the clamp cuts ...
    flipped = U.emulate(H, Y, S, n0, k, clip, srt, wrong="clip-sign")["llr"]
    lone = flipped != emu["llr"]
    assert lone.any() and not (lone & cut).any()                # ... and bits with one side absent
    assert (np.abs(emu["llr"][lone]) == clip).all()
    bits = np.moveaxis(DT.hard_bits(emu["index"], nt, B), (-2, -1), (2, 3))
    assert ((emu["llr"] > 0) == (bits == 1))[lone].all()


def test_the_zero_channel_and_non_finite_points():
    S = DT.qam(2, normalised=False).astype(np.complex64)
    rng = np.random.default_rng(5)
    H = np.zeros((1, 1, 3, 2, 2, 1, 3), np.complex64)
    Y = U.gaussian_integers(rng, (1, 1, 3, 2, 1, 3), 3)
    for k in (1, 4, 16):
        emu = U.emulate(H, Y, S, 0.5, k, 8.0)
        assert not emu["index"].any() and (emu["status"] == U.DEFICIENT).all()
        assert np.array_equal(emu["metric"], (np.abs(Y) ** 2).sum(2).astype(np.float32))
        assert U.same(emu, U.rounded(U.reference(H, Y, S, 0.5, k, 8.0))) is None
        if k == 16:                     # the list holds every hypothesis: all tie, the LLRs are +0
            assert not emu["llr"].any() and not np.signbit(emu["llr"]).any()
    case = U.PLANTINGS[4]
    name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
    H, Y, S, sent, clean, _ = _planted(case)
    for value in (np.nan, np.inf, 1e30):
        for where in ("H", "Y"):
            Hb, Yb = H.copy(), Y.copy()
            if where == "H":
                Hb[0, 1, 2, 1, 1, 0, 3] = value
            else:
                Yb[0, 1, 2, 1, 0, 3] = value
            emu = U.emulate(Hb, Yb, S, n0, k, clip, srt)
            flagged = np.zeros(emu["status"].shape, bool)
            flagged[0, 1, 1, 0, 3] = True
            assert np.array_equal(emu["status"], np.where(flagged, U.NONFINITE, clean["status"]))
            assert (emu["index"][flagged] == U.NO_INDEX).all() and not emu["metric"][flagged].any()
            assert not emu["llr"][0, 1, :, :, 1, 0, 3].any()
            assert np.array_equal(emu["index"][~flagged], clean["index"][~flagged])
            if value != 1e30:           # (its square is finite in float64: the reference does not flag it)
                assert U.same(emu, U.rounded(U.reference(Hb, Yb, S, n0, k, clip, srt))) is None
    # a quotient beyond float flags the point only with LLRs
    tiny = U.emulate(H, Y, S, 2.0 ** -140, 8, clip, srt)
    assert tiny["status"].any() and not U.emulate(H, Y, S, 2.0 ** -140, 8, clip, srt, llr=False)["status"].any()


# ---------------------------------------------------------------- the standard-normal cases: the cap and the bounds

_NORMAL = {}


def _normal(case):
    if case[0] not in _NORMAL:
        name, links, nr, nt, B, T, K, k, srt = case
        H, Y, S, sent = U.normal_case(case)
        _NORMAL[case[0]] = (H, Y, S, sent, U.emulate(H, Y, S, U.NOISE, k, U.CLIP, srt),
                            U.reference(H, Y, S, U.NOISE, k, U.CLIP, srt), U.scale(H, Y, S))
    return _NORMAL[case[0]]


@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_at_most_a_tenth_of_a_case_is_fragile(case):
    name, links, nr, nt, B, T, K, k, srt = case
    H, Y, S, sent, emu, ref, us = _normal(case)
    ok = U.sturdy(ref, nr, nt, srt)
    share = 1.0 - float(ok.mean())
    print("%s: %d points, fragile %.3f, gap below 1e-6: %.3f, below 1e-5: %.3f"
          % (name, ok.size, share, float((ref["gap"] < 1e-6).mean()), float((ref["gap"] < 1e-5).mean())))
    assert 30 <= ok.size <= 400 and share <= U.FRAGILE_CAP
    assert not ref["status"].any() and not emu["status"].any()
    assert U.index_agrees(emu, ref, us, ok, nr, nt)


def test_tolerance_constants_are_four_times_the_emulations_worst():
    metric = llr = 0.0
    for case in U.NORMAL_CASES:
        name, links, nr, nt, B, T, K, k, srt = case
        H, Y, S, sent, emu, ref, us = _normal(case)
        m, l = U.errors(emu, ref, us, U.NOISE, U.sturdy(ref, nr, nt, srt))
        print("%s: metric %.4f llr %.4f" % (name, m, l))
        metric, llr = max(metric, m), max(llr, l)
    assert 0.95 * U.METRIC_WORST <= metric <= U.METRIC_WORST, metric
    assert 0.95 * U.LLR_WORST <= llr <= U.LLR_WORST, llr
    assert U.METRIC_BOUND == 4 * U.METRIC_WORST and U.LLR_BOUND == 4 * U.LLR_WORST


def test_normal_cases_are_the_shapes_of_the_issue():
    shapes = {(x[2], x[3], x[4], x[7]) for x in U.NORMAL_CASES}
    assert shapes == {(4, 4, 4, 16), (4, 4, 6, 64), (8, 8, 2, 32), (2, 2, 4, 4), (64, 2, 2, 2), (3, 3, 2, 64)}
    for case in U.NORMAL_CASES:         # unit mean power
        assert abs((np.abs(U.normal_case(case)[2]) ** 2).mean() - 1.0) < 1e-6
