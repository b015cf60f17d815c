"""The maximum-likelihood detection's design on the CPU (csrc/hrt_detect.h, csrc/hrt_detect.hip; tests/detect_util.py):
the form rule and the LDS image built for the host over every (Nt, B), the float32 emulation on the exact plantings
(equal to the rounded float64 reference, bit for bit), the tolerance constants recomputed, the lead of the float64
reference over the case list (the index cap), the wrong readings of the definition that the cases separate, and the
QAM constellations against the tables of TS 38.211."""
import os
import subprocess

import numpy as np
import pytest

from hermespy_rt_amd import detect as DT

from . import detect_util as U


def _build(tmp_path, body, name):
    prog = tmp_path / (name + ".c")
    prog.write_text('#include <stdio.h>\n#include <stdlib.h>\n#include "hrt_detect.h"\n' + body)
    exe = tmp_path / name
    subprocess.check_call(["gcc", "-O1", "-std=gnu11", "-ffp-contract=off", "-I",
                           os.path.join(U.REPO, "hermespy-rt_amd", "csrc"), str(prog), "-o", str(exe)])
    return str(exe)


# ---------------------------------------------------------------- the form and the LDS image

def test_form_rule_built_for_the_host(tmp_path):
    exe = _build(tmp_path, "int main(void){for (unsigned nt = 0; nt <= 13; ++nt) for (unsigned b = 0; b <= 9; ++b) "
                 'printf("%u %u %u %u %u\\n", nt, b, hrt_detect_form(nt, b), hrt_detect_tiles(nt, b), '
                 "hrt_detect_lds_bytes(b)); "
                 'printf("%u %u %u %u %u %u %u\\n", HRT_DT_THREADS, HRT_DT_WAVES, HRT_DT_MAX_NR, HRT_DT_MAX_B, '
                 "HRT_DT_MAX_BITS, HRT_DT_MAX_M, HRT_DT_LANE_BITS); return 0;}\n", "form")
    lines = [[int(x) for x in l.split()] for l in subprocess.check_output([exe], text=True).splitlines()]
    assert lines[-1] == [U.THREADS, U.WAVES, U.MAX_NR, U.MAX_B, U.MAX_BITS, U.MAX_M, U.LANE_BITS]
    assert len(lines) - 1 == 14 * 10
    inside = set()
    for nt, b, g, tiles, lds in lines[:-1]:
        assert (g, tiles, lds) == (U.form(nt, b), U.tiles(nt, b), U.lds_bytes(b))
        ok = nt >= 1 and 1 <= b <= 8 and nt * b <= 12
        assert (g > 0) == ok and (tiles > 0) == ok
        if ok:
            Q = 1 << (nt * b)
            assert g == min(64, Q) and g * tiles == Q and 64 % g == 0
            assert lds == 8 << b <= 8 * U.MAX_M
            # a lane keeps 1 + 2 (Nt B - 6) minima at the most: 13 registers
            assert 1 + 2 * max(0, nt * b - U.LANE_BITS) <= 13
            inside.add((nt, b))
    assert sorted(inside) == sorted(U.all_shapes()) and len(inside) == 31
    assert U.THREADS == 64 * U.WAVES


@pytest.mark.parametrize("shape", U.all_shapes(), ids=lambda s: "nt%d-b%d" % s)
def test_bit_positions_and_lds_image_over_every_shape(tmp_path, shape):
    nt, B = shape
    exe = _build(tmp_path, "int main(int n, char **v){unsigned nt = atoi(v[1]), B = atoi(v[2]); "
                 'for (unsigned j = 0; j < nt; ++j) for (unsigned b = 0; b < B; ++b) printf("%u\\n", hrt_detect_bit(B, j, b)); '
                 'for (unsigned x = 0; x < (1u << B); ++x) printf("%u\\n", hrt_detect_slot(x)); return 0;}\n', "bits")
    got = np.array(subprocess.check_output([exe, str(nt), str(B)], text=True).split(), np.int64)
    pos, slots = got[:nt * B], got[nt * B:]
    assert np.array_equal(pos, [U.bit_position(B, j, b) for j in range(nt) for b in range(B)])
    # every bit of q is the bit of exactly one (stream, bit), and it is the bit the definition names
    assert np.array_equal(np.sort(pos), np.arange(nt * B))
    q = np.arange(1 << (nt * B))
    bits = DT.hard_bits(q, nt, B)
    for j in range(nt):
        for b in range(B):
            assert np.array_equal((q >> pos[j * B + b]) & 1, bits[:, j, b])
            x = (q >> (j * B)) & ((1 << B) - 1)
            assert np.array_equal(bits[:, j, b], (x >> (B - 1 - b)) & 1)
    # lane bits are the positions below 6, tile bits the rest; the tile is q >> 6
    g, tiles = U.form(nt, B), U.tiles(nt, B)
    assert np.array_equal(q // g, q >> min(U.LANE_BITS, nt * B)) and (q // g).max() == tiles - 1
    # the image: one float2 slot per symbol, every word has one owner, staged by thread w at slot w, w + 256, ..
    assert np.array_equal(slots, np.arange(1 << B)) and slots.size * 8 == U.lds_bytes(B) <= 2048


# ---------------------------------------------------------------- exact plantings

@pytest.mark.parametrize("case", U.INTEGER_CASES, ids=lambda c: c[0])
def test_gaussian_integer_plantings_are_exact(case):
    H, Y, S, n0, sent = U.integer_case(case)
    assert np.log2(n0) == np.round(np.log2(n0))
    assert np.array_equal(S.real % 2, np.ones(S.shape)) and (case[4] == 1 or np.array_equal(S.imag % 2, np.ones(S.shape)))
    ref = DT.ml_reference(H, Y, S, n0, table=True)
    d = ref["distances"]
    assert d.max() < 2 ** 24 and np.array_equal(d, np.round(d))
    assert not ref["status"].any()
    emu = U.emulate(H, Y, S, n0)
    assert U.same(emu, U.rounded(ref)) is None
    assert np.array_equal(U.emulate_distances(H, Y, S), d.astype(np.float32))
    # the offset is small: the planted hypothesis is within the offset's energy of the best
    planted = np.take_along_axis(d, sent[..., None], -1)[..., 0]
    assert (planted <= 2 * case[2]).all() and (ref["metric"] <= planted).all()


def test_integer_cases_cover_every_switch_of_the_form():
    cases = U.INTEGER_CASES
    assert {(c[3], c[4]) for c in cases} == {(1, 1), (1, 5), (1, 6), (1, 7), (1, 8), (2, 2), (3, 2), (2, 3), (6, 2),
                                             (3, 4), (2, 6), (12, 1), (4, 3)}
    assert {c[2] for c in cases} == {1, 2, 5, 64}
    assert all(1 << (c[3] * c[4]) <= 64 for c in cases if c[2] == 64)
    assert {(c[3], c[4]) for c in cases if c[2] == 64} == {(1, 1), (1, 5), (1, 6), (2, 2), (3, 2), (2, 3)}
    assert {c[5] * c[6] for c in cases} >= {1, 3, 4, 5, 7}
    assert any(c[5] > 1 and c[5] % 2 and c[6] > 1 and c[6] % 2 for c in cases)
    assert any(c[1] == (2, 2) for c in cases) and any(c[1] == (1, 2) for c in cases) and any(c[1] == (2, 1) for c in cases)
    # narrow shapes leave groups of the last wave empty, or fill it
    part = [(2 * c[5] * c[6] * c[1][0] * c[1][1]) % (64 // U.form(c[3], c[4])) for c in cases if U.form(c[3], c[4]) < 64]
    assert any(part) and not all(part)
    # both pols decide differently somewhere, and every LLR sign occurs
    differ = signs = 0
    for c in cases:
        H, Y, S, n0, _ = U.integer_case(c)
        r = DT.ml_reference(H, Y, S, n0)
        differ += bool((r["index"][:, :, 0] != r["index"][:, :, 1]).any())
        signs += bool((r["llr"] > 0).any() and (r["llr"] < 0).any())
    assert differ >= 10 and signs >= 15


@pytest.mark.parametrize("shape", ((1, 1, 1), (2, 3, 2), (5, 2, 6), (3, 12, 1), (64, 1, 6), (2, 1, 8), (2, 4, 3)),
                         ids=lambda s: "%dx%d-b%d" % s)
def test_one_hot_plantings_pin_every_row_stream_and_bit(shape):
    nr, nt, B = shape
    H, Y, S, want = U.one_hot_case(nr, nt, B)
    emu = U.emulate(H, Y, S, 1.0)
    assert U.same(emu, U.rounded(DT.ml_reference(H, Y, S, 1.0))) is None
    assert np.array_equal(emu["index"].ravel(), want) and not emu["metric"].any() and not emu["status"].any()
    assert set(want) == {(1 << (B - 1 - b)) << (j * B) for j in range(nt) for b in range(B)}
    # the deciding stream's LLRs name its symbol; the other streams tie: +0
    L = np.moveaxis(emu["llr"], (2, 3), (-2, -1)).reshape(-1, nt, B)
    bits = DT.hard_bits(want, nt, B)
    for p in range(want.size):
        j = int(np.flatnonzero(np.abs(_point(H, p)).sum(0))[0])
        assert ((L[p, j] > 0) == (bits[p, j] == 1)).all() and (L[p, j] != 0).all()
        others = np.delete(L[p], j, 0)
        assert not others.any() and not np.signbit(others).any()


def _point(H, p):
    return U._points(H).reshape((-1,) + H.shape[2:4])[p]


def test_planted_ties_return_the_lowest_index_and_zero_llrs():
    for name, H, Y, S, n0, want, zero_bits in U.tie_cases():
        nt, B = H.shape[3], S.shape[0].bit_length() - 1
        ref = DT.ml_reference(H, Y, S, n0, table=True)
        emu = U.emulate(H, Y, S, n0)
        assert U.same(emu, U.rounded(ref)) is None, name
        assert np.array_equal(emu["index"].ravel(), want), name
        d = ref["distances"].reshape(-1, ref["distances"].shape[-1])
        assert ((d == 0).sum(-1) == 1 << len(zero_bits)).all(), name
        L = np.moveaxis(emu["llr"], (2, 3), (-2, -1)).reshape(-1, nt * B)
        pos = [U.bit_position(B, j, b) for j in range(nt) for b in range(B)]
        for k, p in enumerate(pos):
            col = L[:, k]
            if p in zero_bits:
                assert not col.any() and not np.signbit(col).any(), name
            else:
                assert (col != 0).all(), name
        if name == "tile-edge":
            assert 63 in want and 0 in want and (d[want == 63][:, [63, 127]] == 0).all()
            assert U.form(nt, B) == 64 and U.tiles(nt, B) == 2


def test_the_zero_channel_ties_everywhere():
    for nt, B in ((2, 2), (7, 1), (3, 4)):
        rng = np.random.default_rng(nt)
        S = DT.qam(B, normalised=False).astype(np.complex64)
        H = np.zeros((1, 1, 3, nt, 2, 1, 3), np.complex64)
        Y = U.gaussian_integers(rng, (1, 1, 3, 2, 1, 3), 3)
        emu = U.emulate(H, Y, S, 0.5)
        assert not emu["index"].any() and not emu["status"].any() and not emu["llr"].any()
        assert not np.signbit(emu["llr"]).any()
        assert np.array_equal(emu["metric"], (np.abs(Y.astype(np.complex128)) ** 2).sum(2).astype(np.float32))
        assert U.same(emu, U.rounded(DT.ml_reference(H, Y, S, 0.5))) is None


def test_non_finite_points_are_flagged_alone():
    H, Y, S, _ = U.normal_case(U.NORMAL_CASES[0])
    clean = U.emulate(H, Y, S, U.NOISE)
    for value in (np.nan, np.inf, 1e30):
        for where in ("H", "Y"):
            Hb, Yb = H.copy(), Y.copy()
            if where == "H":
                Hb[0, 0, 1, 0, 1, 2, 3] = value
            else:
                Yb[0, 0, 1, 1, 2, 3] = value
            emu = U.emulate(Hb, Yb, S, U.NOISE)
            flagged = np.zeros(emu["status"].shape, bool)
            flagged[0, 0, 1, 2, 3] = True
            assert np.array_equal(emu["status"] != 0, flagged)
            assert (emu["index"][flagged] == U.NO_INDEX).all() and not emu["metric"][flagged].any()
            assert not emu["llr"][0, 0, :, :, 1, 2, 3].any()
            if value != 1e30:       # (a square beyond float is finite in float64: the reference does not flag it)
                assert np.array_equal(DT.ml_reference(Hb, Yb, S, U.NOISE)["status"], emu["status"])
            assert np.array_equal(emu["index"][~flagged], clean["index"][~flagged])
            assert np.array_equal(emu["metric"][~flagged], clean["metric"][~flagged])
            keep = np.broadcast_to(~flagged[:, :, None, None], emu["llr"].shape)
            assert np.array_equal(emu["llr"][keep], clean["llr"][keep])
    # an LLR beyond float flags the point when LLRs are asked for, and only then
    n0 = 2.0 ** -126
    tiny, ref = U.emulate(H, Y, S, n0), DT.ml_reference(H, Y, S, 1.0)
    over = (np.abs(ref["llr"]) > 8.0).any((2, 3))               # (4 is the edge: |m0 - m1| / 2^-126 beyond float)
    under = (np.abs(ref["llr"]) < 2.0).all((2, 3))
    assert over.any() and (tiny["status"][over] == U.NONFINITE).all() and not tiny["status"][under].any()
    assert not U.emulate(H, Y, S, n0, llr=False)["status"].any()


# ---------------------------------------------------------------- the tolerance and the lead

_NORMAL = {}


def _normal(case):
    if case[0] not in _NORMAL:
        H, Y, S, sent = U.normal_case(case)
        _NORMAL[case[0]] = (H, Y, S, sent, U.emulate(H, Y, S, U.NOISE), DT.ml_reference(H, Y, S, U.NOISE, table=True),
                            U.scale(H, Y, S))
    return _NORMAL[case[0]]


def test_tolerance_constants_are_four_times_the_emulations_worst():
    metric = llr = 0.0
    for case in U.NORMAL_CASES:
        H, Y, S, _, emu, ref, us = _normal(case)
        assert np.array_equal(emu["index"], ref["index"]), case[0]
        m, l = U.metric_error(emu["metric"], ref, us), U.llr_error(emu["llr"], ref, us, U.NOISE)
        print("%s: metric %.4f llr %.4f" % (case[0], m, l))
        metric, llr = max(metric, m), max(llr, l)
    assert 0.95 * U.METRIC_WORST <= metric <= U.METRIC_WORST, metric
    assert 0.95 * U.LLR_WORST <= llr <= U.LLR_WORST, llr
    assert U.METRIC_BOUND == 4 * U.METRIC_WORST and U.LLR_BOUND == 4 * U.LLR_WORST


@pytest.mark.parametrize("case", U.NORMAL_CASES, ids=lambda c: c[0])
def test_reference_lead_exceeds_twice_the_bound_on_every_point(case):
    _, _, _, _, emu, ref, us = _normal(case)
    assert U.lead_share(ref, us) == 1.0
    ok, second = U.index_check(emu["index"], ref, us)
    assert ok and second <= 0.05
    assert not ref["status"].any()


def test_normal_cases_cover_the_form():
    c = U.NORMAL_CASES
    assert 8 <= len(c) <= 10
    assert max(x[2] for x in c) == 16 and any(x[2] == 16 and x[3] * x[4] == 12 for x in c)
    assert {U.form(x[3], x[4]) for x in c} >= {2, 16, 32, 64} and {U.tiles(x[3], x[4]) for x in c} >= {1, 4, 64}
    assert {x[7] for x in c} == {"qam", "psk"}
    assert any(x[1] == (2, 2) for x in c) and any(x[5] > 1 for x in c)
    for x in c:                         # unit mean power
        S = U.normal_case(x)[2]
        assert abs((np.abs(S) ** 2).mean() - 1.0) < 1e-6


# ---------------------------------------------------------------- wrong readings

def _differs(r, w, us, noise):
    """whether a reading's result is told from the right one by the checks the GPU tests apply"""
    if w is None:
        return False
    if not np.array_equal(w["index"], r["index"]):
        return True
    if U.metric_error(w["metric"], r, us) > U.METRIC_BOUND:
        return True
    return U.llr_error(w["llr"], r, us, noise) > U.LLR_BOUND


@pytest.mark.parametrize("wrong", U.WRONG_READINGS)
def test_wrong_readings_are_caught(wrong):
    caught = []
    for case in U.INTEGER_CASES:
        H, Y, S, n0, _ = U.integer_case(case)
        r = DT.ml_reference(H, Y, S, n0)
        if _differs(r, U.reading(H, Y, S, n0, wrong), U.scale(H, Y, S), n0):
            caught.append(case)
    if wrong == "highest-on-ties":      # integer distances tie by themselves; the planted ties tell it at every point
        for name, H, Y, S, n0, want, _ in U.tie_cases():
            w = U.reading(H, Y, S, n0, wrong)
            assert (w["index"].ravel() > want).all(), name
        return
    assert caught, wrong
    if wrong == "H-transposed":
        assert all(c[2] == c[3] for c in caught)
    if wrong in ("Y-pol-time-swapped", "out-pol-time-swapped"):
        assert all(c[5] > 1 for c in caught)
    if wrong == "noise-multiplied":
        assert all(c[7] != 1.0 for c in caught)
    if wrong in ("digits-reversed", "llr-streams-reversed"):
        assert all(c[3] > 1 for c in caught)
    if wrong == "bits-lsb-first":
        assert all(c[4] > 1 for c in caught)


# ---------------------------------------------------------------- constellations

def _table_38211(B):
    """TS 38.211 sections 5.1.3 to 5.1.6, written out from their formulas bit by bit"""
    out = np.empty(1 << B, np.complex128)
    for x in range(1 << B):
        b = [(x >> (B - 1 - i)) & 1 for i in range(B)]
        s = [1 - 2 * v for v in b]
        if B == 2:
            out[x] = (s[0] + 1j * s[1]) / np.sqrt(2)
        elif B == 4:
            out[x] = (s[0] * (2 - s[2]) + 1j * s[1] * (2 - s[3])) / np.sqrt(10)
        elif B == 6:
            out[x] = (s[0] * (4 - s[2] * (2 - s[4])) + 1j * s[1] * (4 - s[3] * (2 - s[5]))) / np.sqrt(42)
        else:
            out[x] = (s[0] * (8 - s[2] * (4 - s[4] * (2 - s[6])))
                      + 1j * s[1] * (8 - s[3] * (4 - s[5] * (2 - s[7])))) / np.sqrt(170)
    return out


@pytest.mark.parametrize("B", (2, 4, 6, 8))
def test_qam_follows_ts_38211(B):
    S = DT.qam(B)
    assert np.allclose(S, _table_38211(B), atol=1e-15)
    assert abs((np.abs(S) ** 2).mean() - 1.0) < 1e-12
    raw = DT.qam(B, normalised=False)
    side = 1 << (B // 2)
    odd = np.arange(-(side - 1), side, 2)
    assert np.array_equal(np.unique(raw.real), odd) and np.array_equal(np.unique(raw.imag), odd)
    assert len(np.unique(raw)) == 1 << B
    # Gray: nearest neighbours (distance 2) differ in exactly one bit
    x = np.arange(1 << B)
    near = np.abs(raw[:, None] - raw[None, :]) == 2
    flips = np.array([[bin(a ^ b).count("1") for b in x] for a in x])
    assert near.sum() == 2 * 2 * side * (side - 1) and (flips[near] == 1).all()


def test_odd_qam_psk_and_the_bit_helpers():
    for B in (1, 3, 5, 7):
        raw = DT.qam(B, normalised=False)
        assert len(np.unique(raw)) == 1 << B and np.array_equal(np.abs(raw.real) % 2, np.ones(1 << B))
        assert abs((np.abs(DT.qam(B)) ** 2).mean() - 1.0) < 1e-12
    assert np.array_equal(DT.qam(1, normalised=False), [1, -1])
    for B in (1, 2, 3, 4):
        S = DT.psk(B)
        assert np.allclose(np.abs(S), 1.0)
        order = np.argsort(np.angle(S * np.exp(-1e-9j)) % (2 * np.pi))
        assert all(bin(int(a) ^ int(b)).count("1") == 1 for a, b in zip(order, np.roll(order, 1))) or B == 1
    rng = np.random.default_rng(0)
    nt, B = 3, 4
    q = rng.integers(0, 1 << (nt * B), (5, 7))
    x = DT.hypothesis_symbols(q, nt, B)
    assert np.array_equal(DT.hypothesis(x, B), q) and x.shape == (5, 7, nt)
    bits = DT.hard_bits(q, nt, B)
    assert np.array_equal(DT.symbol_indices(bits, B), x)
    S = DT.qam(B)
    assert np.array_equal(DT.modulate(bits, S), S[x]) and np.array_equal(DT.modulate(bits.ravel(), S), S[x].ravel())
    assert DT.bit_errors(bits, bits) == 0 and DT.bit_errors(bits, 1 - bits) == bits.size
    assert not DT.hard_bits(np.array([U.NO_INDEX, -1]), nt, B).any()


def test_linear_llrs_agree_with_ml_on_a_diagonal_channel():
    """with orthogonal columns the streams decouple, and the linear receiver's max-log LLRs are the ML ones"""
    rng = np.random.default_rng(4)
    nt, B, n0 = 2, 2, 0.5
    S = DT.qam(B)
    H = np.zeros((1, 1, 2, nt, 2, 1, 4), np.complex128)
    g = rng.uniform(0.5, 2.0, (nt, 2, 1, 4)) * np.exp(2j * np.pi * rng.random((nt, 2, 1, 4)))
    for j in range(nt):
        H[0, 0, j, j] = g[j]
    Y = (rng.standard_normal((1, 1, 2, 2, 1, 4)) + 1j * rng.standard_normal((1, 1, 2, 2, 1, 4)))
    ref = DT.ml_reference(H, Y, S, n0)
    # zero-forcing: W = H^-1, sinr = |g|^2 / N0
    W = np.zeros((1, 1, nt, 2, 2, 1, 4), np.complex128)
    for j in range(nt):
        W[0, 0, j, j] = 1.0 / g[j]
    sinr = (np.abs(g) ** 2 / n0)[None, None]
    assert np.allclose(DT.linear_llrs(W, sinr, Y, S, "zf"), ref["llr"], rtol=1e-10, atol=1e-10)
    # LMMSE: W = conj(g) / (|g|^2 + N0), unbiased sinr the same
    for j in range(nt):
        W[0, 0, j, j] = np.conj(g[j]) / (np.abs(g[j]) ** 2 + n0)
    assert np.allclose(DT.linear_llrs(W, sinr, Y, S, "lmmse"), ref["llr"], rtol=1e-10, atol=1e-10)
