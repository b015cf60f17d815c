"""The design of the tests of the beam taps of path lists (tests/sparse_beam_taps_util.py), without a device: for every
planted case the outputs are Gaussian integers whose intermediates stay below 2^24 in modulus, in float64 (the governing
quantity n max|a| ||W_rx[a]||_1 ||W_tx[b]||_1) and under a float32 mirror of the kernel's gain, U, sinc and accumulation
stages; the library's float64 reference agrees with an independent per-path loop, with beams.apply of the array taps'
reference and, through a DTFT, with the beam channel's reference; no live case expects an all-zero tensor; a mirror of
the tiling rule shows each edge case reaches the form, the blocks and the beam slots it names; and the cases catch each
wrong reading a kernel could make."""
import numpy as np
import pytest

from hermespy_rt_amd import beams, sparse

from . import sparse_beam_taps_util as U


def _is_gaussian_integer(h):
    return np.array_equal(h.real, np.rint(h.real)) and np.array_equal(h.imag, np.rint(h.imag))


def _exact(c, v, re, te, wr, wt, reading=None):
    return U.exact_reference(v, re, te, wr, wt, c["l_min"], c["L"], c["T"], reading)


@pytest.mark.parametrize("name", sorted(U.CASES))
def test_every_case_is_exact_in_float64_and_under_the_float32_mirror(name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    # the governing quantity bounds every intermediate: tile sums and gains by ||W||_1, G and U by their product times
    # max|a|, the accumulators by n times that (a sinc weight is 1 or 0)
    gov = U.governing(v, wr, wt)
    assert gov < U.LIMIT, (name, gov)
    assert U.A_MAX * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max()) < U.LIMIT
    E = _exact(c, v, re, te, wr, wt)
    assert E.shape == (c["nrx"], c["ntx"], c["br"], c["bt"], 2, c["T"], c["L"])
    assert _is_gaussian_integer(E) and np.abs(E).max() <= gov + 0.5
    live = np.minimum(v["kept"], np.uint64(c["K"])) > 0
    for rx, tx in np.argwhere(live):                                   # no live link expects an all-zero tensor
        assert E[rx, tx].any(), (name, rx, tx)
    assert not E[~live].any()
    M, peak = U.mirror_f32(v, re, te, wr, wt, U.F_A, U.FS, U.FC, c["l_min"], c["L"], c["T"])
    assert peak < U.LIMIT, (name, peak)
    U.check_exact(M, E, name)


def test_the_planting_has_delays_at_both_window_edges_and_one_beyond_each():
    for name in ("K33_rt4", "K33_rt1", "taps64_0", "taps257_rt1"):
        c = U.CASES[name]
        v = U.build(c)[0]
        q = set(U.TU.delays(v).ravel() - c["l_min"])
        assert {-1, 0, c["L"] - 1, c["L"]} <= q, (name, sorted(q))


def test_the_tiling_rule_reaches_the_forms_blocks_and_beam_slots_the_cases_name():
    def til(name):
        c = U.CASES[name]
        return U.tiling(c["br"], c["bt"], c["T"], c["L"])

    # the two forms, and their switch at Br Bt T = 13
    for name, c in U.CASES.items():
        t = til(name)
        assert t["form"] == ("<4, 4, 4>" if c["br"] * c["bt"] * c["T"] >= 13 else "<1, 4, 1>"), name
        assert name.endswith("rt1") == (t["form"] == "<1, 4, 1>") or not name.endswith(("rt1", "rt4")), name
    for name, form in (("form2x3x2", "<1, 4, 1>"), ("form4x1x3", "<1, 4, 1>"), ("form1x1x1", "<1, 4, 1>"),
                       ("form13x1x1", "<4, 4, 4>"), ("form1x13x1", "<4, 4, 4>"), ("form1x1x13", "<4, 4, 4>")):
        assert til(name)["form"] == form
    assert til("form2x3x2")["rblocks"] == 3 and til("K33_rt1")["cap"] == 4       # 12 rows: three blocks of 4
    # the <1, 4, 1> form with 2 x 3 beams and T = 2: every block holds two pairs; TX slot s is beam s (Bt = 3 <= 4)
    assert all(b["tx_all"] and b["nb"] == 3 for b in til("K33_rt1")["blocks"])
    assert [b["na"] for b in til("K33_rt1")["blocks"]] == [1, 2, 1]               # the middle block spans two RX beams
    # the row-block edges with T = 1: 63, 64, 65 and 130 pairs
    assert [til("rows%s" % s)["rblocks"] for s in ("7x9x1", "8x8x1", "5x13x1", "10x13x1")] == [1, 1, 2, 3]
    # T = 3: 63 rows in one block; 66 rows: the second block begins inside pair 21
    assert til("rows3x7x3")["rblocks"] == 1
    b = til("rows2x11x3")["blocks"]
    assert len(b) == 2 and b[1]["inside"] and b[1]["pf"] == 21 and b[0]["pl"] == 21
    # T = 64: a pair fills a block; T = 65: the second block begins inside pair 0 and ends inside pair 1
    assert [(x["pf"], x["pl"], x["inside"]) for x in til("T64")["blocks"]] == [(0, 0, False), (1, 1, False)]
    assert [(x["pf"], x["pl"], x["inside"]) for x in til("T65")["blocks"]] == [(0, 0, False), (0, 1, True), (1, 1, True)]
    # Br = 65, Bt = 1: 64 RX slots, then one; Br = 256: four blocks of 64 RX slots
    assert [x["na"] for x in til("br65")["blocks"]] == [64, 1] and [x["na"] for x in til("br256")["blocks"]] == [64] * 4
    # Br = 1: Bt = 63, 64 fit the block (TX slot s is beam s); Bt = 65, 256 do not (the beam of pair pf + s)
    assert [til("bt%d" % n)["blocks"][0]["tx_all"] for n in (63, 64, 65, 256)] == [True, True, False, False]
    assert [x["nb"] for x in til("bt65")["blocks"]] == [64, 1] and [x["nb"] for x in til("bt256")["blocks"]] == [64] * 4
    # Bt = 65 with 3 RX beams: blocks 1 .. 3 wrap from TX beam 64 to 0 inside the block, over two RX beams; a0 differs
    # from ceil(pf / Bt) there; two column blocks
    t = til("bt65_wrap")
    assert t["rblocks"] == 4 and t["cblocks"] == 2
    for x in t["blocks"][1:3]:
        assert not x["tx_all"] and x["na"] == 2 and x["pf"] % 65 + x["nb"] > 65 and -(-x["pf"] // 65) != x["a0"]
    assert any(x["inside"] and not x["tx_all"] for x in til("bt65_T3")["blocks"])
    # the column blocks: 4 tiles a block in the <4, 4, 4> form, 16 in the <1, 4, 1> form
    assert [til("taps%d_0" % n)["cblocks"] for n in (1, 15, 16, 17, 63, 64, 65)] == [1, 1, 1, 1, 1, 1, 2]
    assert [til("taps%d_rt1" % n)["cblocks"] for n in (255, 256, 257)] == [1, 1, 2]


@pytest.mark.parametrize("name", ["K33_rt4", "links5", "rows2x11x3", "rx33"])
def test_float64_reference_gives_the_exact_values(name):
    c = U.CASES[name]
    v, re, te, wr, wt = U.build(c)
    E = _exact(c, v, re, te, wr, wt)
    h, S = sparse.beam_taps_reference(v, re, te, wr, wt, U.F_A, U.FS, U.FC, c["l_min"] + np.arange(c["L"]),
                                      U.T0 + U.DT * np.arange(c["T"]))
    # float64 exp of a whole number of quarter revolutions, numpy's sinc within 1e-16 of 0 off the tap
    scale = float(S.max()) * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max())
    assert np.abs(h - E).max() <= 1e-9 * max(scale, 1.0)
    assert np.array_equal(np.rint(h.real) + 1j * np.rint(h.imag), E)


def test_mirror_is_not_exact_off_the_planting():
    """the mirror rounds: off the lattice it differs from float64, so its exactness above is the planting's"""
    c = U.CASES["K33_rt4"]
    v, re, te, wr, wt = U.build(c)
    v["tau"][...] = v["tau"] * np.float32(1.37)
    re = (re * np.float32(1.013)).astype(np.float32)
    h, S = sparse.beam_taps_reference(v, re, te, wr, wt, U.F_A, U.FS, U.FC, c["l_min"] + np.arange(c["L"]),
                                      U.T0 + U.DT * np.arange(c["T"]))
    M, _ = U.mirror_f32(v, re, te, wr, wt, U.F_A, U.FS, U.FC, c["l_min"], c["L"], c["T"])
    scale = float(S.max()) * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max())
    err = np.abs(M - h).max()
    assert 0 < err <= 1e-5 * scale


def test_reference_against_the_per_path_loop_the_contracted_array_taps_and_the_beam_channel():
    rng = np.random.default_rng(11)
    nrx, ntx, K = 2, 2, 5
    n = 14
    link = rng.integers(0, 3, n)                      # link 3 stays empty
    u = rng.normal(size=(2, n, 3))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    fs, fc, fa = 20e6, 3.5e9, 3.5e9
    v = sparse.cluster_list(nrx, ntx, K, link, rng.normal(size=n) + 1j * rng.normal(size=n),
                            rng.normal(size=n) + 1j * rng.normal(size=n), rng.uniform(0, 1e-6, n),
                            rng.uniform(-200, 200, n), u[0], u[1])
    assert v["kept"][1, 1] == 0 and (v["eligible"] > v["kept"]).any()
    re, te = rng.uniform(-0.1, 0.1, (3, 3)).astype(np.float32), rng.uniform(-0.1, 0.1, (2, 3)).astype(np.float32)
    wr = (rng.normal(size=(2, 3)) + 1j * rng.normal(size=(2, 3))).astype(np.complex64)
    wt = (rng.normal(size=(4, 2)) + 1j * rng.normal(size=(4, 2))).astype(np.complex64)
    l, t = np.arange(-2, 4), 1e-3 * np.arange(3)
    h, S = sparse.beam_taps_reference(v, re, te, wr, wt, fa, fs, fc, l, t)
    scale = S.max() * np.abs(wr).sum(axis=1).max() * np.abs(wt).sum(axis=1).max()
    loop = U.loop_reference(v, re, te, wr, wt, fa, fs, fc, l, t)
    assert h.shape == (2, 2, 2, 4, 2, 3, 6) and np.abs(h - loop).max() <= 1e-9 * scale and np.abs(h).max() > 0
    assert not h[1, 1].any()
    he, S2 = sparse.taps_reference(v, re, te, fa, fs, fc, l, t)
    assert np.array_equal(S, S2)
    assert np.abs(h - beams.apply(he, wr, wt)).max() <= 1e-12 * scale
    # slots at or beyond kept are not read
    live = np.arange(K) < v["kept"][..., None].astype(np.int64)
    w = U.copy(v)
    w["a_te"][~live] = np.nan
    w["u_tx"][~live] = np.nan
    h2, _ = sparse.beam_taps_reference(w, re, te, wr, wt, fa, fs, fc, l, t)
    assert np.array_equal(h, h2)
    # a DTFT of the taps is the beam channel: sum_l h[l] e^{-j 2 pi f l / f_s} = B(f_c + f) for |f| < f_s / 2, the sinc
    # series of a band-limited exponential, truncated where its tail is below the tolerance
    wide = np.arange(-6000, 6001)
    hw, _ = sparse.beam_taps_reference(v, re, te, wr, wt, fa, fs, fc, wide, t)
    f = np.array([-0.2, 0.0, 0.1]) * fs
    D = np.einsum("...l,lk->...k", hw, np.exp(-2j * np.pi * wide[:, None] * f[None, :] / fs))
    B, _ = sparse.beam_reference(v, re, te, wr, wt, fa, fc + f, t)
    assert np.abs(D - B).max() <= 1e-3 * scale and np.abs(B).max() > 0.1 * scale / n


def test_exact_reference_against_the_per_path_loop():
    for c in (U.case(ntx=2, K=5, kept=[[5, 3]], nr=2, nt=3, br=2, bt=3, T=2, L=6, l_min=-2, salt=1),
              U.case(K=4, nr=2, nt=2, br=2, bt=7, T=1, L=4, l_min=1, salt=2)):
        v, re, te, wr, wt = U.build(c)
        loop = U.loop_reference(v, re, te, wr, wt, U.F_A, U.FS, U.FC, c["l_min"] + np.arange(c["L"]),
                                U.T0 + U.DT * np.arange(c["T"]))
        # cmath.exp of phases up to 2^15 revolutions, sin(pi k) / (pi k) of integer k within 1e-16 of 0
        assert np.abs(loop - _exact(c, v, re, te, wr, wt)).max() <= 1e-6


@pytest.mark.parametrize("name", U.MUTANTS)
def test_planted_cases_catch_each_wrong_reading(name):
    """every wrong reading gives a different value somewhere on the planted cases, so the exact comparison on the
    device catches it"""
    caught = []
    for cn in U.MUTANT_CASES:
        c = U.CASES[cn]
        v, re, te, wr, wt = U.build(c)
        E = _exact(c, v, re, te, wr, wt)
        W = U.mutant(name, v, re, te, wr, wt, c["l_min"], c["L"], c["T"])
        assert name == "gain_as_phase" or _is_gaussian_integer(W)
        if not np.array_equal(E, W):
            with pytest.raises(AssertionError):
                U.check_exact(W.astype(np.complex64), E)
            caught.append(cn)
    assert len(caught) >= 1, (name, caught)
    print(name, "moves the reference on", caught)


def test_one_hot_lists_and_codebooks_hit_every_index_once():
    """one live slot with one nonzero component at one tap and one-hot codebooks: the output is nonzero on that link,
    beam pair, polarisation and tap only, there of the weights' modulus at every m"""
    l_min, L, nt = -2, 5, 2
    re, te = U.elements(2, 3)
    for link in range(3):
        for k in range(L):
            v = U.one_hot(1, 3, link, link % 4, l_min + k, salt=link)
            for a in range(2):
                for b in range(3):
                    wr = U.one_hot_codebook(2, 2, a, (a + link) % 2, 1 + 2j)
                    wt = U.one_hot_codebook(3, 3, b, (b + link) % 3, 2 - 1j)
                    E = U.exact_reference(v, re, te, wr, wt, l_min, L, nt)
                    assert np.array_equal(np.abs(E[0, link, a, b, (link % 4) // 2, :, k]), np.full(nt, 5.0))
                    E[0, link, a, b, (link % 4) // 2, :, k] = 0
                    assert not E.any()
