"""What tests/test_sparse_beam_taps_design.py, tests/test_sparse_beam_taps_args.py (no device) and the GPU tests of the
beam taps of path lists (Tracer.sparse_beam_taps) share: the exact planting, an independent per-path loop, a float32
mirror of the kernel's gain, U, sinc and accumulation stages, a mirror of the tiling rule, the wrong readings a kernel
could make (MUTANTS), the cases and the exact check.

The planting is the product of tests/sparse_taps_util.py's and tests/sparse_beam_util.py's: elements on the 1/32 m
lattice, f_a = 8 c, directions on the axes, amplitude components in {0, +-1, +-2}, f_s = 2^18 Hz, f_c = 2^16 Hz and
tau = q 2^-18 s with integer q (a sinc weight is exactly 1 or +-0 and every phase a whole number of quarter
revolutions), and sparse_beam_util.codebook's Gaussian-integer weights.  Every gain, every U and every output is then a
Gaussian integer, exact in float32 in any summation order while its modulus stays below 2^24.  The governing quantity is

    n max|a| ||W_rx[a]||_1 ||W_tx[b]||_1,      max|a| = |2 + 2j|

so the cases with K = 1 024 use small codebooks and the cases with 256 elements a side a small K
(tests/test_sparse_beam_taps_design.py proves the bound and the mirror's exactness for every case below)."""
import cmath
import math

import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import covariance_util as CU
from . import sparse_beam_util as BU
from . import sparse_taps_util as TU
from . import sparse_util as SU

F_A, FS, FC, T0, DT, TAU_STEP = TU.F_A, TU.FS, TU.FC, TU.T0, TU.DT, TU.TAU_STEP
BATCH, ETILE = 32, 32            # HRT_TP_BATCH (csrc/hrt_taps.h), HRT_BM_ETILE (csrc/hrt_beam_channel.h)
LIMIT, A_MAX = BU.LIMIT, BU.A_MAX
planted, one_hot, copy, elements, check_exact = TU.planted, TU.one_hot, TU.copy, TU.elements, TU.check_exact
codebook, one_hot_codebook = BU.codebook, BU.one_hot_codebook


# ------------------------------------------------------------------ the tiling rule (csrc/host/channel.c taps_grid)
def tiling(br, bt, T, L):
    """A mirror of the tiling rule: dict(form, cap, rblocks, cblocks, blocks) where cap is the rows of a block (64 in
    the <4, 4, 4> form, 4 in the <1, 4, 1> form) and blocks lists, per row block, dict(row0, row1, pf, pl, a0, na, nb,
    tx_all, inside): the first and last row and pair, the RX and TX beam slots of csrc/hrt_beam_taps.h, and whether
    the block begins inside a pair"""
    rows = br * bt * T
    rtiles, ctiles = (4 * rows + 15) // 16, (L + 15) // 16
    rt = 4 if rtiles >= 4 else 1
    cap = 64 if rt == 4 else 4
    brows, bcols = (16, 4) if rt == 4 else (1, 16)
    rblocks, cblocks = (rtiles + brows - 1) // brows, (ctiles + bcols - 1) // bcols
    blocks = []
    for rb in range(rblocks):
        row0, row1 = rb * cap, min(rb * cap + cap, rows) - 1
        pf, pl = row0 // T, row1 // T
        a0, tx_all = pf // bt, bt <= cap
        blocks.append(dict(row0=row0, row1=row1, pf=pf, pl=pl, a0=a0, na=pl // bt - a0 + 1,
                           nb=bt if tx_all else pl - pf + 1, tx_all=tx_all, inside=row0 % T != 0))
    return dict(form="<4, 4, 4>" if rt == 4 else "<1, 4, 1>", cap=cap, rblocks=rblocks, cblocks=cblocks, blocks=blocks)


# ------------------------------------------------------------------ the cases
def case(nrx=1, ntx=1, K=9, kept=None, nr=2, nt=3, br=2, bt=7, T=2, L=17, l_min=-3, fill_r=None, fill_t=None, salt=0):
    """the parameters of a planted case: a dict; kept defaults to K on every link.  (2 x 7 beams, T = 2: 28 rows, the
    <4, 4, 4> form; 2 x 3 beams, T = 2: 12 rows, the <1, 4, 1> form)"""
    return dict(nrx=nrx, ntx=ntx, K=K, kept=K if kept is None else kept, nr=nr, nt=nt, br=br, bt=bt, T=T, L=L,
                l_min=l_min, fill_r=fill_r, fill_t=fill_t, salt=salt)


RT1, RT4 = dict(br=2, bt=3), dict(br=2, bt=7)
CASES = {}
for _f, _s in (("rt1", RT1), ("rt4", RT4)):
    for _k in (1, 3, 4, 5, 31, 32, 33, 1024):              # the MFMA step, the batch edge and the largest list
        CASES["K%d_%s" % (_k, _f)] = case(K=_k, salt=_k, **_s)
    for _kept in (0, 1, 32):                               # kept below the list length
        CASES["kept%d_%s" % (_kept, _f)] = case(K=33, kept=_kept, salt=3, **_s)
CASES["links5"] = case(ntx=5, K=33, kept=[[0, 1, 33, 32, 7]], nr=3, nt=5, br=3, bt=11, T=3, L=17, l_min=-40, salt=9)
CASES["links5_rt1"] = case(ntx=5, K=33, kept=[[0, 1, 33, 32, 7]], nr=3, nt=5, br=2, bt=3, T=2, L=17, l_min=-40, salt=9)
for _br, _bt, _t in ((2, 3, 2), (13, 1, 1), (4, 1, 3), (1, 13, 1), (1, 1, 1), (1, 1, 13)):   # Br Bt T = 12, 13, 1
    CASES["form%dx%dx%d" % (_br, _bt, _t)] = case(K=33, br=_br, bt=_bt, T=_t, salt=_br + _t)
for _br, _bt, _t in ((7, 9, 1), (8, 8, 1), (5, 13, 1), (10, 13, 1), (3, 7, 3), (2, 11, 3)):   # 63, 64, 65, 130 pairs; 63, 66 rows
    CASES["rows%dx%dx%d" % (_br, _bt, _t)] = case(br=_br, bt=_bt, T=_t, l_min=2, salt=_br * _t)
for _t in (64, 65):                                        # a pair fills a block / a block begins inside a pair
    CASES["T%d" % _t] = case(K=5, br=1, bt=2, T=_t, L=5, l_min=0, salt=_t)
CASES["br65"] = case(K=33, br=65, bt=1, nr=3, nt=4, T=1, L=5, salt=65)
for _bt in (63, 64, 65, 256):                              # the TX slots: every beam fits / the beam of pair pf + s
    CASES["bt%d" % _bt] = case(K=33, br=1, bt=_bt, nr=3, nt=4, T=1, L=5, salt=_bt)
CASES["bt65_wrap"] = case(K=33, br=3, bt=65, nr=3, nt=4, T=1, L=65, salt=6)    # four row blocks x two column blocks
CASES["bt65_T3"] = case(K=33, br=2, bt=65, nr=3, nt=4, T=3, L=5, salt=8)        # blocks that begin inside a pair
CASES["br256"] = case(K=33, br=256, bt=1, nr=4, nt=3, T=1, L=5, salt=5)
for _n in (1, 31, 32, 33, 64, 256):                        # element tiles, on either side and on both
    _kk = 5 if _n == 256 else 33
    CASES["rx%d" % _n] = case(K=_kk, nr=_n, nt=3, T=1, L=5, salt=_n)
    CASES["tx%d" % _n] = case(K=_kk, nr=2, nt=_n, T=1, L=5, salt=_n + 1)
    CASES["both%d" % _n] = case(K=_kk, nr=_n, nt=_n, T=1, L=5, salt=_n + 2)
CASES["K1024_sparse"] = case(K=1024, nr=33, nt=64, fill_r=3, fill_t=4, T=1, L=5, salt=7)
for _lm in (-70, 0, 9):                                    # column tile and column block edges, the <4, 4, 4> form
    for _l in (1, 15, 16, 17, 63, 64, 65):
        CASES["taps%d_%d" % (_l, _lm)] = case(K=33, T=1, L=_l, l_min=_lm, salt=_l)
for _l, _lm in ((255, -300), (256, 0), (257, 11)):         # the <1, 4, 1> form: 16 column tiles a block
    CASES["taps%d_rt1" % _l] = case(K=33, L=_l, l_min=_lm, salt=_l, **RT1)
# the cases the wrong readings are tried on
MUTANT_CASES = ("links5", "links5_rt1", "bt65_wrap", "bt65_T3", "rows2x11x3", "rx33", "tx64", "both33", "K33_rt4",
                "kept32_rt4", "taps17_9")


def build(c):
    """(v, re, te, wr, wt) of a case.  Slot 0 of every link lies inside the tap window and has a non-zero amplitude, so
    that a link with one live slot does not expect zeros"""
    v = planted(c["nrx"], c["ntx"], c["K"], c["kept"], c["l_min"], c["L"], c["salt"])
    v["tau"][:, :, 0] = np.float32((c["l_min"] + min(1, c["L"] - 1)) * TAU_STEP)
    dead = (v["a_te"][:, :, 0] == 0) & (v["a_tm"][:, :, 0] == 0)
    v["a_te"][:, :, 0] = np.where(dead, np.complex64(1 + 2j), v["a_te"][:, :, 0])
    re, te = elements(c["nr"], c["nt"])
    return (v, re, te, codebook(c["br"], c["nr"], 0, c["fill_r"], c["salt"]),
            codebook(c["bt"], c["nt"], 1, c["fill_t"], c["salt"]))


governing = BU.governing


# ------------------------------------------------------------------ references
def loop_reference(v, re, te, wr, wt, fa, fs, fc, l, t):
    """h of include/hermespy_rt.h by a direct loop over links, slots, beams, elements, polarisations, times and taps
    with cmath and math: shares nothing with sparse.beam_taps_reference but the definition"""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float64), np.asarray(te, np.float64)
    h = np.zeros((nrx, ntx, len(wr), len(wt), 2, len(t), len(l)), np.complex128)
    for rx in range(nrx):
        for tx in range(ntx):
            for p in range(min(int(v["kept"][rx, tx]), K)):
                amp = (complex(v["a_te"][rx, tx, p]), complex(v["a_tm"][rx, tx, p]))
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                urx, utx = v["u_rx"][rx, tx, p].astype(np.float64), v["u_tx"][rx, tx, p].astype(np.float64)
                w = []
                for li in l:
                    x = math.pi * (float(li) - fs * tau)
                    w.append(1.0 if x == 0.0 else math.sin(x) / x)
                for a in range(len(wr)):
                    g_rx = sum(complex(wr[a][i]).conjugate() * cmath.exp(
                        2j * cmath.pi * fa * sum(re[i][q] * urx[q] for q in range(3)) / sparse.SPEED_OF_LIGHT)
                        for i in range(len(re)))
                    for b in range(len(wt)):
                        g_tx = sum(complex(wt[b][j]) * cmath.exp(
                            2j * cmath.pi * fa * sum(te[j][q] * utx[q] for q in range(3)) / sparse.SPEED_OF_LIGHT)
                            for j in range(len(te)))
                        for pol in range(2):
                            for m in range(len(t)):
                                ph = amp[pol] * g_rx * g_tx * cmath.exp(2j * cmath.pi * (nu * t[m] - fc * tau))
                                for k in range(len(l)):
                                    h[rx, tx, a, b, pol, m, k] += ph * w[k]
    return h


_UNIT = np.array([1, 1j, -1, -1j])


def exact_reference(v, re, te, wr, wt, l_min, L, nt, reading=None):
    """the Gaussian-integer h of a planted list and planted codebooks on the exact grid, from the phases counted in
    quarter revolutions and the taps as integers: complex128 [nrx, ntx, Br, Bt, 2, nt, L], every value exact (sums of
    integers below 2^53).  reading: one of the wrong readings (CODE_MUTANTS) below."""
    nrx, ntx, K = v["tau"].shape
    kr = np.rint(np.asarray(re, np.float64) / CU.STEP).astype(np.int64)
    kt = np.rint(np.asarray(te, np.float64) / CU.STEP).astype(np.int64)
    wr, wt = np.asarray(wr).astype(np.complex128), np.asarray(wt).astype(np.complex128)
    br, bt = wr.shape[0], wt.shape[0]
    cr, ct = np.conj(wr), wt
    if reading == "conj_on_tx":
        cr, ct = wr, np.conj(wt)
    if reading == "steering_sign":
        kr, kt = -kr, -kt
    if reading == "weight_index_transposed":         # W[a][i] read at i * B + a
        cr, ct = cr.reshape(cr.shape[1], br).T, ct.reshape(ct.shape[1], bt).T
    if reading == "last_element_tile_only":
        for k_, c_ in ((kr, cr), (kt, ct)):
            c_[:, :ETILE * ((len(k_) - 1) // ETILE)] = 0
    tau_sign = -1 if reading == "tau_phase_sign" else 1
    shift = {"tap_off_by_one": 1, "l_min_ignored": l_min}.get(reading, 0)
    # the beams of every (pair, time) row, through the beam slots of its block
    cap = tiling(br, bt, nt, L)["cap"]
    row = np.arange(br * bt * nt)
    pair, mrow = row // nt, row % nt
    pf = (row // cap * cap) // nt
    amap, bmap = pair // bt, pair % bt
    if reading == "tx_slot_is_beam" and bt > cap:     # TX slot s holds beam s: pair pf + s reads beam s
        bmap = pair - pf
    if reading == "a0_rounded_up":                    # RX slot s holds beam ceil(pf / Bt) + s
        amap = amap + (-(-pf // bt) - pf // bt)
    ok = amap < br
    amap = np.minimum(amap, br - 1)
    h = np.zeros((nrx, ntx, br * bt * nt, 2, L), np.complex128)
    qs = TU.delays(v)
    for rx in range(nrx):
        for tx in range(ntx):
            n = min(int(v["kept"][rx, tx]), K)
            if n == 0:
                continue
            q = qs[rx, tx, :n]
            nu4 = np.rint(v["freq_shift"][rx, tx, :n].astype(np.float64) * DT * 4).astype(np.int64)
            gr = cr @ _UNIT[(kr @ np.rint(v["u_rx"][rx, tx, :n]).astype(np.int64).T) % 4]    # [Br, n]
            gt = ct @ _UNIT[(kt @ np.rint(v["u_tx"][rx, tx, :n]).astype(np.int64).T) % 4]    # [Bt, n]
            G = gr[amap] * gt[bmap] * ok[:, None]                                             # [rows, n]
            if reading == "gain_as_phase":            # arg G added to the phase: |G| lost
                mod = np.abs(G)
                G = np.where(mod > 0, G / np.where(mod > 0, mod, 1.0), 0)
            ph = _UNIT[(nu4[None, :] * mrow[:, None] - tau_sign * q[None, :]) % 4]            # [rows, n]: f_c tau = q / 4
            amp = np.stack([v["a_te"][rx, tx, :n], v["a_tm"][rx, tx, :n]], axis=1).astype(np.complex128)   # [n, 2]
            k = q - l_min + shift
            V = (k[:, None] == np.arange(L)[None, :]).astype(np.float64)                      # [n, L]
            h[rx, tx] = np.einsum("gp,pq,pl->gql", G * ph, amp, V)
    h = np.ascontiguousarray(h.reshape(nrx, ntx, br, bt, nt, 2, L).transpose(0, 1, 2, 3, 5, 4, 6))
    if reading == "pair_b_major":                     # the pair index b * Br + a instead of a * Bt + b
        h = np.ascontiguousarray(h.swapaxes(2, 3)).reshape(h.shape)
    if reading == "rows_time_pair":                   # the (pair, time) row a T + m read as m' Np + a'
        h = TU._rows_time_pair(h)
    return h


CODE_MUTANTS = ("conj_on_tx", "pair_b_major", "steering_sign", "weight_index_transposed", "tx_slot_is_beam",
                "a0_rounded_up", "last_element_tile_only", "gain_as_phase", "rows_time_pair", "tap_off_by_one",
                "l_min_ignored", "tau_phase_sign")
LIST_MUTANTS = ("urx_utx_swapped", "slot_n_read", "los_skipped", "header_eligible_kept")
MUTANTS = CODE_MUTANTS + LIST_MUTANTS


def mutant(name, v, re, te, wr, wt, l_min, L, nt):
    """the exact h a kernel with one wrong reading would give"""
    if name in CODE_MUTANTS:
        return exact_reference(v, re, te, wr, wt, l_min, L, nt, reading=name)
    w = copy(v)
    SU.LIST_MUTANTS[name](w)
    return exact_reference(w, re, te, wr, wt, l_min, L, nt)


def mirror_f32(v, re, te, wr, wt, fa, fs, fc, l_min, L, nt, t0=T0, dt=DT):
    """A float32 mirror of the kernel's stages (csrc/hrt_beam_gains.inc part 1, csrc/hrt_sparse_beam_taps.hip,
    csrc/hrt_taps_gemm.inc): the element phase factors with their phases reduced in float64 and evaluated in float32,
    the gains summed in float32 within a tile of 32 elements and in float64 across the tiles, rounded to float32, G =
    g_rx g_tx in float32, U = a e^{j phase} G as the kernel's float32 product, the sinc weights of csrc/hrt_sinc.h in
    float32, and the sum over the slots in the MFMA's order (index order onto the accumulator) in float32.  Returns
    (complex64 [nrx, ntx, Br, Bt, 2, nt, L], the largest modulus of any intermediate)."""
    nrx, ntx, K = v["tau"].shape
    f32 = np.float32
    re, te = np.asarray(re, f32).astype(np.float64), np.asarray(te, f32).astype(np.float64)
    wr, wt = np.asarray(wr, np.complex64), np.asarray(wt, np.complex64)
    br, bt = wr.shape[0], wt.shape[0]
    t = t0 + np.arange(nt) * dt
    l = l_min + np.arange(L)
    fac = fa / sparse.SPEED_OF_LIGHT
    out = np.zeros((nrx, ntx, br, bt, 2, nt, L), np.complex64)
    peak = 0.0

    def gains(W, conj, el, u):
        """[beams] float32 (re, im) gains of one slot"""
        nonlocal peak
        wre, wim = W.real.astype(f32), (-W.imag if conj else W.imag).astype(f32)
        sn, cs = SU._sincospi32(SU._half_revs(fac * (el @ u)))            # [N]
        gre, gim = np.zeros(W.shape[0]), np.zeros(W.shape[0])
        for e0 in range(0, len(el), ETILE):
            r, i = np.zeros(W.shape[0], f32), np.zeros(W.shape[0], f32)
            for e in range(e0, min(e0 + ETILE, len(el))):                # float32, in the kernel's order
                r = (r + wre[:, e] * cs[e]).astype(f32)
                r = (r - wim[:, e] * sn[e]).astype(f32)
                i = (i + wre[:, e] * sn[e]).astype(f32)
                i = (i + wim[:, e] * cs[e]).astype(f32)
                peak = max(peak, float(np.abs(r).max()), float(np.abs(i).max()))
            gre += r.astype(np.float64)
            gim += i.astype(np.float64)
        return gre.astype(f32), gim.astype(f32)

    for rx in range(nrx):
        for tx in range(ntx):
            acc_r = np.zeros(out.shape[2:], f32)
            acc_i = np.zeros(out.shape[2:], f32)
            for p in range(min(int(v["kept"][rx, tx]), K)):
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                sn, cs = SU._sincospi32(SU._half_revs(nu * t - fc * tau))                     # [nt]
                w = TU.sinc_weights_f32(fs, v["tau"][rx, tx, p], l)                           # [L]
                xr, xi = gains(wr, True, re, v["u_rx"][rx, tx, p].astype(np.float64))
                yr, yi = gains(wt, False, te, v["u_tx"][rx, tx, p].astype(np.float64))
                gr = (xr[:, None] * yr[None, :] - xi[:, None] * yi[None, :]).astype(f32)    # G (float32)
                gi = (xr[:, None] * yi[None, :] + xi[:, None] * yr[None, :]).astype(f32)
                er = (cs * gr[..., None] - sn * gi[..., None]).astype(f32)                   # e^{j phase} G: [Br, Bt, nt]
                ei = (cs * gi[..., None] + sn * gr[..., None]).astype(f32)
                peak = max(peak, float(np.hypot(er.astype(np.float64), ei.astype(np.float64)).max()))
                for pol, a in enumerate((v["a_te"][rx, tx, p], v["a_tm"][rx, tx, p])):
                    ar, ai = f32(a.real), f32(a.imag)
                    ur, ui = (ar * er - ai * ei).astype(f32), (ar * ei + ai * er).astype(f32)   # U (float32)
                    peak = max(peak, float(np.hypot(ur.astype(np.float64), ui.astype(np.float64)).max()))
                    acc_r[:, :, pol] += ur[..., None] * w                  # one MFMA k-step: acc + u v, in float32
                    acc_i[:, :, pol] += ui[..., None] * w
                peak = max(peak, float(np.hypot(acc_r.astype(np.float64), acc_i.astype(np.float64)).max()))
            out[rx, tx] = acc_r + 1j * acc_i
    return out, peak


def tracer_value_errors(tr):
    """the ValueErrors of Tracer.sparse_beam_taps that are its own (tr has nrx, ntx = 2, 3)"""
    import torch
    v = planted(2, 3, 8, 5, 0, 4)
    kw = dict(fs=FS, num_taps=4)
    el = elements(2, 2)
    w = (codebook(2, 2, 0), codebook(3, 2, 1))
    with pytest.raises(ValueError, match="uint8 buffer expected, got float32"):
        tr.sparse_beam_taps(v["buffer"].view(np.float32), *el, *w, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_beam_taps(torch.from_numpy(v["buffer"]), *el, *w, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of 3552 bytes expected for \(nrx, ntx, K\) = \(2, 3, 8\)"):
        tr.sparse_beam_taps({"buffer": v["buffer"][:-8], "power": v["power"]}, *el, *w, **kw)
    with pytest.raises(ValueError, match="element offsets must be finite"):
        tr.sparse_beam_taps(v, np.full((2, 3), np.nan, np.float32), el[1], *w, **kw)
    with pytest.raises(ValueError, match=r"rx_elements must have shape \(n, 3\)"):
        tr.sparse_beam_taps(v, np.zeros((2, 2), np.float32), el[1], *w, **kw)
    with pytest.raises(ValueError, match=r"rx_weights must have shape \(beams, 2\)"):
        tr.sparse_beam_taps(v, *el, codebook(2, 3, 0), w[1], **kw)
    with pytest.raises(ValueError, match=r"tx_weights must have shape \(beams, 2\)"):
        tr.sparse_beam_taps(v, *el, w[0], np.zeros((2, 2, 2), np.complex64), **kw)
    with pytest.raises(ValueError, match="tx_weights must be a real or complex floating-point array"):
        tr.sparse_beam_taps(v, *el, w[0], np.ones((3, 2), np.int32), **kw)
    bad = w[1].copy()
    bad[1, 1] = complex(0.0, np.inf)
    with pytest.raises(ValueError, match="beam weights must be finite"):
        tr.sparse_beam_taps(v, *el, w[0], bad, **kw)
