"""What tests/test_sparse_beam_design.py, tests/test_sparse_beam_args.py (no device) and the GPU tests of the beam
channel of path lists (Tracer.sparse_beam_channel) share: the exact planting of tests/sparse_util.py with planted
codebooks, an independent per-path loop, a float32 mirror of the kernel's gain, G and accumulation stages, the wrong
readings a kernel could make (MUTANTS), the cases and the exact check.

The lists, the elements, f_a and the grid are exactly tests/sparse_util.py's: every phase factor is one of 1, j, -1, -j.
A planted codebook has Gaussian-integer weights with components in {0, +-1, +-2}; every non-zero weight has a non-zero
imaginary part (so the conjugate matters), and the values come from a hash of (side, beam, element): no symmetry
between beams, elements or sides.  Every gain, every G = g_rx g_tx and every output is then a Gaussian integer, exact in
float32 in any summation order while its modulus stays below 2^24.  The governing quantity is

    n max|a| ||W_rx[a]||_1 ||W_tx[b]||_1,      max|a| = |2 + 2j|

so the cases with K = 1 024 use sparse or small codebooks and the cases with 256 elements a side use a small K
(tests/test_sparse_beam_design.py proves the bound and the mirror's exactness for every case below)."""
import cmath

import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import covariance_util as CU
from . import planted as PL
from . import sparse_util as U

F_A, F0, DF, T0, DT = U.F_A, U.F0, U.DF, U.T0, U.DT
BATCH, PAIRS, ETILE = 32, 32, 32   # HRT_AC_BATCH, HRT_AC_PAIRS (csrc/hrt_array_channel.h), HRT_BM_ETILE
LIMIT = float(1 << 24)
A_MAX = abs(2 + 2j)

planted, one_hot, copy, grid, elements, check_exact = U.planted, U.one_hot, U.copy, U.grid, U.elements, U.check_exact


def codebook(beams, n, side, fill=None, salt=0):
    """complex64 [beams, n]: a planted codebook of side 0 (RX) or 1 (TX).  fill: non-zero weights per beam (None: all n),
    at hashed positions; re in {0, +-1, +-2}, im in {+-1, +-2} of every non-zero weight"""
    b, e = np.meshgrid(np.arange(beams), np.arange(n), indexing="ij")
    key = 0xC0 + 2 * salt + side
    re = np.array([0.0, 1.0, -1.0, 2.0, -2.0])[(PL.mix(b, e, key) >> np.uint64(11)) % np.uint64(5)]
    im = np.array([1.0, -1.0, 2.0, -2.0])[(PL.mix(b, e, key + 0x100) >> np.uint64(17)) % np.uint64(4)]
    W = re + 1j * im
    if fill is not None and fill < n:
        rank = np.argsort(np.argsort(PL.mix(b, e, key + 0x200), axis=1, kind="stable"), axis=1, kind="stable")
        W = np.where(rank < fill, W, 0)
    return W.astype(np.complex64)


def one_hot_codebook(beams, n, beam, element, value):
    W = np.zeros((beams, n), np.complex64)
    W[beam, element] = value
    return W


# ------------------------------------------------------------------ the cases
def case(nrx=1, ntx=1, K=33, kept=None, nr=2, nt=3, br=2, bt=3, nk=17, nt_=2, fill_r=None, fill_t=None, salt=0):
    """the parameters of a planted case: a dict; kept defaults to K on every link"""
    return dict(nrx=nrx, ntx=ntx, K=K, kept=K if kept is None else kept, nr=nr, nt=nt, br=br, bt=bt, nk=nk, nt_=nt_,
                fill_r=fill_r, fill_t=fill_t, salt=salt)


CASES = {}
for _k in (1, 31, 32, 33, 1024):                         # the batch edge and the largest list
    CASES["K%d" % _k] = case(K=_k, salt=_k)
for _kept in (0, 1, 32):                                 # kept below the list length
    CASES["kept%d" % _kept] = case(K=33, kept=_kept, salt=3)
CASES["links5"] = case(ntx=5, K=33, kept=[[0, 1, 33, 32, 7]], nr=3, nt=5, br=3, bt=11, nk=17, nt_=3, salt=9)
for _br, _bt in ((1, 1), (1, 31), (4, 8), (3, 11)):      # Br Bt = 1, 31, 32, 33
    CASES["pairs%dx%d" % (_br, _bt)] = case(br=_br, bt=_bt, nk=17, nt_=1, salt=_br + _bt)
for _bt in (31, 32, 33, 40, 256):                        # the TX slots: every beam fits / the beam of pair p0 + s
    CASES["bt%d" % _bt] = case(K=7, br=1, bt=_bt, nr=3, nt=4, nk=5, nt_=1, salt=_bt)
CASES["br256"] = case(K=7, br=256, bt=1, nr=4, nt=3, nk=5, nt_=1, salt=5)
CASES["bt40_br3"] = case(K=33, br=3, bt=40, nr=3, nt=4, nk=257, nt_=1, salt=6)    # four pair blocks x two column blocks
CASES["K1024_sparse"] = case(K=1024, nr=33, nt=64, br=2, bt=3, nk=5, nt_=1, fill_r=3, fill_t=4, salt=7)
for _n in (1, 31, 32, 33, 64, 256):                      # element tiles, on either side and on both
    _kk = 5 if _n == 256 else 33
    CASES["rx%d" % _n] = case(K=_kk, nr=_n, nt=3, nk=5, nt_=1, salt=_n)
    CASES["tx%d" % _n] = case(K=_kk, nr=2, nt=_n, nk=5, nt_=1, salt=_n + 1)
    CASES["both%d" % _n] = case(K=_kk, nr=_n, nt=_n, nk=5, nt_=1, salt=_n + 2)
for _nt in (1, 3):                                       # inner length and column block edges
    for _nk in (1, 15, 16, 17, 256, 257):
        CASES["grid%dx%d" % (_nk, _nt)] = case(K=5, nk=_nk, nt_=_nt, salt=_nk + _nt)
# the cases the wrong readings are tried on: every reading differs from the truth on two of them at least
MUTANT_CASES = ("links5", "pairs3x11", "bt40_br3", "bt33", "rx33", "tx64", "both33", "K33", "kept32")


def build(c):
    """(v, re, te, wr, wt) of a case"""
    v = planted(c["nrx"], c["ntx"], c["K"], c["kept"], c["salt"])
    re, te = elements(c["nr"], c["nt"])
    return (v, re, te, codebook(c["br"], c["nr"], 0, c["fill_r"], c["salt"]),
            codebook(c["bt"], c["nt"], 1, c["fill_t"], c["salt"]))


def governing(v, wr, wt):
    """max over links and beam pairs of n max|a| ||W_rx[a]||_1 ||W_tx[b]||_1"""
    K = v["tau"].shape[2]
    n = int(np.minimum(v["kept"], np.uint64(K)).max())
    return n * A_MAX * float(np.abs(wr).sum(axis=1).max()) * float(np.abs(wt).sum(axis=1).max())


# ------------------------------------------------------------------ references
def loop_reference(v, re, te, wr, wt, fa, f, t):
    """B of include/hermespy_rt.h by a direct loop over links, slots, beams, elements, polarisations and grid points
    with cmath: shares nothing with sparse.beam_reference but the definition"""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float64), np.asarray(te, np.float64)
    B = np.zeros((nrx, ntx, len(wr), len(wt), 2, len(t), len(f)), np.complex128)
    for rx in range(nrx):
        for tx in range(ntx):
            for p in range(min(int(v["kept"][rx, tx]), K)):
                amp = (complex(v["a_te"][rx, tx, p]), complex(v["a_tm"][rx, tx, p]))
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                urx, utx = v["u_rx"][rx, tx, p].astype(np.float64), v["u_tx"][rx, tx, p].astype(np.float64)
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
                                for k in range(len(f)):
                                    B[rx, tx, a, b, pol, m, k] += amp[pol] * g_rx * g_tx * cmath.exp(
                                        2j * cmath.pi * (nu * t[m] - f[k] * tau))
    return B


_UNIT = np.array([1, 1j, -1, -1j])


def exact_reference(v, re, te, wr, wt, nk, nt, reading=None):
    """the Gaussian-integer B of a planted list and planted codebooks on the exact grid, from the phases counted in
    quarter revolutions with integer arithmetic: complex128 [nrx, ntx, Br, Bt, 2, nt, nk], every value exact (sums of
    integers below 2^53).  reading: one of the wrong readings of the codebooks, the elements or the beam slots below."""
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
    pair = np.arange(br * bt)
    amap, bmap = pair // bt, pair % bt
    if reading == "tx_slot_is_beam" and bt > PAIRS:   # TX slot s holds beam s: pair p0 + s reads beam s
        bmap = pair % PAIRS
    if reading == "a0_rounded_up":                    # RX slot s holds beam ceil(p0 / Bt) + s
        p0 = pair // PAIRS * PAIRS
        amap = amap + (-(-p0 // bt) - p0 // bt)
    ok = amap < br
    amap = np.minimum(amap, br - 1)
    B = np.zeros((nrx, ntx, br * bt, 2, nt, nk), np.complex128)
    kk, mm = np.arange(nk), np.arange(nt)
    for rx in range(nrx):
        for tx in range(ntx):
            n = min(int(v["kept"][rx, tx]), K)
            if n == 0:
                continue
            ntau = np.rint(v["tau"][rx, tx, :n].astype(np.float64) / U.TAU_STEP).astype(np.int64)
            nu4 = np.rint(v["freq_shift"][rx, tx, :n].astype(np.float64) * DT * 4).astype(np.int64)
            gr = cr @ _UNIT[(kr @ np.rint(v["u_rx"][rx, tx, :n]).astype(np.int64).T) % 4]    # [Br, n]
            gt = ct @ _UNIT[(kt @ np.rint(v["u_tx"][rx, tx, :n]).astype(np.int64).T) % 4]    # [Bt, n]
            G = gr[amap] * gt[bmap] * ok[:, None]                                             # [pairs, n]
            ph = _UNIT[(nu4[:, None, None] * mm[None, :, None] - ntau[:, None, None] * kk[None, None, :]) % 4]
            amp = np.stack([v["a_te"][rx, tx, :n], v["a_tm"][rx, tx, :n]], axis=1).astype(np.complex128)   # [n, 2]
            B[rx, tx] = np.einsum("gp,pq,pmk->gqmk", G, amp, ph)
    B = B.reshape(nrx, ntx, br, bt, 2, nt, nk)
    if reading == "pair_b_major":                     # the pair index b * Br + a instead of a * Bt + b
        B = np.ascontiguousarray(B.swapaxes(2, 3)).reshape(B.shape)
    return B


CODE_MUTANTS = ("conj_on_tx", "pair_b_major", "steering_sign", "weight_index_transposed", "tx_slot_is_beam",
                "a0_rounded_up", "last_element_tile_only")
LIST_MUTANTS = ("urx_utx_swapped", "slot_n_read", "los_skipped", "header_eligible_kept")
MUTANTS = CODE_MUTANTS + LIST_MUTANTS


def mutant(name, v, re, te, wr, wt, nk, nt):
    """the exact B a kernel with one wrong reading would give"""
    if name in CODE_MUTANTS:
        return exact_reference(v, re, te, wr, wt, nk, nt, reading=name)
    w = copy(v)
    U.LIST_MUTANTS[name](w)
    return exact_reference(w, re, te, wr, wt, nk, nt)


def mirror_f32(v, re, te, wr, wt, fa, nk, nt):
    """A float32 mirror of the kernel's stages (csrc/hrt_beam_gains.inc part 1, csrc/hrt_sparse_beam.hip,
    csrc/hrt_pair_gemm.inc): the element phase factors with their phases reduced in float64 and evaluated in float32,
    the gains summed in float32 within a tile of 32 elements and in float64 across the tiles, rounded to float32, G =
    g_rx g_tx in float32, U and V as tests/sparse_util.py mirrors them, and the sum over the slots in index order in
    float32.  Returns (complex64 [nrx, ntx, Br, Bt, 2, nt, nk], the largest modulus of any intermediate)."""
    nrx, ntx, K = v["tau"].shape
    f32 = np.float32
    re, te = np.asarray(re, f32).astype(np.float64), np.asarray(te, f32).astype(np.float64)
    wr, wt = np.asarray(wr, np.complex64), np.asarray(wt, np.complex64)
    br, bt = wr.shape[0], wt.shape[0]
    k1, k2 = np.arange(nk) // 16, np.arange(nk) % 16
    t = T0 + np.arange(nt) * DT
    fac = fa / sparse.SPEED_OF_LIGHT
    out = np.zeros((nrx, ntx, br, bt, 2, nt, nk), np.complex64)
    peak = 0.0

    def gains(W, conj, el, u):
        """[beams] float32 (re, im) gains of one slot, and the largest tile sum"""
        nonlocal peak
        wre, wim = W.real.astype(f32), (-W.imag if conj else W.imag).astype(f32)
        sn, cs = U._sincospi32(U._half_revs(fac * (el @ u)))            # [N]
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
                us, uc = U._sincospi32(U._half_revs(nu * t[:, None] - (F0 + (k1 * 16) * DF)[None, :] * tau))   # [nt, nk]
                vs, vc = U._sincospi32(U._half_revs(-(k2 * DF) * tau))                                         # [nk]
                xr, xi = gains(wr, True, re, v["u_rx"][rx, tx, p].astype(np.float64))
                yr, yi = gains(wt, False, te, v["u_tx"][rx, tx, p].astype(np.float64))
                gr = (xr[:, None] * yr[None, :] - xi[:, None] * yi[None, :]).astype(f32)    # G (float32)
                gi = (xr[:, None] * yi[None, :] + xi[:, None] * yr[None, :]).astype(f32)
                peak = max(peak, float(np.hypot(gr.astype(np.float64), gi.astype(np.float64)).max()))
                for pol, a in enumerate((v["a_te"][rx, tx, p], v["a_tm"][rx, tx, p])):
                    ar, ai = f32(a.real), f32(a.imag)
                    ur, ui = ar * uc - ai * us, ar * us + ai * uc          # U (float32)
                    b_r, b_i = ur * vc - ui * vs, ur * vs + ui * vc        # B = U V (float32)
                    acc_r[:, :, pol] += gr[:, :, None, None] * b_r - gi[:, :, None, None] * b_i
                    acc_i[:, :, pol] += gi[:, :, None, None] * b_r + gr[:, :, None, None] * b_i
                peak = max(peak, float(np.hypot(acc_r.astype(np.float64), acc_i.astype(np.float64)).max()))
            out[rx, tx] = acc_r + 1j * acc_i
    return out, peak


def tracer_value_errors(tr):
    """the ValueErrors of Tracer.sparse_beam_channel that are its own (tr has nrx, ntx = 2, 3)"""
    import torch
    v = planted(2, 3, 8, 5)
    kw = dict(f0=F0, df=DF, num_freqs=4)
    el = elements(2, 2)
    w = (codebook(2, 2, 0), codebook(3, 2, 1))
    with pytest.raises(ValueError, match="uint8 buffer expected, got float32"):
        tr.sparse_beam_channel(v["buffer"].view(np.float32), *el, *w, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_beam_channel(torch.from_numpy(v["buffer"]), *el, *w, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of 3552 bytes expected for \(nrx, ntx, K\) = \(2, 3, 8\)"):
        tr.sparse_beam_channel({"buffer": v["buffer"][:-8], "power": v["power"]}, *el, *w, **kw)
    with pytest.raises(ValueError, match="element offsets must be finite"):
        tr.sparse_beam_channel(v, np.full((2, 3), np.nan, np.float32), el[1], *w, **kw)
    with pytest.raises(ValueError, match=r"rx_elements must have shape \(n, 3\)"):
        tr.sparse_beam_channel(v, np.zeros((2, 2), np.float32), el[1], *w, **kw)
    with pytest.raises(ValueError, match=r"rx_weights must have shape \(beams, 2\)"):
        tr.sparse_beam_channel(v, *el, codebook(2, 3, 0), w[1], **kw)
    with pytest.raises(ValueError, match=r"tx_weights must have shape \(beams, 2\)"):
        tr.sparse_beam_channel(v, *el, w[0], np.zeros((2, 2, 2), np.complex64), **kw)
    with pytest.raises(ValueError, match="tx_weights must be a real or complex floating-point array"):
        tr.sparse_beam_channel(v, *el, w[0], np.ones((3, 2), np.int32), **kw)
    bad = w[1].copy()
    bad[1, 1] = complex(0.0, np.inf)
    with pytest.raises(ValueError, match="beam weights must be finite"):
        tr.sparse_beam_channel(v, *el, w[0], bad, **kw)
