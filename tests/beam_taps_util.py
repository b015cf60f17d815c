"""What the tests of the beamformed taps (Tracer.beam_taps, hrt_beam_taps, hermespy_rt.compute_beam_taps) share: the
float64 sum written from the definition

    h[rx, tx, a, b, pol, m, l] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
                                       * sinc(l_min + l - f_s tau_p)
    g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)

on term lists (tests/planted.py: plant(), synthetic_terms(); tests/beam_util.py: terms_of()), a float64 array-taps sum
to contract it against, a Python mirror of the tiling rule of csrc/hrt_beam_taps.h (the form, the blocks, and the pairs
and beam slots of each block), and the cases of tests/test_gpu_beam_taps_edges.py.

Bound: |sinc| <= 1, so the bound of tests/beam_util.py carries over per (link, a, b, pol), over all (m, l):
|h - h64| <= 1e-5 ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol| (BU.bound / BU.check), and on planted workspaces
BU.UNIT_TOL ||W_rx[a]||_1 ||W_tx[b]||_1 (BU.check_unit)."""
import numpy as np

from . import beam_util as BU
from . import planted as PL


def sinc_weights(x, l):
    """[p, L]: sinc(l - x) in float64, exactly 1 / 0 where x is an integer (PL.taps_direct's rule)"""
    d = l[None, :] - x[:, None]
    return np.where(d == 0, 1.0, np.where((x == np.rint(x))[:, None], 0.0, np.sinc(d)))


def _seen(T, fs, L, l_min):
    """the terms of T with a non-zero tap in the window (a term at an integer delay outside it adds exact zeros)"""
    x = fs * T["tau"]
    whole = x == np.rint(x)
    keep = ~whole | ((x >= l_min) & (x < l_min + L))
    return {k: v[keep] for k, v in T.items()}   # (BU.terms_of's lists have fewer keys than PL.TERM_KEYS)


def beam_taps_direct(T, nrx, ntx, rxe, txe, cases, fa, fs, fc, L, l_min, t, chunk=256, conj_rx=True, conj_tx=False,
                     gain_as_phase=False):
    """[h64 [nrx, ntx, Br, Bt, 2, T, L] for (W_rx, W_tx) in cases]: the float64 sum from the definition (the weights
    widened from what the device gets: complex64).  cases' entries are (W_rx, W_tx) or (rxe, txe, W_rx, W_tx) with
    their own elements.  The controls of the sensitivity tests: conj_rx / conj_tx (the definition is True / False) and
    gain_as_phase (G replaced by exp(j arg G): the gain added to the phase instead of multiplied)."""
    t = np.asarray(t, np.float64)
    T = _seen(T, fs, L, l_min)
    full = []
    for c in cases:
        re_, te_, wr, wt = c if len(c) == 4 else (rxe, txe) + tuple(c)
        re_ = np.asarray(re_, np.float32).astype(np.float64).reshape(-1, 3)
        te_ = np.asarray(te_, np.float32).astype(np.float64).reshape(-1, 3)
        wr = np.asarray(wr).astype(np.complex64).astype(np.complex128)
        wt = np.asarray(wt).astype(np.complex64).astype(np.complex128)
        full.append((re_, te_, np.conj(wr) if conj_rx else wr, np.conj(wt) if conj_tx else wt))
    out = [np.zeros((nrx * ntx, wr.shape[0] * wt.shape[0], 2, t.size, L), np.complex128) for _, _, wr, wt in full]
    link = PL.link_of(T, ntx)
    l = l_min + np.arange(L, dtype=np.float64)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = PL._phases(T, s, np.array([fc]), t)[:, :, 0]   # [p, T]
        w = sinc_weights(fs * T["tau"][s], l)              # [p, L]
        for h, (re_, te_, wr, wt) in zip(out, full):
            g_rx = PL.cis((fa / PL.C0) * (T["urx"][s] @ re_.T)) @ wr.T   # [p, Br]
            g_tx = PL.cis((fa / PL.C0) * (T["utx"][s] @ te_.T)) @ wt.T   # [p, Bt]
            G = (g_rx[:, :, None] * g_tx[:, None, :]).reshape(-1, wr.shape[0] * wt.shape[0])
            if gain_as_phase:
                G = np.where(G == 0, 1.0, G / np.where(G == 0, 1.0, np.abs(G)))
            for lk in np.unique(link[s]):
                q = link[s] == lk
                for pol, a in enumerate(("a_te", "a_tm")):
                    h[lk, :, pol] += np.einsum("pg,pm,pl->gml", T[a][s][q][:, None] * G[q], e[q], w[q])
    return [h.reshape(nrx, ntx, wr.shape[0], wt.shape[0], 2, t.size, L) for h, (_, _, wr, wt) in zip(out, full)]


def array_taps_direct(T, nrx, ntx, rxe, txe, fa, fs, fc, L, l_min, t, chunk=256):
    """h64 [nrx, ntx, Nr, Nt, 2, T, L]: the float64 array-taps sum (hrt_compute_array_taps' definition)"""
    t = np.asarray(t, np.float64)
    T = _seen(T, fs, L, l_min)
    rxe = np.asarray(rxe, np.float32).astype(np.float64).reshape(-1, 3)
    txe = np.asarray(txe, np.float32).astype(np.float64).reshape(-1, 3)
    nr, nt = rxe.shape[0], txe.shape[0]
    h = np.zeros((nrx * ntx, nr * nt, 2, t.size, L), np.complex128)
    link = PL.link_of(T, ntx)
    l = l_min + np.arange(L, dtype=np.float64)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = PL._phases(T, s, np.array([fc]), t)[:, :, 0]
        w = sinc_weights(fs * T["tau"][s], l)
        st = (fa / PL.C0) * ((T["urx"][s] @ rxe.T)[:, :, None] + (T["utx"][s] @ txe.T)[:, None, :])
        g = PL.cis(st).reshape(-1, nr * nt)
        for lk in np.unique(link[s]):
            q = link[s] == lk
            for pol, a in enumerate(("a_te", "a_tm")):
                h[lk, :, pol] += np.einsum("pg,pm,pl->gml", T[a][s][q][:, None] * g[q], e[q], w[q])
    return h.reshape(nrx, ntx, nr, nt, 2, t.size, L)


# ------------------------------------------------------------------ the tiling rule (csrc/hrt_beam_taps.h, bt_plan)
def tiling(br, bt, nt, nl):
    """The form and the blocks of a call with Br x Bt beams, nt time samples and nl taps, restated from bt_plan
    (csrc/host/channel.c) and the head of hrt_beam_taps_partial_kernel: dict(form = 4 or 1, cap = rows, pairs and beam
    slots of a block, rblocks, cblocks, blocks = [dict(row0, row1, pf, pl, a0, na, tx = [TX beam of slot s])])."""
    rows = br * bt * nt
    rtiles, ctiles = (4 * rows + 15) // 16, (nl + 15) // 16
    form = 4 if rtiles >= 4 else 1
    cap = 64 if form == 4 else 4
    rblocks = -(-rtiles // (16 if form == 4 else 1))
    cblocks = -(-ctiles // (4 if form == 4 else 16))
    blocks = []
    for rb in range(rblocks):
        row0 = rb * cap
        assert row0 < rows
        row1 = min(row0 + cap, rows) - 1
        pf, pl = row0 // nt, row1 // nt
        a0 = pf // bt
        tx = list(range(bt)) if bt <= cap else [(pf + s) % bt for s in range(pl - pf + 1)]
        blocks.append(dict(row0=row0, row1=row1, pf=pf, pl=pl, a0=a0, na=pl // bt - a0 + 1, tx=tx))
    return dict(form=form, cap=cap, rblocks=rblocks, cblocks=cblocks, blocks=blocks)


def tiling_errors(br, bt, nt, nl):
    """what the slot rule would get wrong for this shape (an empty list: every row of every block finds the beams of
    its pair in the block's slots, and no block has more slots than its capacity)"""
    tl = tiling(br, bt, nt, nl)
    errs, seen = [], 0
    for rb, b in enumerate(tl["blocks"]):
        if b["na"] > tl["cap"] or len(b["tx"]) > tl["cap"]:
            errs.append("block %d: %d RX and %d TX slots for a capacity of %d" % (rb, b["na"], len(b["tx"]), tl["cap"]))
        for row in range(b["row0"], b["row1"] + 1):
            pair = row // nt
            a, bb = pair // bt, pair % bt
            sa, sb = a - b["a0"], bb if bt <= tl["cap"] else pair - b["pf"]
            if not (0 <= sa < b["na"]) or not (0 <= sb < len(b["tx"])) or b["tx"][sb] != bb:
                errs.append("block %d row %d: pair (%d, %d) not in its slots" % (rb, row, a, bb))
            seen += 1
    if seen != br * bt * nt:
        errs.append("%d of %d rows covered" % (seen, br * bt * nt))
    return errs


# ------------------------------------------------------------------ the edge cases (tests/test_gpu_beam_taps_edges.py)
W1 = np.array([[0.6 - 0.8j]], np.complex64)

# name: (Br, Bt, T, L, Nr, Nt, l_min, t0 / DT, f_a / carrier, what the case is there for,
#        expected (form, rblocks, cblocks, [(first pair, last pair) of each block]))
EDGE_SHAPES = {
    "f12": (3, 4, 1, 15, 2, 3, 0, 0, 1.0, "Br Bt T = 12: the <1, 4, 1> form, every TX beam a slot",
            (1, 3, 1, [(0, 3), (4, 7), (8, 11)])),
    "f12_t3": (2, 2, 3, 17, 1, 33, 0, 0, 1.0, "12 rows at T = 3: blocks of 4 rows begin inside a pair",
               (1, 3, 1, [(0, 1), (1, 2), (2, 3)])),
    "f12_bt12": (1, 12, 1, 1, 1, 2, 1, 0, 1.0, "12 rows with Bt = 12 > 4: per-pair TX slots in the small form, L = 1",
                 (1, 3, 1, [(0, 3), (4, 7), (8, 11)])),
    "f13": (13, 1, 1, 17, 33, 1, 0, 0, 1.0, "Br Bt T = 13: the <4, 4, 4> form, 13 RX slots, 33 RX elements",
            (4, 1, 1, [(0, 12)])),
    "f13_bt13": (1, 13, 1, 1, 1, 32, 1, 3, 1.0, "13 rows, Bt = 13, L = 1, 32 TX elements", (4, 1, 1, [(0, 12)])),
    "p64": (8, 8, 1, 15, 32, 33, 0, 0, 1.0, "T = 1, 64 pairs: one full block of 64 pairs", (4, 1, 1, [(0, 63)])),
    "p65": (5, 13, 1, 17, 2, 3, -3, 0, 1.0, "T = 1, 65 pairs: a second block of one pair; l_min < 0",
            (4, 2, 1, [(0, 63), (64, 64)])),
    "p130": (10, 13, 1, 65, 2, 3, 2, 0, 1.0, "T = 1, 130 pairs: two full blocks and a partial one, two column blocks",
             (4, 3, 2, [(0, 63), (64, 127), (128, 129)])),
    "t3": (5, 9, 3, 17, 3, 33, 0, 3, 1.0, "T = 3: blocks 1 and 2 begin inside a pair; t0 != 0",
           (4, 3, 1, [(0, 21), (21, 42), (42, 44)])),
    "t5": (3, 7, 5, 15, 33, 2, -3, 0, 0.75, "T = 5: block 1 begins inside a pair; l_min < 0, f_a off the carrier",
           (4, 2, 1, [(0, 12), (12, 20)])),
    "t64": (2, 2, 64, 15, 2, 2, 0, 0, 1.0, "T = 64: every block inside one pair",
            (4, 4, 1, [(0, 0), (1, 1), (2, 2), (3, 3)])),
    "t65": (2, 2, 65, 17, 2, 2, 0, 3, 1.0, "T = 65: the blocks straddle two pairs",
            (4, 5, 1, [(0, 0), (0, 1), (1, 2), (2, 3), (3, 3)])),
    "rx65": (65, 1, 1, 15, 256, 1, 0, 0, 1.0, "Bt = 1, Br = 65: RX slots only, 64 then 1; 256 RX elements",
             (4, 2, 1, [(0, 63), (64, 64)])),
    "tx63": (1, 63, 1, 15, 1, 33, 0, 0, 1.0, "Br = 1, Bt = 63 <= 64: every TX beam a slot", (4, 1, 1, [(0, 62)])),
    "tx64": (1, 64, 1, 15, 1, 33, 0, 0, 1.0, "Br = 1, Bt = 64: every TX beam a slot, all 64 used", (4, 1, 1, [(0, 63)])),
    "tx65": (1, 65, 1, 15, 1, 33, 0, 0, 1.0, "Br = 1, Bt = 65 > 64: per-pair TX slots", (4, 2, 1, [(0, 63), (64, 64)])),
    "tx256": (1, 256, 1, 15, 1, 256, 0, 0, 0.75, "Br = 1, Bt = 256 with 256 TX elements; f_a off the carrier",
              (4, 4, 1, [(0, 63), (64, 127), (128, 191), (192, 255)])),
    "bt65_wrap": (3, 65, 1, 17, 32, 65, 0, 0, 1.0, "Bt = 65 > 64: the TX beam wraps inside blocks 1 and 2",
                  (4, 4, 1, [(0, 63), (64, 127), (128, 191), (192, 194)])),
    "e256": (3, 5, 2, 65, 256, 256, -3, 3, 0.75, "256 elements on both sides, T = 2, two column blocks",
             (4, 1, 2, [(0, 14)])),
}
EDGE_NAMES = sorted(EDGE_SHAPES)


def _elements(n, lam, seed):
    from .pathsum_util import _random, _upa
    if n == 1:
        return np.zeros((1, 3))
    if n == 256:
        return _upa(16, 16, lam / 2)
    return _random(n, 4 * lam, seed)


def edge_case(name, lam):
    """dict(rxe, txe, wr, wt, nt, nl, l_min, t0, fa_scale, why, expect, controls) of an EDGE_SHAPES entry for the
    wavelength lam: probe codebooks (BU.probe_weights; a side with one beam has the single weight W1 on element 0),
    and controls (what, side, beam, element, how) for BU.change_weight at the beams and elements where the slot and
    tile arithmetic can go wrong: the last beam of either side, the beams of the first pair of the last block, and the
    last element of the larger side."""
    br, bt, nt, nl, nr, ntx_el, l_min, t0, fa_scale, why, expect = EDGE_SHAPES[name]
    c = dict(rxe=_elements(nr, lam, 11), txe=_elements(ntx_el, lam, 12), nt=nt, nl=nl, l_min=l_min, t0=t0 * PL.DT,
             fa_scale=fa_scale, why=why, expect=expect)

    def book(beams, elements, seed):
        if beams == 1:
            W = np.zeros((1, elements), np.complex64)
            W[0, 0] = W1[0, 0]
            return W
        return BU.probe_weights(beams, elements, seed)

    c["wr"], c["wt"] = book(br, nr, 0), book(bt, ntx_el, 1)
    tl = tiling(br, bt, nt, nl)
    pf = tl["blocks"][-1]["pf"]
    sel = []
    for side, W, last_block_beam in (("rx", c["wr"], pf // bt), ("tx", c["wt"], pf % bt)):
        how = "move" if W.shape[0] > 1 else "zero"
        sel.append(("last %s beam" % side, side, W.shape[0] - 1, None, how))
        if W.shape[0] > 1 and last_block_beam != W.shape[0] - 1:
            sel.append(("%s beam of the first pair of the last block" % side, side, last_block_beam, None, "zero"))
    side, W = ("rx", c["wr"]) if nr >= ntx_el else ("tx", c["wt"])
    if W.shape[1] > 1 and (W[:, -1] != 0).any():
        sel.append(("last element of the %s side" % side, side, None, W.shape[1] - 1, "zero"))
    c["controls"] = []
    for what, side, beam, element, how in sel:
        beam, element = BU.pick_weight(c["wt"] if side == "tx" else c["wr"], beam, element)
        c["controls"].append((what, side, beam, element, how))
    return c


def edge_times(c):
    return c["t0"] + PL.DT * np.arange(c["nt"])


def edge_direct(T, nrx, ntx, c, books, fa_carrier):
    """the float64 references of an edge case for the codebooks `books` on the planted grid (fs = PL.FS, fc = PL.FC)"""
    return beam_taps_direct(T, nrx, ntx, c["rxe"], c["txe"], books, c["fa_scale"] * fa_carrier, PL.FS, PL.FC, c["nl"],
                            c["l_min"], edge_times(c))


def window_records(T, c):
    """(name, term index) of the terms of T to change in the reference of case c: the scatter terms at the first and
    the last tap of the window that holds one (PL.control_records' records may lie outside a short window)"""
    k = T["n"] - c["l_min"]
    s = np.nonzero(~T["los"] & (k >= 0) & (k < c["nl"]))[0]
    assert s.size, "no planted record in the window"
    return [("first tap", int(s[np.argmin(k[s])])), ("last tap", int(s[np.argmax(k[s])]))]
