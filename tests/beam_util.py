"""What the tests of the beamformed channel (Tracer.beam_channel, hrt_beam_channel, hermespy_rt.compute_beam_channel)
share: random codebooks, the float64 beam sum written from the definition

    B[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
    g_rx[a](u) = sum_i conj(W_rx[a, i]) exp(j 2 pi f_a r_i . u / c),  g_tx[b](u) = sum_j W_tx[b, j] exp(j 2 pi f_a q_j . u / c)

on term lists (tests/planted.py: plant(), synthetic_terms() or terms_of() below), and the bound

    |B - B64| <= scale * ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol|  (+ 1e-30)    per (link, a, b, pol), over all (m, k)

which is the array tolerance 1e-5 sum_p |a_p^pol| per element pair, summed over the pairs with the triangle
inequality."""
import numpy as np

from . import planted as PL


def random_weights(beams, elements, seed):
    """complex64 [beams, elements], re and im uniform in [-1, 1]: no symmetry a wrong convention could hide behind"""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-1, 1, (beams, elements)) + 1j * rng.uniform(-1, 1, (beams, elements))).astype(np.complex64)


def terms_of(tr, los=True, scatter=True):
    """the terms a path-sum family adds for the last trace of `tr`, as a term list of tests/planted.py (the keys the
    references read: rx, tx, a_te, a_tm, tau, nu, urx, utx, los), float64 copies of the float32 values on the device:
    every unblocked scatter record (u_tx: the launch direction of its global path) and, on shard rank 0, the LoS
    entry of every link where it is not blocked (u_tx = HRT_LOS_DIR, u_rx = -u_tx; coincident: a = 1, tau = nu = 0,
    u_tx = (-1, 0, 0))"""
    cols = {k: [] for k in ("rx", "tx", "a_te", "a_tm", "tau", "nu", "urx", "utx", "los")}

    def add(rx, tx, a_te, a_tm, tau, nu, urx, utx, is_los):
        n = np.size(tau)
        cols["rx"].append(np.full(n, rx, np.int64))
        cols["tx"].append(np.full(n, tx, np.int64))
        cols["a_te"].append(np.asarray(a_te).astype(np.complex128).reshape(n))
        cols["a_tm"].append(np.asarray(a_tm).astype(np.complex128).reshape(n))
        cols["tau"].append(np.asarray(tau).astype(np.float64).reshape(n))
        cols["nu"].append(np.asarray(nu).astype(np.float64).reshape(n))
        cols["urx"].append(np.asarray(urx).astype(np.float64).reshape(n, 3))
        cols["utx"].append(np.asarray(utx).astype(np.float64).reshape(n, 3))
        cols["los"].append(np.full(n, is_los, bool))

    if los and tr.shard.rank == 0:
        L = tr.los()
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                q = L[rx, tx]
                status = int(q[0:1].view(np.uint32)[0])
                if status == 0:
                    a, tau, nu, u = 1.0, 0.0, 0.0, np.array([-1.0, 0.0, 0.0], np.float32)
                elif status == 2:
                    a, tau, nu, u = np.float32(q[1]), np.float32(q[2]), np.float32(q[6]), q[3:6].copy()
                else:
                    continue
                add(rx, tx, a, a, tau, nu, -u, u, True)
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=True).items()}
        dirs = PL.launch_dirs(tr).astype(np.float32)
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                s = (P["rx"] == rx) & (P["tx"] == tx)
                add(rx, tx, P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s], P["direction_rx"][s],
                    dirs[P["path"][s]], False)
    out = {k: np.concatenate(v) if v else np.zeros((0, 3) if k in ("urx", "utx") else 0) for k, v in cols.items()}
    for k in ("rx", "tx"):
        out[k] = out[k].astype(np.int64)
    out["los"] = out["los"].astype(bool)
    return out


def amplitude_sums(T, nrx, ntx):
    """S[rx, tx, pol] = sum_p |a_p^pol|"""
    link = PL.link_of(T, ntx)
    S = np.zeros((nrx * ntx, 2))
    for pol, a in enumerate(("a_te", "a_tm")):
        S[:, pol] = np.bincount(link, weights=np.abs(T[a]), minlength=nrx * ntx)
    return S.reshape(nrx, ntx, 2)


def beam_direct(T, nrx, ntx, rxe, txe, cases, fa, f, t, chunk=256, conj_rx=True, conj_tx=False):
    """[B64 [nrx, ntx, Br, Bt, 2, T, K] for (W_rx, W_tx) in cases]: the float64 beam sum from the definition (the
    weights widened from what the device gets: complex64), the path phases formed once for all cases.  cases' entries
    are (W_rx, W_tx) or (rxe, txe, W_rx, W_tx) with their own elements.  conj_rx / conj_tx: the controls of the
    sensitivity test (the definition is conj_rx=True, conj_tx=False)."""
    f, t = np.asarray(f, np.float64), np.asarray(t, np.float64)
    full = []
    for c in cases:
        re_, te_, wr, wt = c if len(c) == 4 else (rxe, txe) + tuple(c)
        re_ = np.asarray(re_, np.float32).astype(np.float64).reshape(-1, 3)
        te_ = np.asarray(te_, np.float32).astype(np.float64).reshape(-1, 3)
        wr = np.asarray(wr).astype(np.complex64).astype(np.complex128)
        wt = np.asarray(wt).astype(np.complex64).astype(np.complex128)
        full.append((re_, te_, np.conj(wr) if conj_rx else wr, np.conj(wt) if conj_tx else wt))
    out = [np.zeros((nrx * ntx, wr.shape[0], wt.shape[0], 2, t.size, f.size), np.complex128) for _, _, wr, wt in full]
    link = PL.link_of(T, ntx)
    for i in range(0, link.size, chunk):
        s = slice(i, i + chunk)
        e = PL._phases(T, s, f, t).reshape(-1, t.size * f.size)
        for B, (re_, te_, wr, wt) in zip(out, full):
            g_rx = PL.cis((fa / PL.C0) * (T["urx"][s] @ re_.T)) @ wr.T   # [p, Br]
            g_tx = PL.cis((fa / PL.C0) * (T["utx"][s] @ te_.T)) @ wt.T   # [p, Bt]
            G = (g_rx[:, :, None] * g_tx[:, None, :]).reshape(-1, wr.shape[0] * wt.shape[0])
            for lk in np.unique(link[s]):
                q = link[s] == lk
                for pol, a in enumerate(("a_te", "a_tm")):
                    w = T[a][s][q][:, None] * e[q]
                    B[lk, :, :, pol] += (G[q].T @ w).reshape(wr.shape[0], wt.shape[0], t.size, f.size)
    return [B.reshape(nrx, ntx, *B.shape[1:]) for B in out]


def bound(S, wr, wt, scale=1e-5):
    """[nrx, ntx, Br, Bt, 2]: scale ||W_rx[a]||_1 ||W_tx[b]||_1 S[rx, tx, pol] + 1e-30"""
    n1r = np.abs(np.asarray(wr).astype(np.complex64).astype(np.complex128)).sum(axis=1)
    n1t = np.abs(np.asarray(wt).astype(np.complex64).astype(np.complex128)).sum(axis=1)
    return scale * n1r[None, None, :, None, None] * n1t[None, None, None, :, None] * S[:, :, None, None, :] + 1e-30


def check(got, B, S, wr, wt, scale=1e-5, what=""):
    """|got - B| <= bound(S, wr, wt, scale) per (link, a, b, pol) over all (m, k); prints the largest error over bound"""
    got = np.asarray(got)
    assert got.shape == B.shape and got.dtype == np.complex64, (what, got.shape, B.shape, got.dtype)
    assert np.isfinite(got.view(np.float32)).all(), what
    err = np.abs(got.astype(np.complex128) - B).reshape(*B.shape[:5], -1).max(axis=-1)
    lim = bound(S, wr, wt, scale)
    worst = float((err / lim).max())
    print("%s: max |err| / bound = %.3g" % (what, worst))
    assert (err <= lim).all(), (what, worst, np.unravel_index(np.argmax(err / lim), err.shape))
    return worst


# ------------------------------------------------------------------ planted workspaces: the unit bound
UNIT_TOL = 0.05   # per element pair: a tenth of the weakest planted term (tests/test_gpu_beam_planted.py)


def check_unit(got, ref, wr, wt, what):
    """|got - ref| <= UNIT_TOL ||W_rx[a]||_1 ||W_tx[b]||_1 everywhere; returns the largest error over bound"""
    got = np.asarray(got).astype(np.complex128)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    tol = UNIT_TOL * np.abs(wr).sum(axis=1)[:, None] * np.abs(wt).sum(axis=1)[None, :]
    err = np.abs(got - ref)
    err = np.where(np.isnan(err), np.inf, err).reshape(*ref.shape[:4], -1).max(axis=-1)   # (rx, tx, a, b)
    worst = float((err / tol).max())
    assert (err <= tol).all(), "%s: |err| / bound = %.3g at (rx, tx, a, b) = %s" % (
        what, worst, np.unravel_index(np.argmax(err / tol), err.shape))
    return worst


def planted_codebooks(nr, nt):
    """3 RX and 5 TX random beams; beam 0 of either side has one non-zero weight (tests/test_gpu_beam_planted.py)"""
    wr, wt = random_weights(3, nr, 21), random_weights(5, nt, 22)
    wr[0], wt[0] = 0, 0
    wr[0, nr - 1], wt[0, 0] = 0.8 - 0.6j, -0.5j   # beam 0: one element
    return wr, wt


# ------------------------------------------------------------------ the S stage's edges (tests/test_gpu_beam_edges.py)
PAIRS = 32   # csrc/hrt_array_channel.h HRT_AC_PAIRS: beam pairs of one workgroup
ETILE = 32   # csrc/hrt_beam_channel.h HRT_BM_ETILE: elements whose phase factors are in LDS at a time


def probe_weights(beams, elements, seed=0):
    """complex64 [beams, elements], sparse: beam a has 1 + (a + seed) % 4 weights of modulus 1 (fewer where the side
    has fewer elements), all phases distinct (a golden-ratio sequence: no symmetry).  The first sits at element
    (37 a + 5) % elements, the others on tile borders (0, 31, 32, 63, 64, elements - 1), those of another tile than the
    first one's taken first: every beam with two weights or more spans two tiles where the side has two.  With
    ||W[a]||_1 <= 4 a weight read from the wrong beam, element or slot moves the output by many times the bound."""
    n = int(elements)
    borders = sorted({e for e in (0, ETILE - 1, ETILE, 2 * ETILE - 1, 2 * ETILE, n - 1) if 0 <= e < n})
    W = np.zeros((beams, n), np.complex64)
    k = 0
    for a in range(beams):
        first = (37 * a + 5) % n
        els = [first]
        r = a % len(borders)
        order = sorted(borders[r:] + borders[:r], key=lambda e: e // ETILE == first // ETILE)   # (stable)
        for e in order:
            if len(els) == 1 + (a + seed) % 4:
                break
            if e not in els:
                els.append(e)
        for e in els:
            k += 1
            W[a, e] = np.exp(2j * np.pi * ((0.137 + 0.6180339887498949 * k) % 1.0))
    return W


def block_slots(pb, br, bt):
    """(a0, na, [TX beam of slot s], pairs) of pair block pb, restated from the S stage of hrt_beam_partial_kernel: RX
    slot s is beam a0 + s, s < na; TX slot s is beam s where Bt <= 32, else the beam of pair p0 + s"""
    p0, npairs = pb * PAIRS, br * bt
    assert p0 < npairs
    last = min(p0 + PAIRS, npairs) - 1
    a0 = p0 // bt
    tx = list(range(bt)) if bt <= PAIRS else [(p0 + s) % bt for s in range(PAIRS)]
    return a0, last // bt - a0 + 1, tx, last - p0 + 1


def pick_weight(W, beam=None, element=None):
    """(beam, element) of the first non-zero weight of W with that beam and / or element"""
    for b, e in np.argwhere(np.asarray(W) != 0):
        if (beam is None or b == beam) and (element is None or e == element):
            return int(b), int(e)
    raise AssertionError("no weight at beam %s, element %s" % (beam, element))


def change_weight(wr, wt, side, beam, element, how):
    """the codebooks with W_side[beam, element] zeroed ("zero") or moved to the next beam ("move")"""
    wr, wt = np.array(wr), np.array(wt)
    W = wt if side == "tx" else wr
    w = W[beam, element]
    assert w != 0 and how in ("zero", "move") and (how == "zero" or W.shape[0] > 1), (side, beam, element, how)
    W[beam, element] = 0
    if how == "move":
        W[(beam + 1) % W.shape[0], element] += w
    return wr, wt


def edge_grid(K, T, t0=0.0):
    """(f0, df, f [K], t [T]) on the planted grid"""
    df = PL.FS / 4096
    return PL.FC, df, PL.FC + np.arange(K) * df, t0 + np.arange(T) * PL.DT


HEAVY = 8.0   # modulus of the weights the controls of case F change (see edge_cases)


def edge_cases(lam):
    """The cases of tests/test_gpu_beam_edges.py by name: dict(rxe, txe, wr, wt, probe, controls), elements for the
    wavelength lam.  controls: (name, side, beam, element, how) for change_weight, at the positions where an index of
    the S stage can go wrong: the last element of the last tile, element 32, the last beam of a block's RX slots, the
    first TX beam after a wrap.  probe: the codebooks have single-weight beams, so one planted record is seen too.

    F has 256 dense weights a beam on both sides.  The bound follows ||W_rx[a]||_1 ||W_tx[b]||_1, about 200 * 200,
    while one weight of modulus 1 moves a sum over N records with unrelated phases by about sqrt(N) |g_tx|, far less.
    So the weights F's controls change have modulus HEAVY: the sums stay dense, and those weights are sharp."""
    from .pathsum_util import _random, _upa
    one = np.zeros((1, 3))
    u256, u64, u33 = _upa(16, 16, lam / 2), _upa(8, 8, lam / 2), _upa(3, 11, lam / 2)
    r65, r256 = _random(65, 6 * lam, 12), _random(256, 8 * lam, 14)
    w1 = np.array([[0.6 - 0.8j]], np.complex64)
    cases = {
        "A": dict(rxe=u256, txe=one, wr=probe_weights(256, 256), wt=w1, probe=True,
                  sel=[("last element of the last tile", "rx", None, 255, "zero"), ("element 32", "rx", None, 32, "move"),
                       ("last RX slot of block 1", "rx", 63, None, "move"), ("RX slot 16 of block 0", "rx", 16, None, "zero")]),
        "B": dict(rxe=one, txe=u256, wr=np.conj(w1) * 1j, wt=probe_weights(256, 256, 1), probe=True,
                  sel=[("last element of the last tile", "tx", None, 255, "zero"), ("element 32", "tx", None, 32, "move"),
                       ("last TX slot of block 1", "tx", 63, None, "move"), ("first TX slot of block 2", "tx", 64, None, "zero")]),
        "C": dict(rxe=_random(2, 4 * lam, 11), txe=r65, wr=probe_weights(3, 2), wt=random_weights(33, 65, 31), probe=True,
                  sel=[("last element of the last tile", "tx", 32, 64, "zero"), ("element 32", "tx", 31, 32, "move"),
                       ("last RX slot of block 1", "rx", 1, None, "move"),
                       ("first TX beam after the wrap of block 1", "tx", 0, 33, "zero")]),
        "D32": dict(rxe=u64, txe=u33, wr=probe_weights(2, 64, 2), wt=probe_weights(32, 33), probe=True,
                    sel=[("last element of the last RX tile", "rx", None, 63, "zero"),
                         ("element 32 (the last TX tile)", "tx", None, 32, "move"),
                         ("the RX beam of block 1", "rx", 1, None, "move"), ("last TX slot", "tx", 31, None, "move")]),
        "D31": dict(rxe=u64, txe=u33, wr=probe_weights(3, 64, 1), wt=probe_weights(31, 33), probe=True,
                    sel=[("last element of the last RX tile", "rx", None, 63, "move"),
                         ("element 32 (the last TX tile)", "tx", None, 32, "zero"),
                         ("last RX slot of block 0", "rx", 1, None, "zero"), ("last TX slot", "tx", 30, None, "move")]),
        "E": dict(rxe=u33, txe=r65, wr=random_weights(2, 33, 41), wt=random_weights(40, 65, 42), probe=False,
                  sel=[("last element of the last RX tile", "rx", 1, 32, "zero"),
                       ("last element of the last TX tile", "tx", 39, 64, "zero"), ("element 32", "tx", 7, 32, "move"),
                       ("first TX beam after the wrap of block 1", "tx", 0, 33, "move"),
                       ("last RX slot of block 1", "rx", 1, 0, "zero")]),
        "F": dict(rxe=u256, txe=r256, wr=random_weights(4, 256, 51), wt=random_weights(8, 256, 52), probe=False,
                  sel=[("last element of the last RX tile, last RX slot", "rx", 3, 255, "zero"),
                       ("last element of the last TX tile", "tx", 7, 255, "move"), ("element 32", "rx", 1, 32, "move"),
                       ("element 32", "tx", 2, 32, "zero")]),
    }
    for name, c in cases.items():
        c["wr"], c["wt"] = np.asarray(c["wr"], np.complex64), np.asarray(c["wt"], np.complex64)
        c["controls"] = []
        for what, side, beam, element, how in c.pop("sel"):
            W = c["wt"] if side == "tx" else c["wr"]
            beam, element = pick_weight(W, beam, element)
            if name == "F":
                W[beam, element] *= HEAVY / abs(W[beam, element])
            c["controls"].append((what, side, beam, element, how))
    return cases
