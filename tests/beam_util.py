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
