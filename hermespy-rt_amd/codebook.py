"""Host side of the per-subband precoder codebook selection (Tracer.codebook_select /
Tracer.channel_codebook_select, hermespy_rt.compute_codebook_select), numpy only: codebooks, the float64 reference in
the device layout, and the rank and quality reports built on the selection.

    select_reference  index, metric, table, effective (and status) of every subband of H in float64, device layout
    dft               rank-1 DFT beams [n oversampling, n, 1] of unit norm
    dual_polarised    beams on two polarisations with a co-phase, [., 2 n, layers], layers 1 or 2, unit norm
    select_rank       one selection per rank L, then the rank of the largest capacity per subband (RI)
    cqi_sinr          the post-equalizer SINR of every layer on the effective channel (CQI)

The conventions are those of include/hermespy_rt.h (hrt_compute_codebook_select): H [nrx, ntx, Nr, Nt, 2, T, K], a
codebook [C, Nt, L] used as given, a subband S consecutive frequencies of one (rx, tx, pol, m) with the remainder in
the last, E = H_k W_c, metric "power" the mean of |E|_F^2 over the subband, "capacity" the mean of
log2 det(I + E^H E / noise); the largest wins, the lowest index on a tie.  These are generic constructions, not NR's
Type I / II tables or their index mapping.
"""
import numpy as np

POWER, CAPACITY = 0, 1
NONFINITE = 1
NO_INDEX = 0xFFFFFFFF
_METRICS = {"power": POWER, "capacity": CAPACITY, POWER: POWER, CAPACITY: CAPACITY}


def _metric(metric):
    k = metric.lower() if isinstance(metric, str) else metric
    if k not in _METRICS:
        raise ValueError("metric must be one of 'power', 'capacity', got %r" % (metric,))
    return _METRICS[k]


def dft(n, oversampling=1):
    """The n * oversampling DFT beams of an n-element uniform line, complex128 [n oversampling, n, 1]: entry c is
    exp(-2 pi j i c / (n oversampling)) / sqrt(n) over the elements i (beams.dft_codebook's convention; unit norm)."""
    n, o = int(n), int(oversampling)
    if n < 1 or o < 1:
        raise ValueError("dft: n and oversampling must be >= 1")
    c, i = np.arange(n * o), np.arange(n)
    return (np.exp(-2j * np.pi * np.outer(c, i) / (n * o)) / np.sqrt(n))[:, :, None]


def dual_polarised(n, oversampling=1, layers=1):
    """Beams of an array of n elements on each of two polarisations, Nt = 2 n (the first n elements one polarisation,
    the last n the other), with v every beam of dft(n, oversampling) scaled back to unit entries:
    layers 1: [v; phi v] / sqrt(2 n) over phi in {1, j, -1, -j}, entry 4 beam + phase, [4 n oversampling, 2 n, 1];
    layers 2: [[v, v]; [phi v, -phi v]] / sqrt(4 n) over phi in {1, j}, entry 2 beam + phase, [2 n oversampling, 2 n, 2].
    Every entry has unit Frobenius norm; the two columns of a rank-2 entry are orthogonal."""
    n, layers = int(n), int(layers)
    v = dft(n, oversampling)[:, :, 0] * np.sqrt(n)                       # [beams, n], unit-modulus entries
    if layers == 1:
        phi = np.array([1, 1j, -1, -1j])
        W = np.concatenate([np.broadcast_to(v[:, None, :], (v.shape[0], 4, n)), phi[None, :, None] * v[:, None, :]], 2)
        return (W / np.sqrt(2 * n)).reshape(-1, 2 * n, 1)
    if layers == 2:
        phi = np.array([1, 1j])
        top = np.broadcast_to(v[:, None, :, None], (v.shape[0], 2, n, 2))
        low = phi[None, :, None, None] * v[:, None, :, None] * np.array([1.0, -1.0])
        return (np.concatenate([top, low], 2) / np.sqrt(4 * n)).reshape(-1, 2 * n, 2)
    raise ValueError("dual_polarised: layers must be 1 or 2, got %r" % (layers,))


def _codebook(codebook, nt):
    W = np.asarray(codebook)
    if W.ndim == 2:
        W = W[:, :, None]
    if W.ndim != 3 or W.shape[1] != nt or W.shape[0] < 1 or not 1 <= W.shape[2] <= nt:
        raise ValueError("codebook must be [C, %d, L], got %s" % (nt, W.shape))
    return W.astype(np.complex128)


def subbands(num_freqs, subband=None):
    """-> S, B and the list of (k0, n) of every subband (subband None: wideband)"""
    K = int(num_freqs)
    S = K if subband is None else int(subband)
    if not 1 <= S <= K:
        raise ValueError("subband must be in 1 .. %d, got %r" % (K, subband))
    B = (K + S - 1) // S
    return S, B, [(b * S, min(S, K - b * S)) for b in range(B)]


def select_reference(H, codebook, metric="capacity", noise=None, subband=None):
    """H complex [nrx, ntx, Nr, Nt, 2, T, K], codebook complex [C, Nt, L] -> dict of arrays in the device layout, in
    float64: index uint32 [nrx, ntx, 2, T, B], metric [nrx, ntx, 2, T, B], status uint32, table [nrx, ntx, C, 2, T, B],
    effective complex128 [nrx, ntx, Nr, L, 2, T, K].  The determinant is numpy.linalg.slogdet's.  A subband with a
    non-finite entry of H or a non-finite score is NONFINITE: index 0xFFFFFFFF, metric 0, zeros in table and
    effective."""
    H = np.asarray(H)
    if H.ndim != 7 or H.shape[4] != 2:
        raise ValueError("select_reference: H must be [nrx, ntx, Nr, Nt, 2, T, K], got %s" % (H.shape,))
    metric = _metric(metric)
    nrx, ntx, nr, nt, _, T, K = H.shape
    W = _codebook(codebook, nt)
    Cn, L = W.shape[0], W.shape[2]
    if metric == CAPACITY:
        if noise is None or not 0.0 < float(noise) < np.inf:
            raise ValueError("select_reference: noise must be finite and > 0 under 'capacity', got %r" % (noise,))
        noise = float(noise)
    S, B, bands = subbands(K, subband)
    Hm = np.moveaxis(H.astype(np.complex128), (2, 3), (-2, -1))          # [nrx, ntx, 2, T, K, Nr, Nt]
    finite = np.isfinite(Hm).all((-2, -1))                               # [nrx, ntx, 2, T, K]
    Hm = np.where(finite[..., None, None], Hm, 0.0)
    table = np.empty((nrx, ntx, Cn, 2, T, B))
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(Cn):
            E = Hm @ W[c]                                                # [.., K, Nr, L]
            if metric == POWER:
                f = (E.real ** 2 + E.imag ** 2).sum((-2, -1))
            else:
                G = np.conj(np.swapaxes(E, -1, -2)) @ E / noise + np.eye(L)
                f = np.linalg.slogdet(G)[1] / np.log(2.0)
            for b, (k0, n) in enumerate(bands):
                table[:, :, c, :, :, b] = f[..., k0:k0 + n].sum(-1) / n
    bad = np.stack([~finite[..., k0:k0 + n].all(-1) for k0, n in bands], -1)
    bad |= ~np.isfinite(table).all(2)
    table = np.where(bad[:, :, None], 0.0, table)
    index = np.argmax(table, axis=2)                                     # the first of the largest
    best = np.take_along_axis(table, index[:, :, None], 2)[:, :, 0]
    eff = np.zeros((nrx, ntx, nr, L, 2, T, K), np.complex128)
    for b, (k0, n) in enumerate(bands):
        Wb = W[index[..., b]]                                            # [nrx, ntx, 2, T, Nt, L]
        Eb = Hm[..., k0:k0 + n, :, :] @ Wb[..., None, :, :]              # [nrx, ntx, 2, T, n, Nr, L]
        Eb = np.where(bad[..., b][..., None, None, None], 0.0, Eb)
        eff[..., k0:k0 + n] = np.moveaxis(Eb, (-2, -1), (2, 3))
    return {"index": np.where(bad, NO_INDEX, index).astype(np.uint32), "metric": np.where(bad, 0.0, best),
            "status": np.where(bad, NONFINITE, 0).astype(np.uint32), "table": table, "effective": eff}


def select_rank(tracer, H, codebooks, noise, subband=None, effective=False):
    """The rank report on top of the selection: `codebooks` is one codebook per rank (a dict {L: [C, Nt, L]} or a
    sequence of codebooks of distinct L); Tracer.codebook_select(H, codebook, "capacity", noise, subband) runs once
    per rank and, per subband, the rank of the largest capacity wins (the lowest rank on a tie; a flagged selection
    counts as minus infinity).  -> dict: rank int64 [nrx, ntx, 2, T, B] (0 where every rank was flagged), index int64
    of that rank's codebook (-1 there), capacity float32, and selections {L: the dict codebook_select returned}."""
    items = sorted(codebooks.items()) if hasattr(codebooks, "items") else \
        sorted((int(np.asarray(w).shape[2]) if np.asarray(w).ndim == 3 else 1, w) for w in codebooks)
    if not items or len({L for L, _ in items}) != len(items):
        raise ValueError("select_rank: one codebook per distinct rank expected")
    torch = tracer.torch
    sel, rank, index, cap = {}, None, None, None
    for L, W in items:
        r = tracer.codebook_select(H, W, "capacity", noise, subband, False, effective)
        sel[L] = r
        mu = torch.where(r["status"] != 0, torch.full_like(r["metric"], -float("inf")), r["metric"])
        if rank is None:
            rank, index, cap = torch.full_like(r["index"], L, dtype=torch.int64), r["index"].to(torch.int64), mu
        else:
            better = mu > cap
            rank = torch.where(better, torch.full_like(rank, L), rank)
            index = torch.where(better, r["index"].to(torch.int64), index)
            cap = torch.where(better, mu, cap)
    none = torch.isinf(cap)
    return {"rank": torch.where(none, torch.zeros_like(rank), rank), "index": torch.where(none, -torch.ones_like(index), index),
            "capacity": torch.where(none, torch.zeros_like(cap), cap), "selections": sel}


def cqi_sinr(tracer, effective, noise, kind="lmmse"):
    """The post-equalizer SINR of every layer on the effective channel of a selection ([nrx, ntx, Nr, L, 2, T, K], as
    codebook_select(effective=True) returns it; needs L <= Nr): Tracer.equalizer(effective, noise, kind, weights=False)
    ["sinr"], float32 [nrx, ntx, L, 2, T, K].  A quantiser to CQI levels is the caller's."""
    return tracer.equalizer(effective, noise, kind, False)["sinr"]
