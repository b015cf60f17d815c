"""Host side of the per-point maximum-likelihood MIMO detection (Tracer.detect / Tracer.channel_detect,
hermespy_rt.compute_channel_detect), numpy only: constellations, the float64 reference in the device layout, and the
bit bookkeeping around the hard decision and the LLRs.

    ml_reference        index, metric, llr (and status) of every point in float64, device layout
    qam                 Gray-labelled QAM per TS 38.211 section 5.1 (B even; odd B: the rectangular extension)
    psk                 Gray-labelled 2^B-PSK
    modulate            bits -> symbols of a constellation
    hypothesis_symbols  the symbol index of every stream of a hypothesis q
    hard_bits           the bits of every stream of a hypothesis q
    bit_errors          the number of differing bits
    linear_llrs         the max-log LLRs behind a linear equalizer (Tracer.equalizer's W and sinr), for comparison
    kbest_reference     the K-best tree search (Tracer.kbest, hrt_kbest_spec) in float64, device layout, with the
                        pruning gaps that tell which points a float32 search may decide differently

The conventions are those of include/hermespy_rt.h (hrt_detect_spec): H [nrx, ntx, Nr, Nt, 2, T, K], Y
[nrx, ntx, Nr, 2, T, K], a constellation [M = 2^B] used as given whose index is the bit label, hypothesis q < M^Nt with
stream j sending symbol (q >> (j B)) & (M - 1), bit b of a stream (x >> (B - 1 - b)) & 1 (b = 0 the label's most
significant bit, the first bit of TS 38.211), d_q = |y - H s(q)|^2, the smallest wins, the lowest q on a tie, and
llr[j][b] = (min over bit 0 - min over bit 1) / noise: positive where bit 1 is the likelier.
"""
import numpy as np

NONFINITE = 1
NO_INDEX = 0xFFFFFFFF
MAX_BITS = 12
DEFICIENT = 2                           # hrt_kbest_spec: a null column
KB_MAX_NT, KB_MAX_BITS, KB_MAX_K = 16, 32, 64


def _bits_of(constellation):
    S = np.asarray(constellation)
    M = S.shape[0] if S.ndim == 1 else 0
    if M < 2 or M & (M - 1):
        raise ValueError("constellation must be [2^B], got shape %s" % (S.shape,))
    return S.astype(np.complex128), M.bit_length() - 1


def _axis(c):
    """the Gray-labelled amplitude of TS 38.211 along one axis from its bits c [n, ...] (c[0] first): (1 - 2 c0)
    [2^(n-1) - (1 - 2 c1) [2^(n-2) - .. [2 - (1 - 2 c_n-1)]]], odd integers in -(2^n - 1) .. 2^n - 1; 0 for n = 0"""
    n = len(c)
    if n == 0:
        return 0.0
    v = 1.0
    for k in range(n - 1, 0, -1):
        v = 2.0 ** (n - k) - (1.0 - 2.0 * c[k]) * v
    return (1.0 - 2.0 * c[0]) * v


def qam(bits, normalised=True):
    """The 2^B-QAM constellation of TS 38.211 section 5.1, complex128 [2^B]: the symbol at index x carries the bits
    b0 .. b_B-1 of x, b0 the most significant; b0, b2, .. set the real part and b1, b3, .. the imaginary part, Gray
    along each axis (B = 2, 4, 6, 8: the tables of 5.1.3 to 5.1.6).  Odd B is the rectangular extension by the same
    rule (ceil(B / 2) bits on the real axis; B = 1 is real +-1, not the diagonal BPSK of 5.1.2).  Unnormalised the
    coordinates are odd integers; normalised the mean power is 1."""
    B = int(bits)
    if not 1 <= B <= MAX_BITS:
        raise ValueError("qam: bits must be in 1 .. %d, got %r" % (MAX_BITS, bits))
    x = np.arange(1 << B)
    b = [(x >> (B - 1 - i)) & 1 for i in range(B)]
    S = _axis(b[0::2]) + 1j * _axis(b[1::2])
    S = np.asarray(S, np.complex128)
    return S / np.sqrt((np.abs(S) ** 2).mean()) if normalised else S


def psk(bits, offset=0.0):
    """Gray-labelled 2^B-PSK of unit modulus, complex128 [2^B]: the k-th point counter-clockwise, at the angle
    2 pi k / M + offset, carries the label k ^ (k >> 1)"""
    B = int(bits)
    if not 1 <= B <= MAX_BITS:
        raise ValueError("psk: bits must be in 1 .. %d, got %r" % (MAX_BITS, bits))
    k = np.arange(1 << B)
    S = np.empty(1 << B, np.complex128)
    S[k ^ (k >> 1)] = np.exp(1j * (2.0 * np.pi * k / (1 << B) + offset))
    return S


def symbol_indices(bits, B):
    """bits [..., B] (the first the most significant) -> the symbol index [...]"""
    b = np.asarray(bits).astype(np.int64)
    if b.shape[-1] != B:
        raise ValueError("bits [..., %d] expected, got %s" % (B, b.shape))
    return (b << (B - 1 - np.arange(B))).sum(-1)


def modulate(bits, constellation):
    """bits [..., B] (or flat, a multiple of B) -> the symbols [...] of `constellation` [2^B]"""
    S, B = _bits_of(constellation)
    b = np.asarray(bits)
    if b.ndim == 1:
        if b.size % B:
            raise ValueError("modulate: %d bits are no multiple of B = %d" % (b.size, B))
        b = b.reshape(-1, B)
    return S[symbol_indices(b, B)]


def hypothesis_symbols(q, nt, bits):
    """the symbol index of every stream of hypothesis q: [..., Nt], stream j is (q >> (j B)) & (2^B - 1)"""
    q = np.asarray(q).astype(np.int64)
    return (q[..., None] >> (np.arange(int(nt)) * int(bits))) & ((1 << int(bits)) - 1)


def hypothesis(symbols, bits):
    """the inverse of hypothesis_symbols: symbol indices [..., Nt] -> q [...]"""
    x = np.asarray(symbols).astype(np.int64)
    return (x << (np.arange(x.shape[-1]) * int(bits))).sum(-1)


def hard_bits(index, nt, bits):
    """the bits of a hard decision: index [...] -> uint8 [..., Nt, B], bit b of stream j (b = 0 the most significant);
    a flagged point (NO_INDEX, -1) gives zeros"""
    B = int(bits)
    q = np.asarray(index).astype(np.int64) & 0xFFFFFFFF
    q = np.where(q == NO_INDEX, 0, q)
    x = hypothesis_symbols(q, nt, B)
    return ((x[..., None] >> (B - 1 - np.arange(B))) & 1).astype(np.uint8)


def bit_errors(a, b):
    """the number of positions at which the bit arrays differ"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError("bit_errors: shapes %s and %s differ" % (a.shape, b.shape))
    return int(((a != 0) != (b != 0)).sum())


def _points(H):
    """[nrx, ntx, Nr, Nt, 2, T, K] -> [nrx, ntx, 2, T, K, Nr, Nt]"""
    return np.moveaxis(np.asarray(H), (2, 3), (-2, -1))


def distances(H, Y, constellation, chunk=512):
    """d_q of every point and hypothesis in float64: [nrx, ntx, 2, T, K, Q]"""
    S, B = _bits_of(constellation)
    H, Y = np.asarray(H, np.complex128), np.asarray(Y, np.complex128)
    if H.ndim != 7 or H.shape[4] != 2 or Y.shape != H.shape[:3] + H.shape[4:]:
        raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] and Y [nrx, ntx, Nr, 2, T, K] expected, got %s and %s"
                         % (H.shape, Y.shape))
    nt = H.shape[3]
    if nt * B > MAX_BITS:
        raise ValueError("Nt * B = %d > %d" % (nt * B, MAX_BITS))
    Q = 1 << (nt * B)
    Hm, Ym = _points(H), np.moveaxis(Y, 2, -1)                  # [.., Nr, Nt], [.., Nr]
    d = np.empty(Hm.shape[:-2] + (Q,))
    with np.errstate(all="ignore"):
        for q0 in range(0, Q, chunk):
            X = S[hypothesis_symbols(np.arange(q0, min(Q, q0 + chunk)), nt, B)]      # [c, Nt]
            r = Ym[..., None, :] - np.einsum("...ij,cj->...ci", Hm, X)
            d[..., q0:q0 + chunk] = (r.real ** 2 + r.imag ** 2).sum(-1)
    return d


def ml_reference(H, Y, constellation, noise, llr=True, table=False):
    """The detection in float64 in the device layout -> dict: index uint32, metric float64 and status uint32
    [nrx, ntx, 2, T, K], llr float64 [nrx, ntx, Nt, B, 2, T, K] (None without llr); with table=True also "distances"
    [nrx, ntx, 2, T, K, Q].  A point with a non-finite distance or LLR is flagged as the device flags it: index
    NO_INDEX, metric 0, zero LLRs."""
    S, B = _bits_of(constellation)
    n0 = float(noise)
    if not 0.0 < n0 < np.inf:
        raise ValueError("noise must be finite and > 0, got %r" % (noise,))
    d = distances(H, Y, S)
    nt = np.asarray(H).shape[3]
    Q = d.shape[-1]
    q = np.arange(Q)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(d).all(-1)
        safe = np.where(bad[..., None], 0.0, d)
        index = np.argmin(safe, -1)                             # the first of the smallest
        best = np.take_along_axis(safe, index[..., None], -1)[..., 0]
        L = None
        if llr:
            L = np.empty(d.shape[:-1] + (nt, B))
            for j in range(nt):
                for b in range(B):
                    one = ((q >> (j * B + (B - 1 - b))) & 1).astype(bool)
                    L[..., j, b] = (safe[..., ~one].min(-1) - safe[..., one].min(-1)) / n0
            bad = bad | ~np.isfinite(L).all((-2, -1))
            L = np.moveaxis(np.where(bad[..., None, None], 0.0, L), (-2, -1), (2, 3))
    out = {"index": np.where(bad, NO_INDEX, index).astype(np.uint32), "metric": np.where(bad, 0.0, best),
           "status": np.where(bad, NONFINITE, 0).astype(np.uint32), "llr": L}
    if table:
        out["distances"] = d
    return out


def kbest_reference(H, Y, constellation, noise, k, clip, sorted=True, llr=True):
    """The K-best tree search of include/hermespy_rt.h (hrt_kbest_spec) in float64 in the device layout: QR of
    [H | y] by modified Gram-Schmidt (sorted: the smallest residual column next, the lowest stream on a tie; a column
    at or below the threshold is null), the tree from the last position with PED = rho at the root, the K smallest
    (PED', key) of a level survive, the decision and the clamped max-log LLRs over the final list.  -> dict:
    index uint32, metric float64 and status uint32 [nrx, ntx, 2, T, K] (NONFINITE: index NO_INDEX, metric 0, zero
    LLRs; DEFICIENT: a null column), llr float64 [nrx, ntx, Nt, B, 2, T, K] (None without llr), and per point
        gap        the smallest PED difference between the K-th and the (K + 1)-th candidate of any level, relative to
                   sigma = (|y|_2 + |H|_F max|S| sqrt(Nt))^2 (inf where no level had more than K candidates)
        order_gap  sorted only: the smallest difference between the two smallest residual norms at a pick, relative
                   to the largest squared column norm of H (inf unsorted)
        lead       the PED difference of the two best leaves of the final list, relative to sigma (inf: one leaf)
    A float32 search may keep another list where gap is of the order of float32's rounding, another order where
    order_gap is, another index where lead is."""
    S, B = _bits_of(constellation)
    n0, cl, K = float(noise), float(clip), int(k)
    if not 0.0 < n0 < np.inf:
        raise ValueError("noise must be finite and > 0, got %r" % (noise,))
    if not 0.0 < cl < np.inf:
        raise ValueError("clip must be finite and > 0, got %r" % (clip,))
    if K < 1 or K > KB_MAX_K or K & (K - 1):
        raise ValueError("k must be 1, 2, 4, .. %d, got %r" % (KB_MAX_K, k))
    H, Y = np.asarray(H, np.complex128), np.asarray(Y, np.complex128)
    if H.ndim != 7 or H.shape[4] != 2 or Y.shape != H.shape[:3] + H.shape[4:]:
        raise ValueError("H [nrx, ntx, Nr, Nt, 2, T, K] and Y [nrx, ntx, Nr, 2, T, K] expected, got %s and %s"
                         % (H.shape, Y.shape))
    nr, nt = H.shape[2], H.shape[3]
    if nt > KB_MAX_NT or nt * B > KB_MAX_BITS:
        raise ValueError("Nt = %d, Nt * B = %d: beyond %d and %d" % (nt, nt * B, KB_MAX_NT, KB_MAX_BITS))
    M = 1 << B
    lead_shape = H.shape[:2] + H.shape[4:]
    A = np.concatenate([_points(H), np.moveaxis(Y, 2, -1)[..., None]], -1).reshape(-1, nr, nt + 1)
    P = A.shape[0]
    ar = np.arange(P)
    with np.errstate(all="ignore"):
        n2 = (A.real ** 2 + A.imag ** 2).sum(1)                 # [P, Nt + 1]
        bad = ~np.isfinite(n2.sum(-1))
        A = np.where(bad[:, None, None], 0.0, A)
        n2 = np.where(bad[:, None], 0.0, n2)
        nmax = n2[:, :nt].max(-1)
        sigma = (np.sqrt(n2[:, nt]) + np.sqrt(n2[:, :nt].sum(-1)) * np.abs(S).max() * np.sqrt(nt)) ** 2
        thr = (nr + nt) * 2.0 ** -23 * np.sqrt(nmax)
        R = np.zeros((P, nt, nt), np.complex128)                # [position, stream]
        z = np.zeros((P, nt), np.complex128)
        order = np.zeros((P, nt), np.int64)
        chosen = np.zeros((P, nt + 1), bool)
        deficient = np.zeros(P, bool)
        order_gap = np.full(P, np.inf)
        for t in range(nt):
            cn = (A[:, :, :nt].real ** 2 + A[:, :, :nt].imag ** 2).sum(1)
            if sorted:
                cn = np.where(chosen[:, :nt], np.inf, cn)
                c = np.argmin(cn, -1)                           # the first of the smallest
                if t + 1 < nt:
                    two = np.sort(cn, -1)[:, :2]
                    order_gap = np.minimum(order_gap, (two[:, 1] - two[:, 0]) / np.where(nmax > 0, nmax, 1.0))
            else:
                c = np.full(P, t)
            r = np.sqrt(cn[ar, c])
            null = ~(r > thr)
            deficient |= null
            q = np.where(null[:, None], 0.0, A[ar, :, c] / np.where(null, 1.0, r)[:, None])
            A[ar, :, c] = np.where(null[:, None], A[ar, :, c], q)
            chosen[ar, c] = True
            w = np.where(chosen, 0.0, np.einsum("pi,pij->pj", np.conj(q), A))
            A = A - q[:, :, None] * w[:, None, :]
            R[:, t, :] = w[:, :nt]
            R[ar, t, c] = np.where(null, 0.0, r)
            z[:, t] = w[:, nt]
            order[:, t] = c
        rho = (A[:, :, nt].real ** 2 + A[:, :, nt].imag ** 2).sum(1)
        bad |= ~np.isfinite(rho)
        ped, key = rho[:, None].copy(), np.zeros((P, 1), np.int64)
        gap = np.full(P, np.inf)
        x = np.arange(M)
        for i in range(nt - 1, -1, -1):
            c = order[:, i]
            b = np.repeat(z[:, i, None], ped.shape[1], 1)
            acc = None
            for t in range(i + 1, nt):
                u = order[:, t]
                term = R[ar, i, u][:, None] * S[(key >> (u * B)[:, None]) & (M - 1)]
                acc = term if acc is None else acc + term
            if acc is not None:
                b = b - acc
            e = b[:, :, None] - R[ar, i, c].real[:, None, None] * S[None, None, :]
            cp = (ped[:, :, None] + (e.real ** 2 + e.imag ** 2)).reshape(P, -1)
            ck = (key[:, :, None] | (x[None, None, :] << (c * B)[:, None, None])).reshape(P, -1)
            o1 = np.argsort(ck, -1, kind="stable")
            cp, ck = np.take_along_axis(cp, o1, -1), np.take_along_axis(ck, o1, -1)
            o2 = np.argsort(cp, -1, kind="stable")              # (NaN last; such a point is flagged)
            cp, ck = np.take_along_axis(cp, o2, -1), np.take_along_axis(ck, o2, -1)
            bad |= ~np.isfinite(cp).all(-1)
            if cp.shape[1] > K:
                gap = np.minimum(gap, (cp[:, K] - cp[:, K - 1]) / np.where(sigma > 0, sigma, 1.0))
            ped, key = cp[:, :K], ck[:, :K]
        index, best = key[:, 0], ped[:, 0]
        lead = (ped[:, 1] - ped[:, 0]) / np.where(sigma > 0, sigma, 1.0) if ped.shape[1] > 1 else np.full(P, np.inf)
        L = None
        if llr:
            L = np.empty((P, nt, B))
            for j in range(nt):
                for bb in range(B):
                    one = ((key >> (j * B + (B - 1 - bb))) & 1).astype(bool)
                    m0 = np.where(one, np.inf, ped).min(-1)
                    m1 = np.where(one, ped, np.inf).min(-1)
                    both = np.isfinite(m0) & np.isfinite(m1)
                    v = np.where(both, m0, 0.0) - np.where(both, m1, 0.0)
                    v = v / n0
                    bad |= both & ~np.isfinite(v)
                    v = np.clip(v, -cl, cl)
                    L[:, j, bb] = np.where(both, v, np.where(np.isfinite(m0), -cl, cl))
            L = np.where(bad[:, None, None], 0.0, L)
            L = np.moveaxis(L.reshape(lead_shape + (nt, B)), (-2, -1), (2, 3))
    status = np.where(bad, NONFINITE, np.where(deficient, DEFICIENT, 0))
    sh = lambda v: v.reshape(lead_shape)
    return {"index": sh(np.where(bad, NO_INDEX, index).astype(np.uint32)), "metric": sh(np.where(bad, 0.0, best)),
            "status": sh(status.astype(np.uint32)), "llr": L, "gap": sh(gap), "order_gap": sh(order_gap),
            "lead": sh(lead)}


def linear_llrs(W, sinr, Y, constellation, kind="lmmse"):
    """The max-log LLRs of the linear receiver, in float64, for comparison with the maximum-likelihood ones: W
    [nrx, ntx, Nt, Nr, 2, T, K] and sinr [nrx, ntx, Nt, 2, T, K] as Tracer.equalizer gives them, Y
    [nrx, ntx, Nr, 2, T, K] -> llr [nrx, ntx, Nt, B, 2, T, K] of the sign convention above.  Stream i of W y is
    beta_i x_i plus noise of variance beta_i^2 / sinr_i, with beta_i = sinr_i / (1 + sinr_i) under "lmmse" (its sinr is
    the unbiased one) and 1 under "zf"; so z = (W y)_i / beta_i is demapped per stream at the noise power 1 / sinr_i:
    llr = sinr_i (min over bit 0 of |z - s|^2 - min over bit 1).  Streams of sinr 0 give 0."""
    S, B = _bits_of(constellation)
    if kind not in ("lmmse", "zf"):
        raise ValueError("kind must be 'lmmse' or 'zf', got %r" % (kind,))
    W, g, Y = np.asarray(W, np.complex128), np.asarray(sinr, np.float64), np.asarray(Y, np.complex128)
    z = np.einsum("rxij...,rxj...->rxi...", W, Y)               # [nrx, ntx, Nt, 2, T, K]
    with np.errstate(all="ignore"):
        beta = g / (1.0 + g) if kind == "lmmse" else np.ones_like(g)
        z = np.where(beta > 0, z / np.where(beta > 0, beta, 1.0), 0.0)
    e = np.abs(z[..., None] - S) ** 2                           # [.., M]
    x = np.arange(S.shape[0])
    out = np.empty(z.shape[:3] + (B,) + z.shape[3:])
    for b in range(B):
        one = ((x >> (B - 1 - b)) & 1).astype(bool)
        out[:, :, :, b] = g * (e[..., ~one].min(-1) - e[..., one].min(-1))
    return out
