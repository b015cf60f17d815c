"""Host side of the per-point linear MIMO precoders (Tracer.precoder / Tracer.channel_precoder,
hermespy_rt.compute_channel_precoder), numpy only: the float64 reference in the device layout and what a link-level
simulator reads from a precoder.

    precoder_reference      P, sinr, status of every point of H [nrx, ntx, Nr, Nt, 2, T, K] in float64, device layout
    sinr_of                 the SINR of any given P through any H (stale CSI: P of one H, scored through another)
    default_regularization  Nr N0 / Ptot, the RZF regularization that maximises the SINR of i.i.d. channels
    sum_rate                sum log2(1 + sinr) over the streams (equalize.rate)

The conventions are those of include/hermespy_rt.h (hrt_compute_channel_precoder): y = H P s + n, E[s s^H] = I,
E[n n^H] = noise I; row i of H is the channel to stream (user port) i, Nt the transmit elements.
P0 = H^H ("mrt"), H^H (H H^H)^-1 ("zf", Nr <= Nt), H^H (H H^H + alpha I)^-1 ("rzf", alpha the regularization);
"total": P = sqrt(Ptot / |P0|_F^2) P0; "stream": column i of P is sqrt(Ptot / Nr) P0[:, i] / |P0[:, i]|;
P is [.., Nt, Nr, ..]; with E = H P, sinr_i = |E_ii|^2 / (sum_{j != i} |E_ij|^2 + noise).  The precoder is not additive
over batches or shards: sum H first.  The multi-user downlink matrix of several single links is
equalize.stack_users(H, "rx"): the users stacked along Nr.
"""
import numpy as np

from . import equalize

MRT, ZF, RZF = 0, 1, 2
TOTAL, STREAM = 0, 1
SINGULAR, NONFINITE = 1, 2
_KINDS = {"mrt": MRT, "zf": ZF, "rzf": RZF, MRT: MRT, ZF: ZF, RZF: RZF}
_NORMS = {"total": TOTAL, "stream": STREAM, TOTAL: TOTAL, STREAM: STREAM}


def _name(value, names, what):
    k = value.lower() if isinstance(value, str) else value
    if k not in names:
        raise ValueError("%s must be one of %s, got %r"
                         % (what, ", ".join(repr(n) for n in names if isinstance(n, str)), value))
    return names[k]


def _positive(v, what):
    v = float(v)
    if not (0.0 < v < np.inf):
        raise ValueError("%s must be finite and > 0, got %r" % (what, v))
    return v


def default_regularization(nr, noise, power=1.0):
    """Nr N0 / Ptot: the regularization of Tracer.precoder(kind="rzf", regularization=None)"""
    return int(nr) * _positive(noise, "noise") / _positive(power, "power")


def _check(H, what):
    H = np.asarray(H)
    if H.ndim != 7 or H.shape[4] != 2:
        raise ValueError("%s: H must be [nrx, ntx, Nr, Nt, 2, T, K], got %s" % (what, H.shape))
    return H


def sinr_of(H, P, noise):
    """H complex [nrx, ntx, Nr, Nt, 2, T, K], P complex [nrx, ntx, Nt, Nr, 2, T, K] (any P: of this H, of an earlier one,
    of another kind) -> float64 [nrx, ntx, Nr, 2, T, K]: with E = H P per point,
    sinr_i = |E_ii|^2 / (sum_{j != i} |E_ij|^2 + noise)."""
    H = _check(H, "sinr_of").astype(np.complex128)
    P = np.asarray(P).astype(np.complex128)
    if P.shape != H.shape[:2] + (H.shape[3], H.shape[2]) + H.shape[4:]:
        raise ValueError("sinr_of: P must be [nrx, ntx, Nt, Nr, 2, T, K] of H's sizes, got %s" % (P.shape,))
    noise = _positive(noise, "noise")
    p = np.abs(np.einsum("abitpmk,abtjpmk->abijpmk", H, P)) ** 2
    sig = np.einsum("abiipmk->abipmk", p)
    off = 1.0 - np.eye(H.shape[2])
    return sig / (np.einsum("abijpmk,ij->abipmk", p, off) + noise)


def sum_rate(sinr, axis=2):
    """sum log2(1 + sinr) along `axis` (default: the streams of [nrx, ntx, Nr, 2, T, K]), bit/s/Hz per point"""
    return equalize.rate(sinr, axis)


def precoder_reference(H, noise, kind="rzf", power=1.0, regularization=None, normalize="total"):
    """H complex [nrx, ntx, Nr, Nt, 2, T, K] -> dict of arrays in the device layout: P complex128 [nrx, ntx, Nt, Nr, 2,
    T, K], sinr float64 [nrx, ntx, Nr, 2, T, K], status uint32 [nrx, ntx, 2, T, K], and cond [nrx, ntx, 2, T, K], the
    condition number of the factored matrix [H^H; sqrt(alpha) I] (1 for "mrt", which factors nothing).  "zf" and "rzf":
    Householder QR of that matrix in float64 per point (numpy.linalg.qr), P0 = Q1 R^-H, with the device's rules: a
    point is SINGULAR when a diagonal entry of R is at or below 2 (Nr + Nt) 2^-24 times the largest column norm, or
    when a column of P0 ("stream") or all of P0 ("total") is zero; NONFINITE when an entry is not finite; both give
    zeros.  regularization None: default_regularization(Nr, noise, power)."""
    H = _check(H, "precoder_reference")
    kind, norm = _name(kind, _KINDS, "kind"), _name(normalize, _NORMS, "normalize")
    noise, power = _positive(noise, "noise"), _positive(power, "power")
    nr, nt = H.shape[2], H.shape[3]
    if kind == ZF and nr > nt:
        raise ValueError("precoder_reference: zero-forcing needs Nr <= Nt")
    alpha = 0.0
    if kind == RZF:
        alpha = default_regularization(nr, noise, power) if regularization is None else \
            _positive(regularization, "regularization")
    Hm = np.moveaxis(H.astype(np.complex128), (2, 3), (-2, -1))          # [nrx, ntx, 2, T, K, Nr, Nt]
    bad = ~np.isfinite(Hm).all((-2, -1))
    Hm = np.where(bad[..., None, None], 0.0, Hm)
    A = np.conj(np.swapaxes(Hm, -1, -2))                                 # H^H: [.., Nt, Nr]
    sing = np.zeros(bad.shape, bool)
    cond = np.ones(bad.shape)
    if kind == MRT:
        P0 = A
    else:
        if kind == RZF:
            A = np.concatenate([A, np.broadcast_to(np.sqrt(alpha) * np.eye(nr), A.shape[:-2] + (nr, nr))], axis=-2)
        q, r = np.linalg.qr(A)
        cmax = np.sqrt((np.abs(A) ** 2).sum(-2)).max(-1)
        diag = np.abs(np.diagonal(r, axis1=-2, axis2=-1))
        sing = (diag <= 2.0 * (nr + nt) * 2.0 ** -24 * cmax[..., None]).any(-1)
        r = np.where((bad | sing)[..., None, None], np.eye(nr), r)
        rinv = np.linalg.solve(r, np.broadcast_to(np.eye(nr, dtype=np.complex128), r.shape))
        P0 = q[..., :nt, :] @ np.conj(np.swapaxes(rinv, -1, -2))         # Q1 R^-H: [.., Nt, Nr]
        s = np.linalg.svd(A, compute_uv=False)
        with np.errstate(divide="ignore", invalid="ignore"):
            cond = s[..., 0] / s[..., -1]
    c = (np.abs(P0) ** 2).sum(-2)                                        # [.., Nr]: squared column norms
    with np.errstate(divide="ignore", invalid="ignore"):
        if norm == STREAM:
            zero = (c == 0).any(-1)
            P = P0 * np.sqrt((power / nr) / c)[..., None, :]
        else:
            zero = c.sum(-1) == 0
            P = P0 * np.sqrt(power / c.sum(-1))[..., None, None]
    flagged = bad | sing | zero
    P = np.where(flagged[..., None, None], 0.0, P)
    p = np.abs(Hm @ P) ** 2                                              # |E|^2: [.., Nr, Nr]
    sig = np.diagonal(p, axis1=-2, axis2=-1)
    itf = (p * (1.0 - np.eye(nr))).sum(-1)
    sinr = np.where(flagged[..., None], 0.0, sig / (itf + noise))
    status = np.where(bad, NONFINITE, np.where(sing | zero, SINGULAR, 0)).astype(np.uint32)
    return {"P": np.moveaxis(P, (-2, -1), (2, 3)), "sinr": np.moveaxis(sinr, -1, 2), "status": status, "cond": cond}
