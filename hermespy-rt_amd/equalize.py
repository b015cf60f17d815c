"""Host side of the per-point linear MIMO equalizers (Tracer.equalizer / Tracer.channel_equalizer,
hermespy_rt.compute_channel_equalizer), numpy only: the float64 reference in the device layout and what a link-level
simulator reads from the post-equalisation SINR.

    equalizer_reference  W, sinr, status of every point of H [nrx, ntx, Nr, Nt, 2, T, K] in float64, device layout
    sinr_from_svd        the same SINR from the SVD of H (Tracer.svd / mimo.svd_reference): a cross-check of the two
    effective_sinr       EESM: -beta ln(mean exp(-sinr / beta)) along an axis
    rate                 sum log2(1 + sinr) along an axis                                   (bit/s/Hz)
    stack_users          several links as one matrix per point, for the multi-user detector

The conventions are those of include/hermespy_rt.h (hrt_compute_channel_equalizer): y = H x + n, E[x x^H] = I,
E[n n^H] = noise I; lambda = noise for "lmmse" and 0 for "zf"; G = (H^H H + lambda I)^-1, W = G H^H [.., Nt, Nr, ..],
sinr_i = 1 / (noise G_ii) - [lmmse].  The equalizer is not additive over batches or shards: sum H first.
"""
import numpy as np

ZF, LMMSE = 0, 1
SINGULAR, NONFINITE = 1, 2
_KINDS = {"zf": ZF, "lmmse": LMMSE, ZF: ZF, LMMSE: LMMSE}


def _kind(kind):
    k = kind.lower() if isinstance(kind, str) else kind
    if k not in _KINDS:
        raise ValueError("kind must be 'zf' or 'lmmse', got %r" % (kind,))
    return _KINDS[k]


def _noise(noise):
    noise = float(noise)
    if not (0.0 < noise < np.inf):
        raise ValueError("noise must be finite and > 0, got %r" % (noise,))
    return noise


def equalizer_reference(H, noise, kind="lmmse"):
    """H complex [nrx, ntx, Nr, Nt, 2, T, K] -> dict of arrays in the device layout: W complex128 [nrx, ntx, Nt, Nr, 2,
    T, K], sinr float64 [nrx, ntx, Nt, 2, T, K], status uint32 [nrx, ntx, 2, T, K], and cond [nrx, ntx, 2, T, K], the
    condition number of the factored matrix [H; sqrt(lambda) I].  Householder QR of that matrix in float64 per point
    (numpy.linalg.qr), with the device's rules: a point is SINGULAR when a diagonal entry of R is at or below
    2 (Nr + Nt) 2^-24 times the largest column norm, NONFINITE when an entry is not finite; both give zeros."""
    H = np.asarray(H)
    if H.ndim != 7 or H.shape[4] != 2:
        raise ValueError("equalizer_reference: H must be [nrx, ntx, Nr, Nt, 2, T, K], got %s" % (H.shape,))
    kind, noise = _kind(kind), _noise(noise)
    nr, nt = H.shape[2], H.shape[3]
    if kind == ZF and nr < nt:
        raise ValueError("equalizer_reference: zero-forcing needs Nr >= Nt")
    lam = noise if kind == LMMSE else 0.0
    A = np.moveaxis(H.astype(np.complex128), (2, 3), (-2, -1))           # [nrx, ntx, 2, T, K, Nr, Nt]
    bad = ~np.isfinite(A).all((-2, -1))
    A = np.where(bad[..., None, None], 0.0, A)
    if kind == LMMSE:
        A = np.concatenate([A, np.broadcast_to(np.sqrt(lam) * np.eye(nt), A.shape[:-2] + (nt, nt))], axis=-2)
    q, r = np.linalg.qr(A)
    cmax = np.sqrt((np.abs(A) ** 2).sum(-2)).max(-1)
    diag = np.abs(np.diagonal(r, axis1=-2, axis2=-1))
    sing = (diag <= 2.0 * (nr + nt) * 2.0 ** -24 * cmax[..., None]).any(-1)
    zero = bad | sing
    r = np.where(zero[..., None, None], np.eye(nt), r)
    rinv = np.linalg.solve(r, np.broadcast_to(np.eye(nt, dtype=np.complex128), r.shape))
    W = rinv @ np.conj(np.swapaxes(q[..., :nr, :], -1, -2))              # [.., Nt, Nr]
    gii = (np.abs(rinv) ** 2).sum(-1)                                    # [.., Nt]
    sinr = 1.0 / (noise * gii) - (1.0 if kind == LMMSE else 0.0)
    W = np.where(zero[..., None, None], 0.0, W)
    sinr = np.where(zero[..., None], 0.0, sinr)
    s = np.linalg.svd(A, compute_uv=False)
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = s[..., 0] / s[..., -1]
    status = np.where(bad, NONFINITE, np.where(sing, SINGULAR, 0)).astype(np.uint32)
    return {"W": np.moveaxis(W, (-2, -1), (2, 3)), "sinr": np.moveaxis(sinr, -1, 2), "status": status, "cond": cond}


def sinr_from_svd(sigma, v, noise, kind="lmmse"):
    """The SINR of equalizer_reference from the SVD H = u diag(sigma) v^H: sigma [nrx, ntx, n, 2, T, K], v [nrx, ntx, Nt,
    n, 2, T, K] (Tracer.svd, mimo.svd_reference) -> float64 [nrx, ntx, Nt, 2, T, K].
    G_ii = sum_j |v_ij|^2 / (sigma_j^2 + lambda) + (1 - sum_j |v_ij|^2) / lambda, the last term only where n < Nt (the
    null space of a wide H, LMMSE only)."""
    kind, noise = _kind(kind), _noise(noise)
    s = np.asarray(sigma, np.float64)
    v = np.asarray(v).astype(np.complex128)
    nt, n = v.shape[2], v.shape[3]
    if kind == ZF and n < nt:
        raise ValueError("sinr_from_svd: zero-forcing needs Nr >= Nt")
    lam = noise if kind == LMMSE else 0.0
    p = np.abs(v) ** 2                                                   # [nrx, ntx, Nt, n, 2, T, K]
    with np.errstate(divide="ignore", invalid="ignore"):
        gii = (p / (s * s + lam)[:, :, None]).sum(3)
        if n < nt:
            gii = gii + (1.0 - p.sum(3)) / lam
        return 1.0 / (noise * gii) - (1.0 if kind == LMMSE else 0.0)


def effective_sinr(sinr, beta, axis=-1):
    """EESM: -beta ln(mean_k exp(-sinr_k / beta)) along `axis` (default: the frequencies), the SINR of the flat
    channel with the same mean exponential error term; beta > 0 is the calibration constant of the modulation and
    coding scheme."""
    beta = float(beta)
    if not beta > 0.0:
        raise ValueError("effective_sinr: beta must be > 0")
    x = -np.asarray(sinr, np.float64) / beta
    m = x.max(axis, keepdims=True)
    return -beta * (np.squeeze(m, axis) + np.log(np.exp(x - m).mean(axis)))


def rate(sinr, axis=2):
    """sum log2(1 + sinr) along `axis` (default: the streams of [nrx, ntx, Nt, 2, T, K]), bit/s/Hz per point"""
    return np.log2(1.0 + np.asarray(sinr, np.float64)).sum(axis)


def stack_users(H, side="tx"):
    """Several links as one matrix per point (numpy array or torch tensor [nrx, ntx, Nr, Nt, 2, T, K]):
    side "tx": the transmitters of an uplink stacked along Nt -> [nrx, 1, Nr, ntx Nt, 2, T, K], column tx Nt + j;
    side "rx": the users of a downlink stacked along Nr      -> [1, ntx, nrx Nr, Nt, 2, T, K], row rx Nr + i.
    The equalizer of the result is the multi-user detector, its sinr the per-user (per-stream) SINR."""
    if len(H.shape) != 7 or H.shape[4] != 2:
        raise ValueError("stack_users: H must be [nrx, ntx, Nr, Nt, 2, T, K], got %s" % (tuple(H.shape),))
    nrx, ntx, nr, nt, _, T, K = (int(x) for x in H.shape)
    perm = H.permute if hasattr(H, "permute") else H.transpose
    if side == "tx":
        return perm(0, 2, 1, 3, 4, 5, 6).reshape(nrx, 1, nr, ntx * nt, 2, T, K)
    if side == "rx":
        return perm(1, 0, 2, 3, 4, 5, 6).reshape(1, ntx, nrx * nr, nt, 2, T, K)
    raise ValueError("stack_users: side must be 'tx' or 'rx', got %r" % (side,))
