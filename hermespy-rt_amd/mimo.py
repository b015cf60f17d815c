"""Host side of the per-point MIMO SVD (Tracer.svd / Tracer.channel_svd, hermespy_rt.compute_channel_svd), numpy only:
the float64 reference in the device layout and what a link-level simulator reads from the decomposition.

    svd_reference     sigma, u, v of every point of H [nrx, ntx, Nr, Nt, 2, T, K] in float64, in the device layout
    capacity          equal-power capacity  sum_i log2(1 + snr sigma_i^2 / Nt)            (bit/s/Hz per point)
    waterfilling      capacity with the power snr poured over the singular values
    condition_number  sigma_0 / sigma_{n-1}
    rank              columns that are not null by the device's rule: sigma_i > max(Nr, Nt) 2^-23 sigma_0
    precoder          the first `streams` right vectors of ONE point as a TX codebook (streams, Nt)
    combiner          the first `streams` left vectors of ONE point as an RX codebook (streams, Nr)

The conventions are those of include/hermespy_rt.h (hrt_compute_channel_svd): H = u diag(sigma) v^H, sigma descending
along axis 2 of [nrx, ntx, n, 2, T, K] (a 1-D sigma is one point).  Codebooks are those of hermespy_rt_amd.beams: the
combiner is applied conjugated (w^H), the precoder as it is, so beam_channel(precoder(v, s), combiner(u, s)) of a point
is diag(sigma[:s]) there.  The noise power is 1: `snr` is the total transmit power over the noise power.
"""
import numpy as np

NULL_EPS = 2.0 ** -23   # times max(Nr, Nt): the device's null rule and column floor


def _axis(sigma, axis):
    s = np.asarray(sigma, np.float64)
    if axis is None:
        axis = 0 if s.ndim == 1 else 2
    return np.moveaxis(s, axis, -1)


def svd_reference(H):
    """H complex [nrx, ntx, Nr, Nt, 2, T, K] -> dict of float64 / complex128 arrays in the device layout: sigma
    [nrx, ntx, n, 2, T, K] (descending), u [nrx, ntx, Nr, n, 2, T, K], v [nrx, ntx, Nt, n, 2, T, K] with
    H = u diag(sigma) v^H (numpy.linalg.svd per point; the gauge is LAPACK's)."""
    H = np.asarray(H)
    if H.ndim != 7 or H.shape[4] != 2:
        raise ValueError("svd_reference: H must be [nrx, ntx, Nr, Nt, 2, T, K], got %s" % (H.shape,))
    A = np.moveaxis(H.astype(np.complex128), (2, 3), (-2, -1))           # [nrx, ntx, 2, T, K, Nr, Nt]
    u, s, vh = np.linalg.svd(A, full_matrices=False)
    v = np.conj(np.swapaxes(vh, -1, -2))
    return {"sigma": np.moveaxis(s, -1, 2), "u": np.moveaxis(u, (-2, -1), (2, 3)),
            "v": np.moveaxis(v, (-2, -1), (2, 3))}


def capacity(sigma, snr, nt, axis=None):
    """sum_i log2(1 + snr sigma_i^2 / nt): the capacity with the power snr spread evenly over the nt transmit
    elements, = log2 det(I + snr / nt H H^H).  sigma [nrx, ntx, n, 2, T, K] (or `axis`; 1-D: one point)."""
    s = _axis(sigma, axis)
    return np.log2(1.0 + float(snr) / float(nt) * s * s).sum(-1)


def waterfilling(sigma, snr, axis=None):
    """The capacity with the power snr poured over the singular values: p_i = max(mu - 1 / sigma_i^2, 0) with
    sum_i p_i = snr, sum_i log2(1 + p_i sigma_i^2).  sigma as in capacity(); a point without gain gives 0."""
    s = -np.sort(-_axis(sigma, axis), axis=-1)
    n = s.shape[-1]
    with np.errstate(divide="ignore"):
        inv = np.where(s > 0, 1.0 / np.where(s > 0, s * s, 1.0), np.inf)    # 1 / g_i, ascending
    out = np.zeros(s.shape[:-1])
    found = np.zeros(s.shape[:-1], bool)
    for k in range(n, 0, -1):                                               # the largest k whose level covers 1 / g_k
        head = inv[..., :k]
        ok = np.isfinite(head).all(-1)
        mu = (float(snr) + np.where(ok[..., None], head, 0.0).sum(-1)) / k
        ok = ok & ~found & (mu > inv[..., k - 1])
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.log2(np.where(ok[..., None], mu[..., None] / np.where(ok[..., None], head, 1.0), 1.0)).sum(-1)
        out = np.where(ok, c, out)
        found |= ok
    return out


def condition_number(sigma, axis=None):
    """sigma_0 / sigma_{n-1} (inf where the smallest is 0, nan for a zero matrix)"""
    s = _axis(sigma, axis)
    with np.errstate(divide="ignore", invalid="ignore"):
        return s.max(-1) / s.min(-1)


def rank(sigma, nr, nt, axis=None):
    """The number of columns that are not null by the device's rule: sigma_i > max(nr, nt) 2^-23 sigma_0 (0 for a zero
    matrix)."""
    s = _axis(sigma, axis)
    return (s > max(int(nr), int(nt)) * NULL_EPS * s.max(-1, keepdims=True)).sum(-1)


def _codebook(x, streams, name):
    x = np.asarray(x)
    if x.ndim != 2:
        raise ValueError("%s: the vectors of one point [N, n] expected, got %s" % (name, x.shape))
    streams = int(streams)
    if not 1 <= streams <= x.shape[1]:
        raise ValueError("%s: streams = %d outside 1 .. %d" % (name, streams, x.shape[1]))
    return np.ascontiguousarray(x[:, :streams].T)


def precoder(v, streams):
    """(streams, Nt): the first right vectors v[:, :streams] of ONE point (v [Nt, n]) as the rows of a TX codebook
    (applied as it is)"""
    return _codebook(v, streams, "precoder")


def combiner(u, streams):
    """(streams, Nr): the first left vectors u[:, :streams] of ONE point (u [Nr, n]) as the rows of an RX codebook
    (applied conjugated: w^H)"""
    return _codebook(u, streams, "combiner")
