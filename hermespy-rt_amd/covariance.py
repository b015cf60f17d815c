"""Host side of the spatial covariance matrices (Tracer.array_covariance, hermespy_rt.compute_array_covariance): the
float64 reference from a path list and what a link-level simulator builds on the matrices, in plain numpy.

    from_terms    R = sum_p p s(u_p) s(u_p)^H from the powers and directions of a link's terms
    correlation   the matrix with a unit diagonal, R[i, k] / sqrt(R[i, i] R[k, k])
    kronecker     the Kronecker model of the full covariance E[vec(H) vec(H)^H] from R_rx and R_tx
    beam_power    the long-term power w^H R w of every beam of a codebook, without running beam_channel
    eigen_beams   the n dominant eigenvectors of R as a codebook that beam_channel / beam_taps accept

The conventions are those of include/hermespy_rt.h (hrt_compute_array_covariance): with H the array channel [Nr, Nt] of a
link under independent uniform path phases, R_rx = E[H H^H] / Nt and R_tx[j, j'] = E[sum_i H[i, j] conj(H[i, j'])] / Nr,
both with trace N sum_p p.  Codebooks are those of hermespy_rt_amd.beams: an RX codebook is a combiner, applied
conjugated (w^H); a TX codebook is a precoder, applied as it is.
"""
import numpy as np

from . import beams

C0 = beams.C0


def _steering(elements, directions, frequency):
    """beams.steering, exact where the phase is a multiple of a quarter revolution (the factor is then one of 1, j,
    -1, -j to the bit, as sincospi gives it on the device)"""
    r = np.asarray(elements, np.float64).reshape(-1, 3)
    u = np.asarray(directions, np.float64).reshape(-1, 3)
    ph = (float(frequency) / C0) * (u @ r.T)
    x = 4.0 * (ph - np.rint(ph))            # quarter revolutions, in [-2, 2]
    k = np.rint(x)
    a = 0.5 * np.pi * (x - k)               # the rest, within an eighth of a revolution
    return (np.cos(a) + 1j * np.sin(a)) * np.array([1, 1j, -1, -1j])[k.astype(np.int64) % 4]


def from_terms(powers, directions, elements, frequency):
    """complex128 [..., N, N]: R[i, k] = sum_p powers[..., p] s_i(u_p) conj(s_k(u_p)) with s = beams.steering of the
    elements [N, 3] (metres) towards the directions u [P, 3] at `frequency` (Hz).  powers [..., P] (e.g. [2, P]: one
    row per polarisation) are the terms' |a|^2; the directions are u_rx for R_rx and u_tx for R_tx."""
    p = np.asarray(powers, np.float64)
    s = _steering(elements, directions, frequency)
    if p.shape[-1] != s.shape[0]:
        raise ValueError("from_terms: %d powers for %d directions" % (p.shape[-1], s.shape[0]))
    R = np.matmul(p[..., None, :] * s.T, s.conj())   # [..., N, P] @ [P, N]
    return 0.5 * (R + R.conj().swapaxes(-1, -2))      # Hermitian to the bit, the diagonal real (exact sums stay exact)


def correlation(R):
    """R [..., N, N] with a unit diagonal: R[i, k] / sqrt(R[i, i] R[k, k]) (0 where an element receives no power)"""
    R = np.asarray(R)
    d = np.real(np.diagonal(R, axis1=-2, axis2=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d > 0, 1.0 / np.sqrt(d), 0.0)
    return R * q[..., :, None] * q[..., None, :]


def kronecker(R_rx, R_tx):
    """The Kronecker model of the full covariance of a link, [..., Nr Nt, Nr Nt]:

        E[vec(H) vec(H)^H] ~ kron(R_tx, R_rx) Nr / trace(R_rx)

    with vec stacking the COLUMNS of H [Nr, Nt] (vec(H)[j Nr + i] = H[i, j]).  It is kron(E[H^T conj(H)], E[H H^H]) /
    E[|H|_F^2] written in this module's normalisation (E[H H^H] = Nt R_rx, E[H^T conj(H)] = Nr R_tx); its trace is
    Nr Nt sum_p p, as that of the full covariance.  A link without power gives zeros."""
    R_rx, R_tx = np.asarray(R_rx), np.asarray(R_tx)
    nr, nt = R_rx.shape[-1], R_tx.shape[-1]
    tr = np.real(np.trace(R_rx, axis1=-2, axis2=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(tr > 0, nr / tr, 0.0)
    K = np.einsum("...jl,...ik->...jilk", R_tx, R_rx)
    return K.reshape(K.shape[:-4] + (nt * nr, nt * nr)) * np.asarray(scale)[..., None, None]


def beam_power(R, weights, side="rx"):
    """float64 [..., B]: the long-term power of every beam of the codebook `weights` [B, N] on R [..., N, N],
    sum_p p |g(u_p)|^2 in beam_channel's notation: w^H R w for an RX codebook (side="rx": the combiner is applied
    conjugated) and w^T R conj(w) for a TX codebook (side="tx": the precoder is applied as it is)."""
    if side not in ("rx", "tx"):
        raise ValueError("beam_power: side must be 'rx' or 'tx', got %r" % (side,))
    R, w = np.asarray(R), np.asarray(weights)
    if w.ndim == 1:
        w = w.reshape(1, -1)
    if w.ndim != 2 or R.ndim < 2 or R.shape[-1] != w.shape[1] or R.shape[-2] != w.shape[1]:
        raise ValueError("beam_power: R %s does not match weights %s" % (R.shape, w.shape))
    if side == "tx":
        w = np.conj(w)
    return np.real(np.einsum("bi,...ik,bk->...b", np.conj(w), R, w))


def eigen_beams(R, n, side="rx"):
    """complex128 [n, N]: the n dominant eigenvectors of the Hermitian R [N, N] (largest eigenvalue first, unit norm,
    the largest component of each real and positive) as a codebook for beam_channel / beam_taps: beam_power(R,
    eigen_beams(R, n, side), side) are the n largest eigenvalues.  side="tx" conjugates the vectors, as a precoder is
    applied without conjugation."""
    if side not in ("rx", "tx"):
        raise ValueError("eigen_beams: side must be 'rx' or 'tx', got %r" % (side,))
    R = np.asarray(R)
    if R.ndim != 2 or R.shape[0] != R.shape[1]:
        raise ValueError("eigen_beams: R must be [N, N], got %s" % (R.shape,))
    n = int(n)
    if not 1 <= n <= R.shape[0]:
        raise ValueError("eigen_beams: n = %d outside 1 .. %d" % (n, R.shape[0]))
    _, v = np.linalg.eigh(0.5 * (R + R.conj().T).astype(np.complex128))
    v = v[:, ::-1][:, :n].T                                   # rows: eigenvectors, largest eigenvalue first
    k = np.argmax(np.abs(v), axis=1)
    v = v * np.exp(-1j * np.angle(v[np.arange(n), k]))[:, None]
    return np.conj(v) if side == "tx" else v
