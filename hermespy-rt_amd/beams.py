"""Host side of the beamformed channel and taps (Tracer.beam_channel, Tracer.beam_taps, hermespy_rt.compute_beam_channel,
hermespy_rt.compute_beam_taps): codebooks, steering vectors and the contraction the device folds into the path sum, in
plain numpy.

    dft_codebook   the unitary DFT codebook of an n-element uniform linear array (one beam per row)
    steering       the plane-wave response of an array towards given directions
    gains          the gains g[beam, direction] of a codebook towards given directions: what ranks the beams of a
                   dominant-path list's directions on the host
    apply          B = conj(W_rx) H W_tx^T on an array_channel or array_taps result: what beam_channel and beam_taps
                   compute without forming H

The convention is that of include/hermespy_rt.h (hrt_compute_beam_channel): the RX codebook is a combiner and is
applied conjugated (w^H), the TX codebook is a precoder and is applied as it is (f); nothing is normalised.  With
rx_weights = steering(rx_elements, u_rx, f_a) a path arriving from u_rx is received with gain Nr; with tx_weights =
conj(steering(tx_elements, u_tx, f_a)) a path leaving along u_tx is sent with gain Nt.
"""
import numpy as np

C0 = 299792458.0


def dft_codebook(n):
    """complex128 [n, n]: row b is the beam exp(-j 2 pi b i / n) / sqrt(n) over the elements i; the rows are
    orthonormal (W W^H = I)"""
    n = int(n)
    if n < 1:
        raise ValueError("dft_codebook: n must be >= 1, got %d" % n)
    i = np.arange(n)
    return np.exp(-2j * np.pi * np.outer(i, i) / n) / np.sqrt(n)


def steering(elements, directions, frequency):
    """complex128 [d, n]: exp(j 2 pi f r_i . u / c) of the elements r_i [n, 3] (metres) towards the unit vectors u
    [d, 3] (or [3]: one row), the per-path factor of array_channel() for an arrival (RX) or departure (TX) direction u"""
    r = np.asarray(elements, np.float64).reshape(-1, 3)
    u = np.asarray(directions, np.float64)
    one = u.ndim == 1
    ph = (float(frequency) / C0) * (u.reshape(-1, 3) @ r.T)
    s = np.exp(2j * np.pi * (ph - np.rint(ph)))
    return s[0] if one else s


def gains(elements, weights, directions, frequency, conj=False):
    """complex128 [b, d]: g[beam, direction] = sum_i w[beam, i] exp(j 2 pi f r_i . u / c) of a codebook w [b, n] (or [n]:
    one beam) over the elements r_i [n, 3] towards the unit vectors u [d, 3] (or [3]: one column); conj=True applies the
    codebook conjugated, as the RX side does.  With the u_rx (conj=True) or u_tx of a dominant-path list these are the
    g_rx[a](u_rx_p) and g_tx[b](u_tx_p) of beam_channel() and sparse_beam_channel()."""
    w = np.asarray(weights, np.complex128)
    w = w.reshape(1, -1) if w.ndim == 1 else w
    s = steering(elements, np.asarray(directions, np.float64).reshape(-1, 3), frequency)   # [d, n]
    if w.ndim != 2 or w.shape[1] != s.shape[1]:
        raise ValueError("gains: weights %s do not match %d elements" % (w.shape, s.shape[1]))
    return (np.conj(w) if conj else w) @ s.T


def apply(H, rx_weights, tx_weights):
    """B[rx, tx, a, b, ...] = sum_ij conj(W_rx[a, i]) H[rx, tx, i, j, ...] W_tx[b, j] of an array channel
    (array_channel) or of array taps (array_taps: the trailing axes are then pol, time, tap) [nrx, ntx, Nr, Nt, ...]
    (numpy; complex128 unless everything is complex64) with W_rx [Br, Nr] and W_tx [Bt, Nt]"""
    H = np.asarray(H)
    wr, wt = np.asarray(rx_weights), np.asarray(tx_weights)
    if wr.ndim != 2 or wt.ndim != 2 or H.ndim < 4 or H.shape[2] != wr.shape[1] or H.shape[3] != wt.shape[1]:
        raise ValueError("apply: H %s does not match rx_weights %s and tx_weights %s"
                         % (H.shape, wr.shape, wt.shape))
    return np.einsum("ai,rtij...,bj->rtab...", np.conj(wr), H, wt)
