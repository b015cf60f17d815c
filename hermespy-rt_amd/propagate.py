"""Host side of the received signals (Tracer.apply_taps / Tracer.propagate, hrt_propagate), numpy only: the float64
reference of the definition, the block times a block-wise time-variant channel is formed at, the default sizes and the
rounding-error bound the device result is held to.

    y[rx, i, pol, n] = sum_tx sum_j sum_{l < L} h[rx, tx, i, j, pol, m(n), l] x[tx, j, n - l_min - l]
    m(n) = min(n // S, M - 1),   x[.., k] = 0 outside 0 <= k < N
"""
import numpy as np


def num_blocks(num_out, samples_per_block):
    """M of a block-wise channel over num_out samples: ceil(num_out / S); 1 for S None (time-invariant)"""
    if samples_per_block is None:
        return 1
    s = int(samples_per_block)
    if s < 1:
        raise ValueError("samples_per_block must be >= 1")
    return max((int(num_out) + s - 1) // s, 1)


def block_times(fs, samples_per_block, t_start=0.0):
    """(t0, dt) of the taps of a block-wise channel: block m is formed at its centre, t0 + m dt with
    t0 = t_start + (S - 1) / (2 fs), dt = S / fs; S None (one block): (t_start, 0)"""
    if samples_per_block is None:
        return float(t_start), 0.0
    s = int(samples_per_block)
    return float(t_start) + (s - 1) / (2.0 * float(fs)), s / float(fs)


def default_num_out(num_samples, num_taps, l_min=0):
    """the output length that holds every non-zero sample of a causal window: N + L - 1 + max(l_min, 0)"""
    return int(num_samples) + int(num_taps) - 1 + max(int(l_min), 0)


def _shapes(h, x):
    h, x = np.asarray(h), np.asarray(x)
    if h.ndim == 5:   # taps(): [nrx, ntx, 2, M, L]
        h = h[:, :, None, None]
    if x.ndim == 2:
        x = x[:, None]
    if h.ndim != 7 or x.ndim != 3 or h.shape[4] != 2 or h.shape[1] != x.shape[0] or h.shape[3] != x.shape[1]:
        raise ValueError("taps [nrx, ntx, Nr, Nt, 2, M, L] and signal [ntx, Nt, N] expected, got %s and %s"
                         % (h.shape, x.shape))
    return h, x


def apply_taps_reference(h, x, l_min=0, samples_per_block=None, num_out=None, dtype=np.complex128):
    """The definition in float64 (complex128), as plain loops over blocks, taps and TX ports -> [nrx, Nr, 2, num_out].
    samples_per_block None requires M = 1."""
    h, x = _shapes(h, x)
    nrx, ntx, nr, nt, _, M, L = h.shape
    N = x.shape[2]
    if samples_per_block is None and M != 1:
        raise ValueError("samples_per_block=None requires num_times = 1")
    n_out = default_num_out(N, L, l_min) if num_out is None else int(num_out)
    S = n_out if samples_per_block is None else int(samples_per_block)
    h = h.astype(dtype)
    x = x.astype(dtype)
    y = np.zeros((nrx, nr, 2, n_out), dtype)
    for m in range(M):
        lo = m * S
        hi = n_out if m == M - 1 else min((m + 1) * S, n_out)   # the last block keeps every later sample
        if lo >= hi:
            break
        n = np.arange(lo, hi)
        for l in range(L):
            k = n - int(l_min) - l
            ok = (k >= 0) & (k < N)
            if not ok.any():
                continue
            for tx in range(ntx):
                for j in range(nt):
                    # [nrx, nr, 2] x [samples]
                    y[:, :, :, n[ok]] += h[:, tx, :, j, :, m, l][..., None] * x[tx, j, k[ok]]
    return y


def error_bound(h, x, l_min=0, samples_per_block=None, num_out=None):
    """Per output element, the bound of a float32 multiply-add chain of the 2K real products of its K = ntx Nt L complex
    terms, in any order, with or without fused multiply-adds: gamma_2K sum |h| |x| with gamma_k = k u / (1 - k u),
    u = 2^-24.  (The two real products of a term that enter one part have |h_re x_re| + |h_im x_im| <= |h| |x|, so the
    sum of the complex moduli bounds the sum of the moduli of the chain's products; the bound holds for the real and
    the imaginary part each, hence for their larger.)  float64 [nrx, Nr, 2, num_out]."""
    h, x = _shapes(h, x)
    K = h.shape[1] * h.shape[3] * h.shape[6]
    ah = np.abs(h).astype(np.float64)
    ax = np.abs(x).astype(np.float64)
    s = apply_taps_reference(ah, ax, l_min, samples_per_block, num_out, dtype=np.float64)
    u = 2.0 ** -24
    return (2 * K * u) / (1.0 - 2 * K * u) * s
