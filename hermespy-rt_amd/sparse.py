"""Host side of the array channel of dominant-path lists (Tracer.sparse_array_channel / Tracer.sparse_channel,
hermespy_rt.compute_sparse_array_channel), numpy only:

    reference       H of include/hermespy_rt.h (hrt_compute_sparse_array_channel) in float64, in the device layout,
                    together with S = sum_p |a_p^pol| per link and polarisation (what the float32 result's error
                    scales with)
    taps_reference  h of include/hermespy_rt.h (hrt_compute_sparse_array_taps: Tracer.sparse_array_taps /
                    Tracer.sparse_taps, hermespy_rt.compute_sparse_array_taps) in float64, likewise, with S
    beam_reference  B of include/hermespy_rt.h (hrt_compute_sparse_beam_channel: Tracer.sparse_beam_channel,
                    hermespy_rt.compute_sparse_beam_channel) in float64, likewise, with S
    beam_taps_reference  h of include/hermespy_rt.h (hrt_compute_sparse_beam_taps: Tracer.sparse_beam_taps,
                    hermespy_rt.compute_sparse_beam_taps) in float64, likewise, with S
    dropped_power   the link's power from power_profiles minus the power the kept paths carry
    cluster_list    a synthetic list (clusters of rays per link) as a result dict, through dominant.from_terms

`views` is a result dict of abi.dominant_views (Tracer.dominant_paths, dominant.merge, dominant.from_terms), numpy or
torch.
"""
import numpy as np

from . import abi, dominant

SPEED_OF_LIGHT = 299792458.0


def _numpy(v):
    return v if isinstance(v, np.ndarray) else v.cpu().numpy()


def reference(views, rx_elements, tx_elements, fa, f, t):
    """(H, S): H complex128 [nrx, ntx, Nr, Nt, 2, T, K] over the first min(kept, K) slots of every link at the
    frequencies f [K] (Hz) and times t [T] (s), elements [Nr, 3] / [Nt, 3] (m) and array frequency fa (Hz); S float64
    [nrx, ntx, 2] = sum_p |a_p^pol| over the same slots.  The slots' floats are widened to float64, nothing else is
    rounded; slots at or beyond min(kept, K) are not read."""
    re = abi.elements(rx_elements, "rx_elements").astype(np.float64)
    te = abi.elements(tx_elements, "tx_elements").astype(np.float64)
    f = np.atleast_1d(np.asarray(f, np.float64))
    t = np.atleast_1d(np.asarray(t, np.float64))
    kept = _numpy(views["kept"]).astype(np.int64).view(np.uint64)
    nrx, ntx, K = _numpy(views["tau"]).shape
    amp = np.stack([_numpy(views["a_te"]), _numpy(views["a_tm"])], axis=-1).astype(np.complex128)   # [.., K, 2]
    tau, nu = _numpy(views["tau"]).astype(np.float64), _numpy(views["freq_shift"]).astype(np.float64)
    urx, utx = _numpy(views["u_rx"]).astype(np.float64), _numpy(views["u_tx"]).astype(np.float64)
    H = np.zeros((nrx, ntx, re.shape[0], te.shape[0], 2, t.size, f.size), np.complex128)
    S = np.zeros((nrx, ntx, 2), np.float64)
    for rx in range(nrx):
        for tx in range(ntx):
            n = int(min(int(kept[rx, tx]), K))
            if n == 0:
                continue
            a = amp[rx, tx, :n]                                                               # [n, 2]
            W = np.exp(2j * np.pi * (nu[rx, tx, :n, None, None] * t[None, :, None]
                                     - f[None, None, :] * tau[rx, tx, :n, None, None]))      # [n, T, K]
            d = (urx[rx, tx, :n] @ re.T)[:, :, None] + (utx[rx, tx, :n] @ te.T)[:, None, :]   # [n, Nr, Nt] metres
            St = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * d)
            H[rx, tx] = np.einsum("pij,pq,pmk->ijqmk", St, a, W)
            S[rx, tx] = np.abs(a).sum(axis=0)
    return H, S


def taps_reference(views, rx_elements, tx_elements, fa, fs, fc, l, t):
    """(h, S): h complex128 [nrx, ntx, Nr, Nt, 2, T, L] of include/hermespy_rt.h (hrt_compute_sparse_array_taps) over the
    first min(kept, K) slots of every link at the taps l [L] (integers), times t [T] (s), sampling rate fs and baseband
    centre fc (Hz), elements [Nr, 3] / [Nt, 3] (m) and array frequency fa (Hz); S float64 [nrx, ntx, 2] =
    sum_p |a_p^pol| over the same slots.  The slots' floats are widened to float64, nothing else is rounded; the sinc
    is numpy's sin(pi x) / (pi x); slots at or beyond min(kept, K) are not read."""
    re = abi.elements(rx_elements, "rx_elements").astype(np.float64)
    te = abi.elements(tx_elements, "tx_elements").astype(np.float64)
    l = np.atleast_1d(np.asarray(l, np.float64))
    t = np.atleast_1d(np.asarray(t, np.float64))
    kept = _numpy(views["kept"]).astype(np.int64).view(np.uint64)
    nrx, ntx, K = _numpy(views["tau"]).shape
    amp = np.stack([_numpy(views["a_te"]), _numpy(views["a_tm"])], axis=-1).astype(np.complex128)   # [.., K, 2]
    tau, nu = _numpy(views["tau"]).astype(np.float64), _numpy(views["freq_shift"]).astype(np.float64)
    urx, utx = _numpy(views["u_rx"]).astype(np.float64), _numpy(views["u_tx"]).astype(np.float64)
    h = np.zeros((nrx, ntx, re.shape[0], te.shape[0], 2, t.size, l.size), np.complex128)
    S = np.zeros((nrx, ntx, 2), np.float64)
    for rx in range(nrx):
        for tx in range(ntx):
            n = int(min(int(kept[rx, tx]), K))
            if n == 0:
                continue
            a = amp[rx, tx, :n]                                                               # [n, 2]
            W = np.exp(2j * np.pi * (nu[rx, tx, :n, None] * t[None, :] - fc * tau[rx, tx, :n, None]))   # [n, T]
            V = np.sinc(l[None, :] - fs * tau[rx, tx, :n, None])                              # [n, L]
            d = (urx[rx, tx, :n] @ re.T)[:, :, None] + (utx[rx, tx, :n] @ te.T)[:, None, :]   # [n, Nr, Nt] metres
            St = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * d)
            h[rx, tx] = np.einsum("pij,pq,pm,pl->ijqml", St, a, W, V, optimize=True)
            S[rx, tx] = np.abs(a).sum(axis=0)
    return h, S


def beam_reference(views, rx_elements, tx_elements, rx_weights, tx_weights, fa, f, t):
    """(B, S): B complex128 [nrx, ntx, Br, Bt, 2, T, K] of include/hermespy_rt.h (hrt_compute_sparse_beam_channel) over
    the first min(kept, K) slots of every link at the frequencies f [K] (Hz) and times t [T] (s), elements [Nr, 3] /
    [Nt, 3] (m), array frequency fa (Hz) and codebooks rx_weights [Br, Nr] (applied conjugated) / tx_weights [Bt, Nt];
    S float64 [nrx, ntx, 2] = sum_p |a_p^pol| over the same slots.  The slots' floats and the weights are widened to
    float64, nothing else is rounded; slots at or beyond min(kept, K) are not read.  The element-domain matrix is not
    formed: the gains g_rx[a](u_rx_p) and g_tx[b](u_tx_p) are, per slot."""
    re = abi.elements(rx_elements, "rx_elements").astype(np.float64)
    te = abi.elements(tx_elements, "tx_elements").astype(np.float64)
    wr = abi.weights(rx_weights, re.shape[0], "rx_weights").astype(np.complex128)
    wt = abi.weights(tx_weights, te.shape[0], "tx_weights").astype(np.complex128)
    f = np.atleast_1d(np.asarray(f, np.float64))
    t = np.atleast_1d(np.asarray(t, np.float64))
    kept = _numpy(views["kept"]).astype(np.int64).view(np.uint64)
    nrx, ntx, K = _numpy(views["tau"]).shape
    amp = np.stack([_numpy(views["a_te"]), _numpy(views["a_tm"])], axis=-1).astype(np.complex128)   # [.., K, 2]
    tau, nu = _numpy(views["tau"]).astype(np.float64), _numpy(views["freq_shift"]).astype(np.float64)
    urx, utx = _numpy(views["u_rx"]).astype(np.float64), _numpy(views["u_tx"]).astype(np.float64)
    B = np.zeros((nrx, ntx, wr.shape[0], wt.shape[0], 2, t.size, f.size), np.complex128)
    S = np.zeros((nrx, ntx, 2), np.float64)
    for rx in range(nrx):
        for tx in range(ntx):
            n = int(min(int(kept[rx, tx]), K))
            if n == 0:
                continue
            a = amp[rx, tx, :n]                                                               # [n, 2]
            W = np.exp(2j * np.pi * (nu[rx, tx, :n, None, None] * t[None, :, None]
                                     - f[None, None, :] * tau[rx, tx, :n, None, None]))      # [n, T, K]
            gr = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * (urx[rx, tx, :n] @ re.T)) @ np.conj(wr).T   # [n, Br]
            gt = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * (utx[rx, tx, :n] @ te.T)) @ wt.T            # [n, Bt]
            B[rx, tx] = np.einsum("pa,pb,pq,pmk->abqmk", gr, gt, a, W, optimize=True)
            S[rx, tx] = np.abs(a).sum(axis=0)
    return B, S


def beam_taps_reference(views, rx_elements, tx_elements, rx_weights, tx_weights, fa, fs, fc, l, t):
    """(h, S): h complex128 [nrx, ntx, Br, Bt, 2, T, L] of include/hermespy_rt.h (hrt_compute_sparse_beam_taps) over the
    first min(kept, K) slots of every link at the taps l [L] (integers), times t [T] (s), sampling rate fs and baseband
    centre fc (Hz), elements [Nr, 3] / [Nt, 3] (m), array frequency fa (Hz) and codebooks rx_weights [Br, Nr] (applied
    conjugated) / tx_weights [Bt, Nt]; S float64 [nrx, ntx, 2] = sum_p |a_p^pol| over the same slots.  The slots'
    floats and the weights are widened to float64, nothing else is rounded; the sinc is numpy's sin(pi x) / (pi x);
    slots at or beyond min(kept, K) are not read.  The element-domain taps are not formed: the gains g_rx[a](u_rx_p)
    and g_tx[b](u_tx_p) are, per slot."""
    re = abi.elements(rx_elements, "rx_elements").astype(np.float64)
    te = abi.elements(tx_elements, "tx_elements").astype(np.float64)
    wr = abi.weights(rx_weights, re.shape[0], "rx_weights").astype(np.complex128)
    wt = abi.weights(tx_weights, te.shape[0], "tx_weights").astype(np.complex128)
    l = np.atleast_1d(np.asarray(l, np.float64))
    t = np.atleast_1d(np.asarray(t, np.float64))
    kept = _numpy(views["kept"]).astype(np.int64).view(np.uint64)
    nrx, ntx, K = _numpy(views["tau"]).shape
    amp = np.stack([_numpy(views["a_te"]), _numpy(views["a_tm"])], axis=-1).astype(np.complex128)   # [.., K, 2]
    tau, nu = _numpy(views["tau"]).astype(np.float64), _numpy(views["freq_shift"]).astype(np.float64)
    urx, utx = _numpy(views["u_rx"]).astype(np.float64), _numpy(views["u_tx"]).astype(np.float64)
    h = np.zeros((nrx, ntx, wr.shape[0], wt.shape[0], 2, t.size, l.size), np.complex128)
    S = np.zeros((nrx, ntx, 2), np.float64)
    for rx in range(nrx):
        for tx in range(ntx):
            n = int(min(int(kept[rx, tx]), K))
            if n == 0:
                continue
            a = amp[rx, tx, :n]                                                               # [n, 2]
            W = np.exp(2j * np.pi * (nu[rx, tx, :n, None] * t[None, :] - fc * tau[rx, tx, :n, None]))   # [n, T]
            V = np.sinc(l[None, :] - fs * tau[rx, tx, :n, None])                              # [n, L]
            gr = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * (urx[rx, tx, :n] @ re.T)) @ np.conj(wr).T   # [n, Br]
            gt = np.exp(2j * np.pi * (fa / SPEED_OF_LIGHT) * (utx[rx, tx, :n] @ te.T)) @ wt.T            # [n, Bt]
            h[rx, tx] = np.einsum("pa,pb,pq,pm,pl->abqml", gr, gt, a, W, V, optimize=True)
            S[rx, tx] = np.abs(a).sum(axis=0)
    return h, S


def dropped_power(views, moments):
    """the power of every link that the list does not carry, [nrx, ntx]: the link's whole power (the moments of
    power_profiles for the same parts, POWER_P of both polarisations) minus the kept slots' power"""
    power, kept = _numpy(views["power"]), _numpy(views["kept"]).astype(np.int64)
    m = _numpy(moments)
    total = m[..., 0, abi.POWER_P] + m[..., 1, abi.POWER_P]
    got = np.where(np.arange(power.shape[-1]) < kept[..., None], power, 0.0).sum(axis=-1)
    return total - got


def cluster_list(nrx, ntx, K, link, a_te, a_tm, tau, freq_shift, u_rx, u_tx, bounce=None, path=None):
    """A synthetic list as a result dict (numpy): one term per entry of `link` [n] (rx * ntx + tx) with complex
    amplitudes a_te / a_tm [n], delay tau and Doppler freq_shift [n] and unit directions u_rx / u_tx [n, 3]; the K
    strongest per link are kept in the order of the contract (dominant.from_terms).  bounce defaults to 1 and path to
    the term's index, which keeps the order strict."""
    link = np.asarray(link, np.int64).reshape(-1)
    n = link.size
    a_te = np.asarray(a_te).astype(np.complex64).reshape(n)
    a_tm = np.asarray(a_tm).astype(np.complex64).reshape(n)
    f32 = lambda x, s: np.asarray(x).astype(np.float32).reshape(s)   # noqa: E731
    cols = dict(power=dominant.term_power(a_te, a_tm),
                path=(np.arange(n) if path is None else np.asarray(path)).astype(np.int64).view(np.uint64),
                bounce=(np.ones(n) if bounce is None else np.asarray(bounce)).astype(np.int32),
                tri=np.zeros(n, np.uint32), a_te=a_te, a_tm=a_tm, tau=f32(tau, n), freq_shift=f32(freq_shift, n),
                u_rx=f32(u_rx, (n, 3)), u_tx=f32(u_tx, (n, 3)))
    return dominant.from_terms(link, cols, nrx, ntx, K)
