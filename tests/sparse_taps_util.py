"""What tests/test_sparse_taps_design.py, tests/test_sparse_taps_args.py (no device) and the GPU tests of the array taps
of path lists (Tracer.sparse_array_taps) share: the exact planting, an independent per-path loop, a float32 mirror of
the kernel's U, sinc and MFMA-order stages, the wrong readings a kernel could make (MUTANTS) and the exact check.

The exact planting extends tests/sparse_util.py's (elements on the 1/32 m lattice, f_a = 8 c, directions on the axes,
amplitude components in {0, +-1, +-2}, nu in {+-64, +-128, 256} Hz, dt = 2^-8 s, t0 = 0) with

    f_s = 2^18 Hz, f_c = 2^16 Hz, tau = q 2^-18 s with integer q        f_s tau = q,  f_c tau = q / 4

so f_s tau is the integer q exactly: by csrc/hrt_sinc.h sinpif(0) = 0, the sinc weight is exactly 1 at tap q and +-0 at
every other tap, and every phase is a whole number of quarter revolutions.  Every output is a Gaussian integer of
modulus at most 4 K: the sum of the terms whose q lands on that tap.  The q of a planted list lie inside the window
[l_min, l_min + L) and outside it, l_min - 1 and l_min + L among them.  As in sparse_util EVERY slot holds such a term,
the slots at and beyond `kept` too, and eligible = kept + 3."""
import cmath
import math

import numpy as np
import pytest

from hermespy_rt_amd import sparse

from . import covariance_util as CU
from . import planted as PL
from . import sparse_util as U

F_A = U.F_A
FS, FC = float(1 << 18), float(1 << 16)
T0, DT = U.T0, U.DT
TAU_STEP = 2.0 ** -18
BATCH = 32            # HRT_TP_BATCH of csrc/hrt_taps.h
elements, copy, check_exact = U.elements, U.copy, U.check_exact


def offsets(L):
    """the delays of a planting relative to l_min: both window edges, one beyond each, and taps inside"""
    return np.array(sorted({-1, 0, L - 1, L, L // 2, min(1, L - 1), L + 5, -7, (3 * L) // 4}), np.int64)


def planted(nrx, ntx, K, kept, l_min, L, salt=0, los_slot=True):
    """tests/sparse_util.py's planted list with the delays of this planting: q = l_min + one of offsets(L) per slot"""
    v = U.planted(nrx, ntx, K, kept, salt, los_slot)
    link = np.broadcast_to(np.arange(nrx * ntx).reshape(nrx, ntx, 1), (nrx, ntx, K))
    slot = np.broadcast_to(np.arange(K), (nrx, ntx, K))
    off = offsets(L)
    q = l_min + off[((PL.mix(link, slot, 0xC0 + salt) >> np.uint64(11)) % np.uint64(len(off))).astype(np.int64)]
    v["tau"][...] = (q.astype(np.float64) * TAU_STEP).astype(np.float32)
    return v


def one_hot(nrx, ntx, link, component, q, salt=0):
    """sparse_util.one_hot with the live slot's delay at tap q"""
    v = U.one_hot(nrx, ntx, link, component, salt=salt)
    v["tau"][...] = np.float32(q * TAU_STEP)
    return v


def delays(v):
    """the integer q of every slot"""
    q = v["tau"].astype(np.float64) / TAU_STEP
    assert np.array_equal(q, np.rint(q))
    return np.rint(q).astype(np.int64)


def loop_reference(v, re, te, fa, fs, fc, l, t):
    """h of include/hermespy_rt.h by a direct loop over links, slots, pairs, polarisations, times and taps with cmath
    and math: shares nothing with sparse.taps_reference but the definition"""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float64), np.asarray(te, np.float64)
    h = np.zeros((nrx, ntx, len(re), len(te), 2, len(t), len(l)), np.complex128)
    for rx in range(nrx):
        for tx in range(ntx):
            for p in range(min(int(v["kept"][rx, tx]), K)):
                amp = (complex(v["a_te"][rx, tx, p]), complex(v["a_tm"][rx, tx, p]))
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                urx, utx = v["u_rx"][rx, tx, p].astype(np.float64), v["u_tx"][rx, tx, p].astype(np.float64)
                w = []
                for li in l:
                    x = math.pi * (float(li) - fs * tau)
                    w.append(1.0 if x == 0.0 else math.sin(x) / x)
                for i in range(len(re)):
                    for j in range(len(te)):
                        d = sum(re[i][q] * urx[q] for q in range(3)) + sum(te[j][q] * utx[q] for q in range(3))
                        s = cmath.exp(2j * cmath.pi * fa * d / sparse.SPEED_OF_LIGHT)
                        for pol in range(2):
                            for m in range(len(t)):
                                ph = amp[pol] * s * cmath.exp(2j * cmath.pi * (nu * t[m] - fc * tau))
                                for k in range(len(l)):
                                    h[rx, tx, i, j, pol, m, k] += ph * w[k]
    return h


def exact_reference(v, re, te, l_min, L, nt, tau_phase_sign=1, tap_shift=0):
    """the Gaussian-integer h of a planted list on the exact grid, from the phases counted in quarter revolutions and the
    taps as integers: complex128 [nrx, ntx, Nr, Nt, 2, nt, L], every value exact.  (tau_phase_sign = -1 and tap_shift
    = +-1 are two of the wrong readings.)"""
    nrx, ntx, K = v["tau"].shape
    kr = np.rint(np.asarray(re, np.float64) / CU.STEP).astype(np.int64)
    kt = np.rint(np.asarray(te, np.float64) / CU.STEP).astype(np.int64)
    unit = np.array([1, 1j, -1, -1j])
    h = np.zeros((nrx, ntx, len(kr), len(kt), 2, nt, L), np.complex128)
    mm = np.arange(nt)
    qs = delays(v)
    for rx in range(nrx):
        for tx in range(ntx):
            for p in range(min(int(v["kept"][rx, tx]), K)):
                q = int(qs[rx, tx, p])
                k = q - l_min + tap_shift
                if not 0 <= k < L:
                    continue
                nu4 = int(round(float(v["freq_shift"][rx, tx, p]) * DT * 4))                  # quarter revs per step
                st = (kr @ np.rint(v["u_rx"][rx, tx, p]).astype(np.int64))[:, None] + \
                     (kt @ np.rint(v["u_tx"][rx, tx, p]).astype(np.int64))[None, :]          # [Nr, Nt] quarter revs
                ph = unit[(st[:, :, None] + (nu4 * mm)[None, None, :] - tau_phase_sign * q) % 4]   # f_c tau = q / 4
                h[rx, tx, :, :, 0, :, k] += complex(v["a_te"][rx, tx, p]) * ph
                h[rx, tx, :, :, 1, :, k] += complex(v["a_tm"][rx, tx, p]) * ph
    return h


def _sinpi32(x):
    """float32 sin(pi x) of float32 x in [-1/2, 1/2], exactly 0 at 0 (as sinpif is)"""
    return np.sin(np.pi * x.astype(np.float64)).astype(np.float32)


def sinc_weights_f32(fs, tau, l):
    """float32 mirror of csrc/hrt_sinc.h (sinc_prep, sinc_tap) for one float32 delay at the integer taps l [L]"""
    f32 = np.float32
    x = fs * float(tau)
    n = np.rint(x)
    k = min(max(n, -67108864.0), 67108864.0)
    s = f32(_sinpi32(np.array(x - n, f32)) * f32(0.318309886183790672))
    r = f32(x - k)
    c = s if (0.5 * n) != math.floor(0.5 * n) else f32(-s)
    d = (np.asarray(l, np.int64) - int(k)).astype(f32) - r
    cc = np.where(np.asarray(l, np.int64) & 1, -c, c).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = cc * (f32(1.0) / d)
    return np.where(np.abs(d) < f32(1e-4), f32(1.0), w).astype(f32)


def mirror_f32(v, re, te, fa, fs, fc, l_min, L, nt, t0=T0, dt=DT):
    """A float32 mirror of the kernel's stages (csrc/hrt_sparse_taps.hip, csrc/hrt_taps_gemm.inc): U = a exp(j 2 pi (nu
    t_m - f_c tau + f_a (r . u_rx + q . u_tx) / c)) with its phase formed and reduced in float64 and evaluated in float32,
    the sinc weights of csrc/hrt_sinc.h in float32, and the sum over the slots in the MFMA's order: four slots a step
    added in index order onto the accumulator, in float32.  complex64 [nrx, ntx, Nr, Nt, 2, nt, L]."""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float32).astype(np.float64), np.asarray(te, np.float32).astype(np.float64)
    t = t0 + np.arange(nt) * dt
    l = l_min + np.arange(L)
    fac = fa / sparse.SPEED_OF_LIGHT
    f32 = np.float32
    h = np.zeros((nrx, ntx, len(re), len(te), 2, nt, L), np.complex64)
    for rx in range(nrx):
        for tx in range(ntx):
            acc_r = np.zeros(h.shape[2:], f32)
            acc_i = np.zeros(h.shape[2:], f32)
            for p in range(min(int(v["kept"][rx, tx]), K)):
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                d = (re @ v["u_rx"][rx, tx, p].astype(np.float64))[:, None] + \
                    (te @ v["u_tx"][rx, tx, p].astype(np.float64))[None, :]
                sn, cs = U._sincospi32(U._half_revs(nu * t[None, None, :] - fc * tau + fac * d[:, :, None]))  # [Nr,Nt,nt]
                w = sinc_weights_f32(fs, v["tau"][rx, tx, p], l)                                              # [L]
                for pol, a in enumerate((v["a_te"][rx, tx, p], v["a_tm"][rx, tx, p])):
                    ar, ai = f32(a.real), f32(a.imag)
                    ur, ui = ar * cs - ai * sn, ar * sn + ai * cs          # U (float32)
                    acc_r[:, :, pol] += ur[..., None] * w                  # one MFMA k-step: acc + u v, in float32
                    acc_i[:, :, pol] += ui[..., None] * w
            h[rx, tx] = acc_r + 1j * acc_i
    return h


# ------------------------------------------------------------------ the wrong readings a kernel could make
def _rows_time_pair(h):
    """the (pair, time) row a T + m read as m' Np + a'"""
    s = h.shape
    nl, npair, T, L = s[0] * s[1], s[2] * s[3], s[5], s[6]
    g = h.reshape(nl, npair, 2, T, L).transpose(0, 3, 1, 2, 4).reshape(nl, npair, T, 2, L)
    return np.ascontiguousarray(g.transpose(0, 1, 3, 2, 4)).reshape(s)


MUTANTS = tuple(sorted(n for n in U.LIST_MUTANTS if n != "tau_sign")) + (
    "pair_transposed", "steering_sign", "tau_phase_sign", "tap_off_by_one", "l_min_ignored", "rows_time_pair")


def mutant(name, v, re, te, l_min, L, nt):
    """the exact h a kernel with one wrong reading would give for the planted list v"""
    if name == "pair_transposed":   # the pair index j * Nr + i instead of i * Nt + j
        h = exact_reference(v, re, te, l_min, L, nt)
        return np.ascontiguousarray(h.swapaxes(2, 3)).reshape(h.shape)
    if name == "steering_sign":
        return exact_reference(v, -np.asarray(re, np.float64), -np.asarray(te, np.float64), l_min, L, nt)
    if name == "tau_phase_sign":
        return exact_reference(v, re, te, l_min, L, nt, tau_phase_sign=-1)
    if name == "tap_off_by_one":
        return exact_reference(v, re, te, l_min, L, nt, tap_shift=1)
    if name == "l_min_ignored":     # the taps counted from 0
        return exact_reference(v, re, te, l_min, L, nt, tap_shift=l_min)
    if name == "rows_time_pair":
        return _rows_time_pair(exact_reference(v, re, te, l_min, L, nt))
    w = copy(v)
    U.LIST_MUTANTS[name](w)
    return exact_reference(w, re, te, l_min, L, nt)


def tracer_value_errors(tr):
    """the ValueErrors of Tracer.sparse_array_taps / sparse_taps that are its own (tr has nrx, ntx = 2, 3)"""
    import torch
    v = planted(2, 3, 8, 5, 0, 4)
    kw = dict(fs=FS, num_taps=4)
    el = elements(2, 2)
    with pytest.raises(ValueError, match="uint8 buffer expected, got float32"):
        tr.sparse_array_taps(v["buffer"].view(np.float32), *el, **kw)
    with pytest.raises(ValueError, match="uint8 buffer"):
        tr.sparse_array_taps(torch.zeros(6 * (16 + 72 * 8) // 4, dtype=torch.float32), *el, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_array_taps(torch.from_numpy(v["buffer"]), *el, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_taps({"buffer": torch.from_numpy(v["buffer"]), "power": v["power"]}, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of 3552 bytes expected for \(nrx, ntx, K\) = \(2, 3, 8\)"):
        tr.sparse_array_taps({"buffer": v["buffer"][:-8], "power": v["power"]}, *el, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of \d+ bytes expected for \(nrx, ntx, K\) = \(2, 3, 7\)"):
        tr.sparse_array_taps(v["buffer"][:-8], *el, **kw)      # a bare buffer: this tracer's links, K from the size
    with pytest.raises(ValueError, match="element offsets must be finite"):
        tr.sparse_array_taps(v, np.full((2, 3), np.nan, np.float32), el[1], **kw)
    with pytest.raises(ValueError, match=r"rx_elements must have shape \(n, 3\)"):
        tr.sparse_array_taps(v, np.zeros((2, 2), np.float32), el[1], **kw)
