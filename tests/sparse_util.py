"""What tests/test_sparse_design.py, tests/test_sparse_args.py (no device) and the GPU tests of the array channel of
path lists (Tracer.sparse_array_channel) share: the exact planting of lists, an independent per-path loop, a float32
mirror of the kernel's U, V and S stages, the wrong readings a kernel could make (MUTANTS) and the exact check.

The exact planting:

    f_a = 8 c Hz, elements on (1/32 m) {0..7}^3    (tests/covariance_util.py): f_a r . u / c = k / 4 for u on an axis
    u_rx, u_tx in {+-e_x, +-e_y, +-e_z}
    amplitudes in {+-1, +-2, 0} per component
    f0 = 2^30 Hz, df = 2^16 Hz, tau = n 2^-18 s, n in 0 .. 7         f_k tau = n 2^12 + k n / 4
    nu in {+-64, +-128, 256} Hz, t0 = 0, dt = 2^-8 s                 nu t_m = +-m / 4, +-m / 2, m

so every phase is a whole number of quarter revolutions, every factor is one of 1, j, -1, -j, and every output is a
Gaussian integer of modulus at most 4 K <= 2^12: exact in float32 in any summation order.  EVERY slot of a planted list
holds such a term, the slots at and beyond `kept` too, and `eligible` = kept + 3: a kernel that reads a slot it must
not, or the header the other way round, gives another Gaussian integer somewhere."""
import cmath

import numpy as np
import pytest

from hermespy_rt_amd import abi, sparse

from . import covariance_util as CU
from . import planted as PL

F_A = CU.F_A
F0, DF = float(1 << 30), float(1 << 16)
T0, DT = 0.0, 2.0 ** -8
TAU_STEP = 2.0 ** -18
NUS = np.array([64.0, -64.0, 128.0, -128.0, 256.0])
AMPS = np.array([1.0, -1.0, 2.0, -2.0, 0.0])
BATCH, PAIRS, COLS = 32, 32, 256   # HRT_AC_BATCH, HRT_AC_PAIRS, HRT_AC_GROWS * 16 of csrc/hrt_array_channel.h


def grid(nk, nt):
    """(f [nk], t [nt]) of the exact grid"""
    return F0 + DF * np.arange(nk), T0 + DT * np.arange(nt)


def elements(nr, nt):
    """exact element offsets: (rx [nr, 3], tx [nt, 3]) on the lattice, the two sides different"""
    return CU.exact_elements(nr, 1), CU.exact_elements(nt, 2)


def _pick(table, *key):
    return table[(PL.mix(*key) >> np.uint64(13)) % np.uint64(len(table))]


def planted(nrx, ntx, K, kept, salt=0, los_slot=True):
    """A planted result dict (numpy, abi.dominant_views of a new buffer) with `kept` [nrx, ntx] (or one number for every
    link) live slots and eligible = kept + 3; every one of the K slots of every link holds an exact term (module
    docstring).  Slot 1 of every link (slot 0 where K = 1) is a LoS entry (bounce -1, a_te = a_tm real) if los_slot."""
    v = abi.dominant_views(np.zeros(nrx * ntx * (16 + 72 * K), np.uint8), nrx, ntx, K)
    link = np.broadcast_to(np.arange(nrx * ntx).reshape(nrx, ntx, 1), (nrx, ntx, K))
    slot = np.broadcast_to(np.arange(K), (nrx, ntx, K))
    comp = [_pick(AMPS, link, slot, 0xA0 + q + 16 * salt) for q in range(4)]
    dead = (comp[0] == 0) & (comp[1] == 0) & (comp[2] == 0) & (comp[3] == 0)
    comp[0] = np.where(dead, 1.0, comp[0])
    v["a_te"][...] = (comp[0] + 1j * comp[1]).astype(np.complex64)
    v["a_tm"][...] = (comp[2] + 1j * comp[3]).astype(np.complex64)
    v["tau"][...] = ((PL.mix(link, slot, 0xB0 + salt) >> np.uint64(9)) % np.uint64(8)).astype(np.float32) * TAU_STEP
    v["freq_shift"][...] = _pick(NUS, link, slot, 0xB1 + salt)
    v["u_rx"][...] = _pick(CU.AXES, link, slot, 0xB2 + salt)
    v["u_tx"][...] = _pick(CU.AXES, link, slot, 0xB3 + salt)
    v["bounce"][...] = 1 + (slot % 3)
    v["path"][...] = (link * K + slot).astype(np.uint64)
    v["tri"][...] = 7
    if los_slot:
        s = min(1, K - 1)
        v["bounce"][:, :, s] = -1
        v["path"][:, :, s] = np.uint64(0xFFFFFFFFFFFFFFFF)
        v["tri"][:, :, s] = 0xFFFFFFFF
        a = v["a_te"][:, :, s].real
        v["a_te"][:, :, s] = np.where(a == 0, 2.0, a)
        v["a_tm"][:, :, s] = v["a_te"][:, :, s]
        v["u_rx"][:, :, s] = -v["u_tx"][:, :, s]
    v["power"][...] = (np.abs(v["a_te"]).astype(np.float64) ** 2 + np.abs(v["a_tm"]).astype(np.float64) ** 2)
    kept = np.broadcast_to(np.asarray(kept, np.uint64), (nrx, ntx))
    v["kept"][...] = kept
    v["eligible"][...] = kept + np.uint64(3)
    return v


def one_hot(nrx, ntx, link, component, value=1.0, salt=0):
    """A list of K = 1 whose only live slot is on `link` and has one nonzero amplitude component (0 te re, 1 te im,
    2 tm re, 3 tm im); the slots of the other links hold terms but are not live (kept = 0)."""
    kept = np.zeros(nrx * ntx, np.uint64)
    kept[link] = 1
    v = planted(nrx, ntx, 1, kept.reshape(nrx, ntx), salt, los_slot=False)
    a = np.zeros(4)
    a[component] = value
    rx, tx = divmod(link, ntx)
    v["a_te"][rx, tx, 0] = a[0] + 1j * a[1]
    v["a_tm"][rx, tx, 0] = a[2] + 1j * a[3]
    return v


def copy(v):
    """a deep copy of a result dict"""
    nrx, ntx, K = v["tau"].shape
    return abi.dominant_views(v["buffer"].copy(), nrx, ntx, K)


def loop_reference(v, re, te, fa, f, t):
    """H of include/hermespy_rt.h by a direct loop over links, slots, pairs, polarisations and grid points with cmath:
    shares nothing with sparse.reference but the definition"""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float64), np.asarray(te, np.float64)
    H = np.zeros((nrx, ntx, len(re), len(te), 2, len(t), len(f)), np.complex128)
    for rx in range(nrx):
        for tx in range(ntx):
            n = min(int(v["kept"][rx, tx]), K)
            for p in range(n):
                amp = (complex(v["a_te"][rx, tx, p]), complex(v["a_tm"][rx, tx, p]))
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                urx, utx = v["u_rx"][rx, tx, p].astype(np.float64), v["u_tx"][rx, tx, p].astype(np.float64)
                for i in range(len(re)):
                    for j in range(len(te)):
                        d = sum(re[i][q] * urx[q] for q in range(3)) + sum(te[j][q] * utx[q] for q in range(3))
                        s = cmath.exp(2j * cmath.pi * fa * d / sparse.SPEED_OF_LIGHT)
                        for pol in range(2):
                            for m in range(len(t)):
                                for k in range(len(f)):
                                    H[rx, tx, i, j, pol, m, k] += amp[pol] * s * cmath.exp(
                                        2j * cmath.pi * (nu * t[m] - f[k] * tau))
    return H


def exact_reference(v, re, te, nk, nt):
    """the Gaussian-integer H of a planted list on the exact grid, from the phases counted in quarter revolutions with
    integer arithmetic: complex128 [nrx, ntx, Nr, Nt, 2, nt, nk], every value exact"""
    nrx, ntx, K = v["tau"].shape
    kr = np.rint(np.asarray(re, np.float64) / CU.STEP).astype(np.int64)
    kt = np.rint(np.asarray(te, np.float64) / CU.STEP).astype(np.int64)
    unit = np.array([1, 1j, -1, -1j])
    H = np.zeros((nrx, ntx, len(kr), len(kt), 2, nt, nk), np.complex128)
    kk, mm = np.arange(nk), np.arange(nt)
    for rx in range(nrx):
        for tx in range(ntx):
            n = min(int(v["kept"][rx, tx]), K)
            for p in range(n):
                nt_ = int(round(float(v["tau"][rx, tx, p]) / TAU_STEP))
                nu4 = int(round(float(v["freq_shift"][rx, tx, p]) * DT * 4))                  # quarter revs per step
                st = (kr @ np.rint(v["u_rx"][rx, tx, p]).astype(np.int64))[:, None] + \
                     (kt @ np.rint(v["u_tx"][rx, tx, p]).astype(np.int64))[None, :]          # [Nr, Nt] quarter revs
                q = (st[:, :, None, None] + (nu4 * mm)[None, None, :, None] - (nt_ * kk)[None, None, None, :]) % 4
                ph = unit[q]
                H[rx, tx, :, :, 0] += complex(v["a_te"][rx, tx, p]) * ph
                H[rx, tx, :, :, 1] += complex(v["a_tm"][rx, tx, p]) * ph
    return H


def _half_revs(ph):
    return (2.0 * (ph - np.rint(ph))).astype(np.float32)


def _sincospi32(x):
    """float32 sin(pi x), cos(pi x) of float32 x in [-1, 1], exact at the multiples of 1/2 (as sincospif is)"""
    x = x.astype(np.float64)
    s, c = np.sin(np.pi * x), np.cos(np.pi * x)
    h = np.rint(2 * x)
    on = (2 * x == h)
    s = np.where(on, np.array([0.0, 1.0, 0.0, -1.0])[h.astype(np.int64) % 4], s)
    c = np.where(on, np.array([1.0, 0.0, -1.0, 0.0])[h.astype(np.int64) % 4], c)
    return s.astype(np.float32), c.astype(np.float32)


def mirror_f32(v, re, te, fa, nk, nt, f0=F0, df=DF, t0=T0, dt=DT):
    """A float32 mirror of the kernel's stages (csrc/hrt_pair_gemm.inc, csrc/hrt_sparse_channel.hip): U = a exp(j 2 pi
    (nu t_m - f_{16 k1} tau)), V = exp(-j 2 pi k2 df tau) and S = exp(j 2 pi f_a (r . u_rx + q . u_tx) / c) with their
    phases reduced in float64 and evaluated in float32, B = U V in float32, and the sum over the slots in index order in
    float32.  complex64 [nrx, ntx, Nr, Nt, 2, nt, nk]."""
    nrx, ntx, K = v["tau"].shape
    re, te = np.asarray(re, np.float32).astype(np.float64), np.asarray(te, np.float32).astype(np.float64)
    k1, k2 = np.arange(nk) // 16, np.arange(nk) % 16
    t = t0 + np.arange(nt) * dt
    fac = fa / sparse.SPEED_OF_LIGHT
    H = np.zeros((nrx, ntx, len(re), len(te), 2, nt, nk), np.complex64)
    f32 = np.float32
    for rx in range(nrx):
        for tx in range(ntx):
            acc_r = np.zeros(H.shape[2:], f32)
            acc_i = np.zeros(H.shape[2:], f32)
            for p in range(min(int(v["kept"][rx, tx]), K)):
                tau, nu = float(v["tau"][rx, tx, p]), float(v["freq_shift"][rx, tx, p])
                us, uc = _sincospi32(_half_revs(nu * t[:, None] - (f0 + (k1 * 16) * df)[None, :] * tau))   # [nt, nk]
                vs, vc = _sincospi32(_half_revs(-(k2 * df) * tau))                                         # [nk]
                d = (re @ v["u_rx"][rx, tx, p].astype(np.float64))[:, None] + \
                    (te @ v["u_tx"][rx, tx, p].astype(np.float64))[None, :]
                ss, sc = _sincospi32(_half_revs(fac * d))                                                  # [Nr, Nt]
                for pol, a in enumerate((v["a_te"][rx, tx, p], v["a_tm"][rx, tx, p])):
                    ar, ai = f32(a.real), f32(a.imag)
                    ur, ui = ar * uc - ai * us, ar * us + ai * uc          # U (float32)
                    br, bi = ur * vc - ui * vs, ur * vs + ui * vc          # B = U V (float32)
                    acc_r[:, :, pol] += sc[:, :, None, None] * br - ss[:, :, None, None] * bi
                    acc_i[:, :, pol] += ss[:, :, None, None] * br + sc[:, :, None, None] * bi
            H[rx, tx] = acc_r + 1j * acc_i
    return H


# ------------------------------------------------------------------ the wrong readings a kernel could make
def _swap_dirs(v):
    a = v["u_rx"].copy()
    v["u_rx"][...] = v["u_tx"]
    v["u_tx"][...] = a


def _swap_pols(v):
    a = v["a_te"].copy()
    v["a_te"][...] = v["a_tm"]
    v["a_tm"][...] = a


def _neg(key):
    def f(v):
        v[key][...] = -v[key]
    return f


def _kept_plus_one(v):
    K = v["tau"].shape[2]
    v["kept"][...] = np.minimum(v["kept"] + np.uint64(1), np.uint64(K))


def _skip_los(v):
    los = v["bounce"] == -1
    v["a_te"][los] = 0
    v["a_tm"][los] = 0


def _header_swapped(v):
    v["kept"][...] = v["eligible"]


LIST_MUTANTS = {
    "urx_utx_swapped": _swap_dirs,
    "tau_sign": _neg("tau"),
    "nu_sign": _neg("freq_shift"),
    "te_tm_swapped": _swap_pols,
    "slot_n_read": _kept_plus_one,
    "los_skipped": _skip_los,
    "header_eligible_kept": _header_swapped,
}
MUTANTS = tuple(sorted(LIST_MUTANTS)) + ("pair_transposed", "steering_sign")


def mutant(name, v, re, te, nk, nt):
    """the exact H a kernel with one wrong reading would give for the planted list v"""
    if name == "pair_transposed":   # the pair index j * Nr + i instead of i * Nt + j
        H = exact_reference(v, re, te, nk, nt)
        return np.ascontiguousarray(H.swapaxes(2, 3)).reshape(H.shape)
    if name == "steering_sign":
        return exact_reference(v, -np.asarray(re, np.float64), -np.asarray(te, np.float64), nk, nt)
    w = copy(v)
    LIST_MUTANTS[name](w)
    return exact_reference(w, re, te, nk, nt)


def check_exact(got, ref, what=""):
    """got (complex64) equals the Gaussian-integer ref value for value (`==`: either sign of a zero passes)"""
    got = np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.complex64, (what, got.shape, ref.shape, got.dtype)
    want = ref.astype(np.complex64)
    assert np.array_equal(want.astype(np.complex128), ref), (what, "the reference is not exact in float32")
    bad = got != want
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def tracer_value_errors(tr):
    """the ValueErrors of Tracer.sparse_array_channel / sparse_channel that are its own (tr has nrx, ntx = 2, 3)"""
    import torch
    v = planted(2, 3, 8, 5)
    kw = dict(f0=F0, df=DF, num_freqs=4)
    el = elements(2, 2)
    with pytest.raises(ValueError, match="uint8 buffer expected, got float32"):
        tr.sparse_array_channel(v["buffer"].view(np.float32), *el, **kw)
    with pytest.raises(ValueError, match="uint8 buffer"):
        tr.sparse_array_channel(torch.zeros(6 * (16 + 72 * 8) // 4, dtype=torch.float32), *el, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_array_channel(torch.from_numpy(v["buffer"]), *el, **kw)
    with pytest.raises(ValueError, match="must be on cuda:0, got cpu"):
        tr.sparse_channel({"buffer": torch.from_numpy(v["buffer"]), "power": v["power"]}, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of 3552 bytes expected for \(nrx, ntx, K\) = \(2, 3, 8\)"):
        tr.sparse_array_channel({"buffer": v["buffer"][:-8], "power": v["power"]}, *el, **kw)
    with pytest.raises(ValueError, match=r"a flat buffer of \d+ bytes expected for \(nrx, ntx, K\) = \(2, 3, 7\)"):
        tr.sparse_array_channel(v["buffer"][:-8], *el, **kw)      # a bare buffer: this tracer's links, K from the size
    with pytest.raises(ValueError, match=r"a flat buffer of 3552 bytes expected"):
        tr.sparse_array_channel({"buffer": v["buffer"].reshape(6, -1), "power": v["power"]}, *el, **kw)
    with pytest.raises(ValueError, match="element offsets must be finite"):
        tr.sparse_array_channel(v, np.full((2, 3), np.nan, np.float32), el[1], **kw)
    with pytest.raises(ValueError, match=r"rx_elements must have shape \(n, 3\)"):
        tr.sparse_array_channel(v, np.zeros((2, 2), np.float32), el[1], **kw)
