"""Antenna-array (MIMO) sampled impulse responses formed on the device (Tracer.array_taps, hrt_array_taps,
hermespy_rt.compute_array_taps) against float64 numpy sums over the same float inputs:

    h[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p))
                                       * exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c) sinc(l_min + k - f_s tau_p)

u_rx: Tracer.paths()' direction_rx (LoS: -HRT_LOS_DIR); u_tx: hrt_launch_dirs_host of the record's global path (LoS:
HRT_LOS_DIR).  Tolerance per (link, i, j, pol), over all (m, k): |h - h64| <= 1e-5 * sum_p |a_p^pol|.  Then the
identities of the contract (the DTFT is compute_array_channel, one element is compute_taps, a pair is a one-pair
call), the planted workspaces of tests/planted.py record by record, the structure (shards, accumulate, determinism,
record chunks) and the drop-in entries."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import planted as PL
from . import scenes_gen as G
from .pathsum_util import ARRAY_CASES as CASES
from .pathsum_util import (C0, CONFIGS, FS, PARTS, _bits, _cfg, _expect_failure, _force_los_classes, _geometries, _lam,
                           _los_status, _traced, _tracer, _ula, _upa)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sum(h, S, link, a_te, a_tm, tau, nu, urx, utx, rxe, txe, fa, fs, fc, l, t, chunk=512):
    """h[link] += float64 sums over the given paths (float32 inputs), S[link] += sum |a| (per pol)"""
    rxe, txe = np.asarray(rxe, np.float64), np.asarray(txe, np.float64)
    nr, nt = rxe.shape[0], txe.shape[0]
    for i in range(0, tau.size, chunk):
        ta, nv = tau[i:i + chunk].astype(np.float64), nu[i:i + chunk].astype(np.float64)
        ph = nv[:, None] * t[None, :] - fc * ta[:, None]
        e = np.exp(2j * np.pi * (ph - np.rint(ph)))                                      # [p, T]
        st = (fa / C0) * ((urx[i:i + chunk].astype(np.float64) @ rxe.T)[:, :, None] +
                          (utx[i:i + chunk].astype(np.float64) @ txe.T)[:, None, :])
        s = np.exp(2j * np.pi * (st - np.rint(st))).reshape(ta.size, nr * nt)            # [p, pairs]
        v = np.sinc(l[None, :] - fs * ta[:, None])                                        # [p, L]
        for pol, a in enumerate((a_te, a_tm)):
            u = a[i:i + chunk].astype(np.complex128)[:, None, None] * s[:, :, None] * e[:, None, :]
            h[link][:, :, pol] += np.einsum("pam,pl->aml", u, v).reshape(nr, nt, t.size, l.size)
    S[link][0] += np.abs(a_te.astype(np.complex128)).sum()
    S[link][1] += np.abs(a_tm.astype(np.complex128)).sum()


def _reference_lt(tr, fs, l, t, rxe, txe, fa=None, fc=None, los=True, scatter=True):
    """float64 array taps on the taps l and times t, from Tracer.paths() + Tracer.los()"""
    fa = tr.f_ghz * 1e9 if fa is None else fa
    fc = tr.f_ghz * 1e9 if fc is None else fc
    l, t = np.asarray(l, np.float64), np.asarray(t, np.float64)
    h = np.zeros((tr.nrx, tr.ntx, len(rxe), len(txe), 2, t.size, l.size), np.complex128)
    S = np.zeros((tr.nrx, tr.ntx, 2))
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
        ub = P["unblocked"]
        dirs = PL.launch_dirs(tr).astype(np.float32)
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                s = (P["rx"] == rx) & (P["tx"] == tx) & ub
                _sum(h, S, (rx, tx), P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s],
                     P["direction_rx"][s], dirs[P["path"][s]], rxe, txe, fa, fs, fc, l, t)
    if los and tr.shard.rank == 0:
        L = tr.los()
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                q = L[rx, tx]
                status = _los_status(q)
                if status == 0:   # coincident: directions_tx = (-1, 0, 0), directions_rx = (1, 0, 0)
                    a, tau, nu, u = 1.0, 0.0, 0.0, np.array([-1.0, 0.0, 0.0], np.float32)
                elif status == 2:   # HRT_LOS_DIR is directions_tx
                    a, tau, nu, u = float(q[1]), float(q[2]), float(q[6]), q[3:6].copy()
                else:
                    continue
                one = np.array([a], np.float32)
                _sum(h, S, (rx, tx), one, one, np.array([tau], np.float32), np.array([nu], np.float32),
                     -u[None, :], u[None, :], rxe, txe, fa, fs, fc, l, t)
    return h, S


def _reference(tr, fs, nl, rxe, txe, l_min=0, t0=0.0, dt=0.0, nt=1, **kw):
    return _reference_lt(tr, fs, l_min + np.arange(nl), t0 + np.arange(nt) * dt, rxe, txe, **kw)


def _check(got, h, S, scale=1.0):
    got = np.asarray(got)
    assert got.shape == h.shape and got.dtype == np.complex64
    assert np.isfinite(got.view(np.float32)).all()
    err = np.abs(got.astype(np.complex128) - h).reshape(*h.shape[:5], -1).max(axis=-1)   # (rx, tx, i, j, pol)
    bound = scale * 1e-5 * S[:, :, None, None, :] + 1e-30
    assert (err <= bound).all(), (err / np.maximum(S[:, :, None, None, :], 1e-30)).max()


ONE = np.zeros((1, 3))


def _small_geometry(c):
    """2 x 1 pairs: Nr Nt T < 13 at T = 1 and T = 4 (the RT = 1 form)"""
    return ("ula2_one", _ula(2, _lam(c) / 2), np.array([[0.0, 0.0, _lam(c) / 3]]))


# (num_times, num_taps, l_min, fs): T = 1 and T = 4, L not a multiple of 16, a negative l_min
GRIDS = [(1, 77, -7, FS), (4, 40, 3, 1e9)]


# ------------------------------------------------------------------ 1. float64 reference
@pytest.mark.parametrize("name,n", [(c[0], c[1]) for c in CASES], ids=[c[0] for c in CASES])
def test_array_taps_match_float64(name, n):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    for gname, rxe, txe in _geometries(c) + [_small_geometry(c)]:
        for nt, nl, l_min, fs in GRIDS:
            dt = 1e-4 if nt > 1 else 0.0
            got = tr.array_taps(rxe, txe, fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
            h, S = _reference(tr, fs, nl, rxe, txe, l_min, dt=dt, nt=nt)
            _check(got, h, S)
    tr.close()


# ------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize("nt", [1, 2])
def test_dtft_of_the_array_taps_is_the_array_channel(nt):
    """single TX, every delay at least M taps inside the window: the DTFT of the taps at |f| <= f_s / 4 is
    Tracer.array_channel at f_c + f with the same f_a and elements"""
    c = K.small(K.C3_DOPPLER, 20000)
    tr = _tracer(c)
    assert tr.ntx == 1
    tr.trace()
    lam = _lam(c)
    rxe, txe = _ula(2, lam / 2), _upa(2, 2, lam / 2)
    fs, M = FS, 2000
    P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=True).items()}
    taus = [P["tau"].astype(np.float64)]
    los = tr.los()
    for rx in range(tr.nrx):
        if _los_status(los[rx, 0]) == 2:
            taus.append(np.array([float(los[rx, 0, 2])]))
    x = np.concatenate(taus) * fs
    lo, hi = int(np.floor(x.min())), int(np.ceil(x.max()))
    l_min, nl = lo - M, (hi - lo) + 2 * M
    fc = tr.f_ghz * 1e9
    dt = 1e-4
    h = tr.array_taps(rxe, txe, fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy().astype(np.complex128)
    nk = 33
    f = -fs / 4 + np.arange(nk) * (fs / 2 / (nk - 1))
    H = tr.array_channel(rxe, txe, fc - fs / 4, fs / 2 / (nk - 1), nk, dt=dt, num_times=nt).cpu().numpy()
    l = l_min + np.arange(nl, dtype=np.float64)
    dtft = h @ np.exp(-2j * np.pi * np.outer(l, f) / fs)
    # the sinc tails cut at M taps (see test_gpu_taps.test_dtft_of_the_taps_is_the_channel), plus the float error
    _, S = _reference(tr, fs, 1, ONE, ONE)
    tol = (2 * math.sqrt(2) / (math.pi * (M - 1)) + 1e-5) * S
    assert tol.max() <= 2e-3 * S.max()
    err = np.abs(dtft - H).reshape(*H.shape[:5], -1).max(axis=-1)   # (rx, tx, i, j, pol)
    assert (err <= tol[:, :, None, None, :]).all(), (err / S[:, :, None, None, :]).max()
    tr.close()


@pytest.mark.parametrize("name,n", [("C3", 20000), ("C4_DOPPLER", 4000), ("COINCIDENT", 8000)])
def test_single_element_at_the_origin_is_the_taps(name, n):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    for nt, nl, l_min in ((2, 150, -3), (16, 40, 0)):   # (T = 16: the RT = 4 form of both)
        dt = 1e-4
        got = tr.array_taps(ONE, ONE, FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
        want = tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
        assert got.shape == (tr.nrx, tr.ntx, 1, 1, 2, nt, nl)
        h, S = _reference(tr, FS, nl, ONE, ONE, l_min, dt=dt, nt=nt)
        _check(got, h, S)
        bound = 1e-5 * S[:, :, :, None, None]
        assert (np.abs(got[:, :, 0, 0].astype(np.complex128) - want) <= 2 * bound).all()
        print(name, nt, "bit-identical to taps:", np.array_equal(got[:, :, 0, 0].view(np.float32),
                                                                 want.view(np.float32)))
    tr.close()


def test_pair_is_the_one_pair_call():
    """pair (i, j) of a many-element call equals a call with the single pair (r_i, q_j)"""
    c = K.small(K.C4_DOPPLER, 4000)
    tr = _tracer(c)
    tr.trace()
    _, rxe, txe = _geometries(c)[1]   # random7 x ULA2
    nl, l_min, nt, dt = 70, -5, 3, 1e-4
    got = tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
    _, S = _reference(tr, FS, 1, ONE, ONE)
    for i in range(rxe.shape[0]):
        for j in range(txe.shape[0]):
            one = tr.array_taps(rxe[i:i + 1], txe[j:j + 1], FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
            d = np.abs(got[:, :, i, j].astype(np.complex128) - one[:, :, 0, 0])
            assert (d.reshape(tr.nrx, tr.ntx, 2, -1).max(axis=-1) <= 2e-5 * S).all(), (i, j)
    tr.close()


# ------------------------------------------------------------------ 3. planted workspaces
PLANTED_TOL = 1e-3   # one f32 sincospi per term; the weakest planted term is 1/2


def array_taps_planted(T, nrx, ntx, rxe, txe, fa, L, l_min, t):
    """float64 array taps of planted terms (fs = FS, fc = FC: every fs tau_p = n_p an integer): tap n_p - l_min of
    pair (i, j) is the record's taps term (PL.taps_direct) times its steering (PL.array_direct), every other tap 0"""
    t = np.asarray(t, np.float64)
    rxe, txe = np.asarray(rxe, np.float32).astype(np.float64), np.asarray(txe, np.float32).astype(np.float64)
    nr, nt = rxe.shape[0], txe.shape[0]
    assert np.array_equal(T["tau"] * PL.FS, T["n"].astype(np.float64))
    h = np.zeros((nrx * ntx, nr * nt, 2, t.size, L), np.complex128)
    k = T["n"] - l_min
    ok = (k >= 0) & (k < L)
    U = PL.select(T, ok)
    link = PL.link_of(U, ntx)
    e = PL.cis(U["nu"][:, None] * t[None, :] - PL.FC * U["tau"][:, None])                     # [p, T]
    g = PL.cis((fa / PL.C0) * ((U["urx"] @ rxe.T)[:, :, None] + (U["utx"] @ txe.T)[:, None, :]))
    g = g.reshape(-1, nr * nt)                                                                   # [p, pairs]
    for pol, a in enumerate(("a_te", "a_tm")):
        w = U[a][:, None, None] * g[:, :, None] * e[:, None, :]                                  # [p, pairs, T]
        for pr in range(nr * nt):
            for m in range(t.size):
                np.add.at(h[:, pr, pol, m], (link, k[ok]), w[:, pr, m])
    return h.reshape(nrx, ntx, nr, nt, 2, t.size, L)


def _check_planted(got, T, nrx, ntx, rxe, txe, fa, L, l_min, t, what="array taps"):
    return PL.check_close(got, array_taps_planted(T, nrx, ntx, rxe, txe, fa, L, l_min, t), PLANTED_TOL, what, T, ntx)


@pytest.fixture(scope="module", params=["C3", "C4_DOPPLER"])
def planted(request, tmp_path_factory):
    tr, c = _traced(request.param, tmp_path_factory)
    T = PL.plant(tr)
    assert not PL.design_errors(T), PL.design_errors(T)
    yield request.param, tr, T
    tr.close()


def test_zero_offsets_give_the_planted_taps_on_every_pair(planted):
    name, tr, T = planted
    nmax, nt = int(T["n"].max()), 3
    t = PL.DT * np.arange(nt)
    z = np.zeros((2, 3)), np.zeros((3, 3))
    for los, scatter in PARTS:
        got = tr.array_taps(*z, PL.FS, nmax + 1, 0, fc=PL.FC, dt=PL.DT, num_times=nt, los=los,
                            scatter=scatter).cpu().numpy()
        Ts = PL.select(T, (T["los"] & los) | (~T["los"] & scatter))
        for i in range(2):
            for j in range(3):
                PL.check_taps_planted(np.ascontiguousarray(got[:, :, i, j]), Ts, tr.nrx, tr.ntx, nmax + 1, 0, t)


@pytest.mark.parametrize("nt", [1, 4])
def test_each_tap_is_one_record_times_its_steering(planted, nt):
    name, tr, T = planted
    lam = PL.C0 / (tr.f_ghz * 1e9)
    rxe = np.array([[0, 0, 0], [0, lam / 2, 0]], np.float32)
    txe = np.array([[0, 0, 0], [lam / 2, 0, lam / 3], [0, -lam / 4, lam / 2]], np.float32)
    fa = tr.f_ghz * 1e9
    nl = int(T["n"].max()) + 1
    t = PL.DT * np.arange(nt)
    full = None
    for los, scatter in PARTS:
        got = tr.array_taps(rxe, txe, PL.FS, nl, 0, fc=PL.FC, dt=PL.DT, num_times=nt, los=los,
                            scatter=scatter).cpu().numpy()
        Ts = PL.select(T, (T["los"] & los) | (~T["los"] & scatter))
        err = _check_planted(got, Ts, tr.nrx, tr.ntx, rxe, txe, fa, nl, 0, t)
        print(name, "array taps", nt, (los, scatter), "max |err|", err)
        full = got if los and scatter else full
    _expect_failure(lambda U: _check_planted(full, U, tr.nrx, tr.ntx, rxe, txe, fa, nl, 0, t), T, "array taps")
    # a window that cuts records off at both ends, with a negative t0
    lm, nw = 37, max(nl // 2, 1)
    tw = -5 * PL.DT + PL.DT * np.arange(nt)
    got = tr.array_taps(rxe, txe, PL.FS, nw, lm, fc=PL.FC, t0=tw[0], dt=PL.DT, num_times=nt).cpu().numpy()
    _check_planted(got, T, tr.nrx, tr.ntx, rxe, txe, fa, nw, lm, tw)
    assert (T["n"] < lm).any() and (T["n"] >= lm + nw).any()


def _run_array_taps(tr, los, scatter):
    """the array taps in both forms (RT = 4 and RT = 1) on the traced workspace, as raw output bytes"""
    rxe = np.array([[0, 0, 0], [0, 0.04, 0]], np.float32)
    txe = np.array([[0, 0, 0], [0.04, 0, 0], [0, 0, 0.04]], np.float32)
    out = {"rt4": _bits(tr.array_taps(rxe, txe, 122.88e6, 64, -8, t0=1e-3, dt=2e-4, num_times=3, los=los,
                                      scatter=scatter)),
           "rt1": _bits(tr.array_taps(rxe[:1], txe[:2], 122.88e6, 40, 5, t0=1e-3, dt=2e-4, num_times=2, los=los,
                                      scatter=scatter))}
    tr.torch.cuda.synchronize(tr.device)
    return out


@pytest.mark.parametrize("name", list(CONFIGS))
def test_poison_does_not_change_the_array_taps(name, tmp_path_factory):
    tr, c = _traced(name, tmp_path_factory)
    counts = tr.counts()
    _force_los_classes(tr)
    base = {parts: _run_array_taps(tr, *parts) for parts in PARTS}
    for parts, outs in base.items():
        for form, b in outs.items():
            assert bool(tr.torch.isfinite(b.view(tr.torch.float32)).all()), (name, parts, form)
    for value in (float("nan"), 1e30):
        hit = PL.poison(tr, counts, value)
        for cls in ("blocked_records", "tail_slots", "tail_mask_bits"):
            assert hit[cls] > 0, (name, cls, hit)
        for parts in PARTS:
            got = _run_array_taps(tr, *parts)
            for form, b in base[parts].items():
                assert bool(tr.torch.equal(got[form], b)), "%s: %s with %s changed after poison %r" % (
                    name, form, parts, value)
    tr.close()


# ------------------------------------------------------------------ 4. structure
def _nchunks(tr, rxe, txe, nl, nt):
    """the record chunks of an array taps call (host/channel.c at_plan), from its scratch size"""
    spec = abi.taps_spec(PL.FS, nl, 0, PL.FC, 0.0, 0.0, nt)
    el = np.ascontiguousarray(np.concatenate([rxe, txe]).astype(np.float32))
    arr = abi.ArraySpec(len(rxe), len(txe), el.ctypes.data, el.ctypes.data + 12 * len(rxe), 3e9)
    need = C.c_uint64(0)
    assert tr.L.hrt_array_taps_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(arr),
                                             C.byref(need)) == 0
    seg = (tr.nb * (tr.ntx + 1) * 4 + 255) // 256 * 256
    per = tr.nrx * tr.ntx * 2 * len(rxe) * len(txe) * nt * nl * 8
    assert (need.value - seg) % per == 0
    return (need.value - seg) // per


@pytest.mark.parametrize("rays,chunks", [(600, "one"), (1100, "two"), (20000, "many")])
def test_record_chunks(rays, chunks):
    tr = _tracer(K.small(K.C4_DOPPLER, rays))
    tr.trace()
    rxe = np.array([[0, 0, 0], [0, 0.05, 0]], np.float32)
    txe = np.array([[0, 0, 0], [0.05, 0, 0]], np.float32)
    T = PL.plant(tr)
    nl, nt = int(T["n"].max()) + 1, 2
    n = _nchunks(tr, rxe, txe, nl, nt)
    assert {"one": n == 1, "two": n == 2, "many": n > 2}[chunks], n
    t = 3 * PL.DT + PL.DT * np.arange(nt)
    got = tr.array_taps(rxe, txe, PL.FS, nl, 0, fc=PL.FC, t0=t[0], dt=PL.DT, num_times=nt).cpu().numpy()
    _check_planted(got, T, tr.nrx, tr.ntx, rxe, txe, tr.f_ghz * 1e9, nl, 0, t)
    tr.close()


def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nl, l_min, nt, dt = 120, -3, 2, 1e-4
    _, rxe, txe = _geometries(c)[0]
    tr = _tracer(c)
    tr.trace()
    whole = tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt)
    again = tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt, out=out, accumulate=True)
    tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt, out=out, accumulate=True)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    h, S = _reference(tr, FS, nl, rxe, txe, l_min, dt=dt, nt=nt)
    _check(whole.cpu().numpy(), h, S)
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt, out=acc,
                                accumulate=acc is not None)
            ts.close()
        _check(acc.cpu().numpy(), h, S)   # LoS counted once: the shards sum to the whole result


def test_scratch_too_small_is_refused():
    import torch
    c = K.small(K.C1, 2000)
    tr = _tracer(c)
    tr.trace()
    spec = abi.taps_spec(FS, 64, 0, 3e9)
    el = torch.zeros(6, dtype=torch.float32, device=tr.device)
    arr = abi.ArraySpec(1, 1, el.data_ptr(), el.data_ptr() + 12, 3e9)
    need = C.c_uint64(0)
    assert tr.L.hrt_array_taps_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(arr),
                                             C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty((1, 1, 1, 1, 2, 1, 64), dtype=torch.complex64, device=tr.device)
    rc = tr.L.hrt_array_taps(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec),
                             C.byref(arr), C.c_void_p(scratch.data_ptr()), C.c_uint64(int(need.value) - 1),
                             C.c_void_p(out.data_ptr()), 0, None)
    assert rc == -1 and b"hrt_array_taps: scratch" in tr.L.hrt_last_error()
    tr.close()


# ------------------------------------------------------------------ 5. drop-in entries
_PYBIND_CALL = """import sys
import numpy as np
sys.path.insert(0, {repo!r})
import hermespy_rt_amd
import torch  # noqa: F401  (HIP runtime first, see hermespy_rt_amd.lib)
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from tests import configs as K
c = K.small(K.C3, 20000)
rxe = np.load(sys.argv[2]).astype(np.float32)
txe = np.load(sys.argv[3]).astype(np.float32)
h = hermespy_rt.compute_array_taps(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                   np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                   np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]), len(c["tx_pos"]),
                                   c["num_paths"], c["num_bounces"], {fs!r}, {nl}, rxe, txe, l_min={l_min},
                                   dt={dt!r}, num_times={nt})
np.save(sys.argv[1], h)
st = lib.Stats()
spec = abi.taps_spec({fs!r}, {nl}, {l_min}, c["f_ghz"] * 1e9, 0.0, {dt!r}, {nt})
h2 = abi.run_compute_array_taps(lib.load(), *K.args(c), spec, rxe, txe, stats=st)
assert np.array_equal(h.view(np.float32), h2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_array_taps_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C) agrees with Tracer.array_taps on C3 at 20 k rays, also when a small workspace
    budget cuts the call into several batches"""
    c = K.small(K.C3, 20000)
    nl, l_min, nt, dt = 100, -7, 2, 1e-4
    _, rxe, txe = _geometries(c)[0]
    tr = _tracer(c)
    tr.trace()
    want = tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
    h, S = _reference(tr, FS, nl, rxe, txe, l_min, dt=dt, nt=nt)
    _check(want, h, S)
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    out, fr, ft = tmp_path / "h.npy", tmp_path / "rx.npy", tmp_path / "tx.npy"
    np.save(fr, rxe)
    np.save(ft, txe)
    code = _PYBIND_CALL.format(repo=REPO, fs=FS, nl=nl, l_min=l_min, dt=dt, nt=nt)
    p = subprocess.run([sys.executable, "-c", code, str(out), str(fr), str(ft)], env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = np.load(out)
    _check(got, h, S)
    assert np.abs(got.astype(np.complex128) - want).max() <= 2e-5 * S.max()


def test_generated_scene_resorted_two_tx(tmp_path):
    """> 1 024 triangles (the live list is re-sorted between bounces) and 2 TX: the TX segments of the hit blocks"""
    p = str(tmp_path / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
              tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    tr = _tracer(c)
    assert tr.num_tri > 1024
    tr.trace()
    nl, nt, dt = 75, 3, 1e-3
    for _, rxe, txe in _geometries(c):
        got = tr.array_taps(rxe, txe, FS, nl, l_min=-2, dt=dt, num_times=nt).cpu().numpy()
        h, S = _reference(tr, FS, nl, rxe, txe, -2, dt=dt, nt=nt)
        _check(got, h, S)
    tr.close()


def test_largest_grid():
    """Nr * Nt * T * L = 2^24 (the largest accepted): 64 pairs, T * L = 2^18; finite, and a slice matches"""
    c = K.small(K.C1, 512)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    lam = _lam(c)
    rxe, txe = _ula(4, lam / 2), _upa(4, 4, lam / 2)
    nl, nt, dt, l_min = 1 << 14, 16, 1e-4, -100
    got = tr.array_taps(rxe, txe, FS, nl, l_min=l_min, dt=dt, num_times=nt)
    assert tuple(got.shape) == (1, 1, 4, 16, 2, nt, nl)
    h = got.cpu().numpy()
    assert np.isfinite(h.view(np.float32)).all()
    ks, ms = np.arange(0, nl, 997), np.arange(0, nt, 5)
    sub = np.ascontiguousarray(h[:, :, :, :, :, ms][..., ks])
    ref, S = _reference_lt(tr, FS, l_min + ks, ms * dt, rxe, txe)
    tr.close()
    _check(sub, ref, S)
