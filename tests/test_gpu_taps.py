"""Sampled channel impulse responses formed on the device (Tracer.taps, hrt_taps, hermespy_rt.compute_taps) against
float64 numpy sums over the same float inputs:

    h[rx, tx, pol, m, i] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) sinc(l_i - f_s tau_p),
    t_m = t0 + m dt,  l_i = l_min + i.

Tolerance per (rx, tx, pol), over all (m, i): |h - h64| <= 1e-5 * sum_p |a_p^pol|."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import scenes_gen as G
from .pathsum_util import FS, _cfg, _los_status, _tracer

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _taps_sum(h, S, rx, tx, a_te, a_tm, tau, nu, fs, fc, l, t, chunk=2048):
    """h[rx, tx] += float64 sums of the given paths (float32 inputs), S[rx, tx] += sum |a|"""
    for i in range(0, tau.size, chunk):
        ta, nv = tau[i:i + chunk].astype(np.float64), nu[i:i + chunk].astype(np.float64)
        ph = nv[:, None] * t[None, :] - fc * ta[:, None]
        e = np.exp(2j * np.pi * (ph - np.rint(ph)))          # [p, m]
        v = np.sinc(l[None, :] - fs * ta[:, None])            # [p, i]
        for pol, a in enumerate((a_te, a_tm)):
            u = a[i:i + chunk].astype(np.complex128)[:, None] * e
            h[rx, tx, pol] += u.T @ v
    S[rx, tx, 0] += np.abs(a_te.astype(np.complex128)).sum()
    S[rx, tx, 1] += np.abs(a_tm.astype(np.complex128)).sum()


def _los_sum(h, S, los, fs, fc, l, t):
    nrx, ntx = los.shape[:2]
    for rx in range(nrx):
        for tx in range(ntx):
            L = los[rx, tx]
            status = _los_status(L)
            if status == 0:
                a, tau, nu = 1.0, 0.0, 0.0
            elif status == 2:
                a, tau, nu = float(L[1]), float(L[2]), float(L[6])
            else:
                continue
            ph = nu * t - fc * tau
            e = a * np.exp(2j * np.pi * (ph - np.rint(ph)))
            h[rx, tx, :] += e[:, None] * np.sinc(l - fs * tau)[None, :]
            S[rx, tx, :] += abs(a)


def _reference(tr, fs, nl, l_min=0, fc=None, t0=0.0, dt=0.0, nt=1, los=True, scatter=True):
    """float64 taps from Tracer.paths(nonzero_only=False) + Tracer.los()"""
    fc = tr.f_ghz * 1e9 if fc is None else fc
    l = l_min + np.arange(nl, dtype=np.float64)
    t = t0 + np.arange(nt, dtype=np.float64) * dt
    h = np.zeros((tr.nrx, tr.ntx, 2, nt, nl), np.complex128)
    S = np.zeros((tr.nrx, tr.ntx, 2))
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
        ub = P["unblocked"]
        assert not np.any(P["a_te"][~ub]) and not np.any(P["a_tm"][~ub])   # blocked records: exact zeros
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                s = (P["rx"] == rx) & (P["tx"] == tx) & ub
                _taps_sum(h, S, rx, tx, P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s], fs, fc, l, t)
    if los and tr.shard.rank == 0:
        _los_sum(h, S, tr.los(), fs, fc, l, t)
    return h, S


def _check(got, h, S):
    got = np.asarray(got)
    assert got.shape == h.shape and got.dtype == np.complex64
    assert np.isfinite(got.view(np.float32)).all()
    err = np.abs(got.astype(np.complex128) - h).reshape(h.shape[0], h.shape[1], 2, -1).max(axis=-1)
    bound = 1e-5 * S + 1e-30
    assert (err <= bound).all(), (err / np.maximum(S, 1e-30)).max()


# (scene, rays, [(num_times, num_taps, l_min, fs)])
CASES = [
    ("C1", None, [(1, 64, 0, FS), (3, 300, -7, 1e9)]),
    ("TEST_PY", None, [(1, 300, -7, 1e9), (3, 1, 0, FS)]),
    ("COINCIDENT", 8000, [(1, 64, -7, FS), (3, 300, 0, 1e9)]),
    ("C3", 20000, [(1, 300, 0, FS), (3, 64, -7, 1e9), (1, 1, 0, FS)]),
    ("C4_DOPPLER", 4000, [(3, 64, 0, FS), (1, 300, -7, 1e9)]),
    ("IN_PLANE_canyon", None, [(1, 300, -7, FS), (3, 64, 0, 1e9)]),
]


@pytest.mark.parametrize("name,n,grids", CASES, ids=[c[0] for c in CASES])
def test_taps_match_numpy_over_paths(name, n, grids):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    for nt, nl, l_min, fs in grids:
        dt = 1e-4 if nt > 1 else 0.0
        got = tr.taps(fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
        h, S = _reference(tr, fs, nl, l_min, dt=dt, nt=nt)
        _check(got, h, S)
    tr.close()


def _clear_los_link(c):
    """c cut down to its first (rx, tx) whose LoS is clear"""
    tr = _tracer(c)
    tr.trace()
    los = tr.los()
    tr.close()
    rx, tx = next((r, t) for r in range(los.shape[0]) for t in range(los.shape[1]) if _los_status(los[r, t]) == 2)
    d = dict(c)
    for k, j in (("rx_pos", rx), ("rx_vel", rx), ("tx_pos", tx), ("tx_vel", tx)):
        d[k] = [[float(v) for v in c[k][j]]]
    return d


def test_los_closed_form_at_an_integer_delay():
    """parts = LoS only, t0 = 0, f_s with f_s tau_LoS exactly an integer n in double: a e^{-j 2 pi f_c tau} at tap n
    (the branch where l - x is exactly 0), zero elsewhere; LoS + scatter add up to both"""
    c = _clear_los_link(K.small(K.C4_DOPPLER, 3000))
    tr = _tracer(c)
    tr.trace()
    L = tr.los()[0, 0]
    assert _los_status(L) == 2
    a, tau = float(L[1]), float(L[2])
    n = 41
    fs = n / tau
    while fs * tau != n:   # the f_s next to n / tau whose product with tau rounds to n exactly
        fs = np.nextafter(fs, math.inf if fs * tau < n else 0.0)
    fc = tr.f_ghz * 1e9
    nl, l_min = 128, -5
    got = tr.taps(fs, nl, l_min=l_min, scatter=False).cpu().numpy()
    want = a * np.exp(-2j * np.pi * ((fc * tau) - np.rint(fc * tau)))
    i = n - l_min
    for pol in range(2):
        assert abs(complex(got[0, 0, pol, 0, i]) - want) <= 1e-6 * abs(a)
        rest = np.delete(got[0, 0, pol, 0], i)
        assert np.abs(rest).max() <= 1e-6 * abs(a)
    # LoS + scatter = both, and both match the float64 sum
    nt, dt = 3, 2e-4
    both = tr.taps(fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
    los = tr.taps(fs, nl, l_min=l_min, dt=dt, num_times=nt, scatter=False).cpu().numpy()
    scat = tr.taps(fs, nl, l_min=l_min, dt=dt, num_times=nt, los=False).cpu().numpy()
    h, S = _reference(tr, fs, nl, l_min, dt=dt, nt=nt)
    _check(both, h, S)
    _check(los + scat, h, S)
    hl, sl = _reference(tr, fs, nl, l_min, dt=dt, nt=nt, scatter=False)
    _check(los, hl, sl)
    assert np.array_equal(los[:, :, 0], los[:, :, 1])   # TE = TM for LoS
    tr.close()


@pytest.mark.parametrize("nt", [1, 2])
def test_dtft_of_the_taps_is_the_channel(nt):
    """single TX, every delay at least M taps inside the window: the DTFT of the taps at |f| <= f_s / 4 is
    Tracer.channel at f_c + f.  This pins the signs of f_c, nu and tau."""
    c = K.small(K.C3_DOPPLER, 20000)
    tr = _tracer(c)
    assert tr.ntx == 1
    tr.trace()
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
    h = tr.taps(fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy().astype(np.complex128)
    nk = 33
    f = -fs / 4 + np.arange(nk) * (fs / 2 / (nk - 1))
    H = tr.channel(fc - fs / 4, fs / 2 / (nk - 1), nk, dt=dt, num_times=nt).cpu().numpy()
    l = l_min + np.arange(nl, dtype=np.float64)
    E = np.exp(-2j * np.pi * np.outer(l, f) / fs)   # [i, k]
    dtft = h @ E
    # the sinc tails cut at M taps: by Abel summation each side is at most 2 / (pi (M - 1) |1 - e^{j theta}|), with
    # |1 - e^{j theta}| >= sqrt(2) for |f| <= f_s / 4; plus the float error of both sides
    _, S = _reference(tr, fs, 1, 0, dt=dt, nt=1)
    tol = (2 * math.sqrt(2) / (math.pi * (M - 1)) + 1e-5) * S
    assert tol.max() <= 2e-3 * S.max()
    err = np.abs(dtft - H).reshape(tr.nrx, 1, 2, -1).max(axis=-1)
    assert (err <= tol).all(), (err / S).max()
    tr.close()


def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nl, l_min, nt, dt = 200, -3, 2, 1e-4
    tr = _tracer(c)
    tr.trace()
    whole = tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt)
    again = tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt, out=out, accumulate=True)
    tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt, out=out, accumulate=True)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    h, S = _reference(tr, FS, nl, l_min, dt=dt, nt=nt)
    _check(whole.cpu().numpy(), h, S)
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt, out=acc, accumulate=acc is not None)
            ts.close()
        # LoS counted once: the sum of the shards is the whole result
        _check(acc.cpu().numpy(), h, S)


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
h = hermespy_rt.compute_taps(c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
                             np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"],
                             len(c["rx_pos"]), len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {fs!r}, {nl},
                             l_min={l_min}, dt={dt!r}, num_times={nt})
np.save(sys.argv[1], h)
st = lib.Stats()
spec = abi.taps_spec({fs!r}, {nl}, {l_min}, c["f_ghz"] * 1e9, 0.0, {dt!r}, {nt})
h2 = abi.run_compute_taps(lib.load(), *K.args(c), spec, stats=st)
assert np.array_equal(h.view(np.float32), h2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_taps_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C) agrees with Tracer.taps on C3 at 20 k rays, also when a small workspace budget
    cuts the call into several batches"""
    c = K.small(K.C3, 20000)
    nl, l_min, nt, dt = 256, -7, 2, 1e-4
    tr = _tracer(c)
    tr.trace()
    want = tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
    h, S = _reference(tr, FS, nl, l_min, dt=dt, nt=nt)
    _check(want, h, S)
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    out = tmp_path / "h.npy"
    code = _PYBIND_CALL.format(repo=REPO, fs=FS, nl=nl, l_min=l_min, dt=dt, nt=nt)
    p = subprocess.run([sys.executable, "-c", code, str(out)], env=env, capture_output=True, text=True, timeout=900)
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
    nl, nt, dt = 150, 3, 1e-3
    got = tr.taps(FS, nl, l_min=-2, dt=dt, num_times=nt).cpu().numpy()
    h, S = _reference(tr, FS, nl, -2, dt=dt, nt=nt)
    _check(got, h, S)
    tr.close()


def test_eight_by_eight_at_the_largest_grid():
    """C5 endpoints (8 TX x 8 RX), few rays, num_taps * num_times = 2^20 (the largest accepted)"""
    c = K.small(K.C5, 256)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    nl, nt, dt, l_min = 1 << 14, 64, 1e-4, -100
    got = tr.taps(FS, nl, l_min=l_min, dt=dt, num_times=nt)
    assert tuple(got.shape) == (8, 8, 2, nt, nl)
    # check a slice of the grid (the whole float64 reference would be 2^20 points x every path)
    ms, iss = np.arange(0, nt, 7), np.arange(0, nl, 61)
    sub = got[:, :, :, ::7, ::61].cpu().numpy()
    fc = tr.f_ghz * 1e9
    l = l_min + iss.astype(np.float64)
    t = ms * dt
    h = np.zeros(sub.shape, np.complex128)
    S = np.zeros(sub.shape[:3])
    P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=True).items()}
    for rx in range(8):
        for tx in range(8):
            s = (P["rx"] == rx) & (P["tx"] == tx)
            _taps_sum(h, S, rx, tx, P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s], FS, fc, l, t)
    _los_sum(h, S, tr.los(), FS, fc, l, t)
    _check(sub, h, S)
    tr.close()


def test_scratch_too_small_is_refused():
    import torch
    c = K.small(K.C1, 2000)
    tr = _tracer(c)
    tr.trace()
    spec = abi.taps_spec(FS, 64, 0, 3e9)
    need = C.c_uint64(0)
    assert tr.L.hrt_taps_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty((1, 1, 2, 1, 64), dtype=torch.complex64, device=tr.device)
    rc = tr.L.hrt_taps(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec),
                       C.c_void_p(scratch.data_ptr()), C.c_uint64(int(need.value) - 1), C.c_void_p(out.data_ptr()),
                       0, None)
    assert rc == -1 and b"scratch" in tr.L.hrt_last_error()
    tr.close()
