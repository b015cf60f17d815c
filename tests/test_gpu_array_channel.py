"""Antenna-array channel responses formed on the device (Tracer.array_channel, hrt_array_channel,
hermespy_rt.compute_array_channel) against float64 numpy sums over the same float inputs:

    H[rx, tx, i, j, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) exp(j 2 pi f_a (r_i . u_rx + q_j . u_tx) / c)

u_rx: Tracer.paths()' direction_rx (LoS: -HRT_LOS_DIR); u_tx: hrt_launch_dirs_host of the record's global path
(LoS: HRT_LOS_DIR).  Tolerance per (link, i, j, pol), over all (m, k): |H - H64| <= 1e-5 * sum_p |a_p^pol|."""
import os
import subprocess
import sys

import numpy as np
import pytest

from . import configs as K
from . import scenes_gen as G
from . import planted as PL
from .pathsum_util import ARRAY_CASES as CASES
from .pathsum_util import C0, DF, _cfg, _geometries, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sum(H, S, link, a_te, a_tm, tau, nu, urx, utx, rxe, txe, fa, f, t, chunk=512):
    """H[link] += float64 sums over the given paths, S[link] += sum |a| (per pol)"""
    rxe, txe = rxe.astype(np.float64), txe.astype(np.float64)
    nr, nt = rxe.shape[0], txe.shape[0]
    for i in range(0, tau.size, chunk):
        ta, nv = tau[i:i + chunk].astype(np.float64), nu[i:i + chunk].astype(np.float64)
        ph = nv[:, None, None] * t[None, :, None] - f[None, None, :] * ta[:, None, None]
        e = np.exp(2j * np.pi * (ph - np.rint(ph))).reshape(ta.size, -1)
        st = (fa / C0) * ((urx[i:i + chunk].astype(np.float64) @ rxe.T)[:, :, None] +
                          (utx[i:i + chunk].astype(np.float64) @ txe.T)[:, None, :])
        s = np.exp(2j * np.pi * (st - np.rint(st))).reshape(ta.size, nr * nt)
        for pol, a in enumerate((a_te, a_tm)):
            w = a[i:i + chunk].astype(np.complex128)[:, None] * e
            H[link][:, :, pol] += (s.T @ w).reshape(nr, nt, *H.shape[-2:])
    S[link][0] += np.abs(a_te.astype(np.complex128)).sum()
    S[link][1] += np.abs(a_tm.astype(np.complex128)).sum()


def _reference_ft(tr, f, t, rxe, txe, fa, los=True, scatter=True):
    """float64 array channel on the frequencies f and times t, from Tracer.paths() + Tracer.los()"""
    H = np.zeros((tr.nrx, tr.ntx, rxe.shape[0], txe.shape[0], 2, t.size, f.size), np.complex128)
    S = np.zeros((tr.nrx, tr.ntx, 2))
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
        ub = P["unblocked"]
        dirs = PL.launch_dirs(tr).astype(np.float32)
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                s = (P["rx"] == rx) & (P["tx"] == tx) & ub
                _sum(H, S, (rx, tx), P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s],
                     P["direction_rx"][s], dirs[P["path"][s]], rxe, txe, fa, f, t)
    if los and tr.shard.rank == 0:
        L = tr.los()
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                q = L[rx, tx]
                status = int(q[0:1].view(np.uint32)[0])
                if status == 0:   # coincident: directions_tx = (-1, 0, 0), directions_rx = (1, 0, 0)
                    a, tau, nu, u = 1.0, 0.0, 0.0, np.array([-1.0, 0.0, 0.0], np.float32)
                elif status == 2:   # HRT_LOS_DIR is directions_tx
                    a, tau, nu, u = float(q[1]), float(q[2]), float(q[6]), q[3:6].copy()
                else:
                    continue
                one = np.array([a], np.float32)
                _sum(H, S, (rx, tx), one, one, np.array([tau], np.float32), np.array([nu], np.float32),
                     -u[None, :], u[None, :], rxe, txe, fa, f, t)
    return H, S


def _reference(tr, f0, nk, rxe, txe, fa, t0=0.0, dt=0.0, nt=1, los=True, scatter=True):
    f = f0 + np.arange(nk, dtype=np.float64) * DF
    t = t0 + np.arange(nt, dtype=np.float64) * dt
    return _reference_ft(tr, f, t, rxe, txe, fa, los, scatter)


def _check(got, H, S):
    got = np.asarray(got)
    assert got.shape == H.shape and got.dtype == np.complex64
    assert np.isfinite(got.view(np.float32)).all()
    err = np.abs(got.astype(np.complex128) - H).reshape(*H.shape[:5], -1).max(axis=-1)   # (rx, tx, i, j, pol)
    bound = 1e-5 * S[:, :, None, None, :] + 1e-30
    assert (err <= bound).all(), (err / np.maximum(S[:, :, None, None, :], 1e-30)).max()


@pytest.mark.parametrize("name,n,nt,nk", CASES, ids=[c[0] for c in CASES])
def test_array_channel_matches_float64(name, n, nt, nk):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    dt = 1e-3 if nt > 1 else 0.0
    f0 = _grid(c, nk)
    for _, rxe, txe in _geometries(c):
        got = tr.array_channel(rxe, txe, f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
        H, S = _reference(tr, f0, nk, rxe, txe, c["f_ghz"] * 1e9, 0.0, dt, nt)
        _check(got, H, S)
    tr.close()


@pytest.mark.parametrize("name,n", [("C3", 20000), ("C4_DOPPLER", 4000), ("COINCIDENT", 8000)])
def test_single_element_at_the_origin_is_the_channel(name, n):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    nk, nt, dt = 300, 2, 1e-3
    f0 = _grid(c, nk)
    one = np.zeros((1, 3))
    got = tr.array_channel(one, one, f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    want = tr.channel(f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    assert got.shape == (tr.nrx, tr.ntx, 1, 1, 2, nt, nk)
    H, S = _reference(tr, f0, nk, one, one, c["f_ghz"] * 1e9, 0.0, dt, nt)
    _check(got, H, S)
    bound = 1e-5 * S[:, :, None, :, None, None]
    assert (np.abs(got[:, :, 0, 0].astype(np.complex128) - want) <= 2 * bound).all()
    tr.close()


# a clear LoS of 30 m in the street canyon (TX above the cars)
SIGN_CFG = K.cfg("simple_street_canyon_with_cars.hrt", [[-10.0, 1.0, 3.0]], [[-40.0, 0.0, 5.0]], 3.5, 2000, 1)


@pytest.mark.parametrize("side", ["rx", "tx"])
def test_steering_sign_against_moved_endpoint(side):
    """LoS only, K = 1 at f0 = f_a: an element at offset r must see what a plain trace from the moved endpoint
    sees (plane-wave and amplitude errors ~5e-3 here; a flipped sign misses by ~2 |H|)"""
    c = dict(SIGN_CFG)
    tr = _tracer(c)
    tr.trace()
    L = tr.los()[0, 0]
    assert int(L[0:1].view(np.uint32)[0]) == 2 and L[2] * C0 >= 20.0
    u = L[3:6].astype(np.float64)   # TX -> RX
    across = np.cross(u, [0.0, 0.0, 1.0])
    across /= np.linalg.norm(across)
    lam = _lam(c)
    r = lam / 4 * u + lam / 2 * across
    fa = c["f_ghz"] * 1e9
    one = np.zeros((1, 3))
    if side == "rx":
        got = tr.array_channel(r[None, :], one, fa, DF, 1, scatter=False, array_frequency=fa).cpu().numpy()
    else:
        got = tr.array_channel(one, r[None, :], fa, DF, 1, scatter=False, array_frequency=fa).cpu().numpy()
    tr.close()
    moved = dict(c)
    key = side + "_pos"
    moved[key] = [list(np.asarray(c[key][0], np.float64) + r)]
    tm = _tracer(moved)
    tm.trace()
    assert int(tm.los()[0, 0][0:1].view(np.uint32)[0]) == 2
    want = tm.channel(fa, DF, 1, scatter=False).cpu().numpy()
    tm.close()
    g, w = got[0, 0, 0, 0], want[0, 0]
    assert np.abs(g - w).max() <= 1e-2 * np.abs(w).max(), (g.ravel(), w.ravel())


def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nk, f0 = 200, _grid(c, 200)
    _, rxe, txe = _geometries(c)[0]
    fa = c["f_ghz"] * 1e9
    tr = _tracer(c)
    tr.trace()
    whole = tr.array_channel(rxe, txe, f0, DF, nk)
    again = tr.array_channel(rxe, txe, f0, DF, nk)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.array_channel(rxe, txe, f0, DF, nk, out=out, accumulate=True)
    tr.array_channel(rxe, txe, f0, DF, nk, out=out, accumulate=True)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    H, S = _reference(tr, f0, nk, rxe, txe, fa)
    _check(whole.cpu().numpy(), H, S)
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.array_channel(rxe, txe, f0, DF, nk, out=acc, accumulate=acc is not None)
            ts.close()
        _check(acc.cpu().numpy(), H, S)   # LoS counted once: the shards sum to the whole channel


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
H = hermespy_rt.compute_array_channel(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                      np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                      np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
                                      len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {f0!r}, {df!r}, {nk},
                                      rxe, txe)
np.save(sys.argv[1], H)
st = lib.Stats()
H2 = abi.run_compute_array_channel(lib.load(), *K.args(c), abi.channel_spec({f0!r}, {df!r}, {nk}), rxe, txe,
                                   stats=st)
assert np.array_equal(H.view(np.float32), H2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_array_channel_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C) agrees with Tracer.array_channel on C3 at 20 k rays, also when a small
    workspace budget cuts the call into several batches"""
    c = K.small(K.C3, 20000)
    nk = 256
    f0 = _grid(c, nk)
    _, rxe, txe = _geometries(c)[0]
    tr = _tracer(c)
    tr.trace()
    want = tr.array_channel(rxe, txe, f0, DF, nk).cpu().numpy()
    H, S = _reference(tr, f0, nk, rxe, txe, c["f_ghz"] * 1e9)
    _check(want, H, S)
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    out, fr, ft = tmp_path / "h.npy", tmp_path / "rx.npy", tmp_path / "tx.npy"
    np.save(fr, rxe)
    np.save(ft, txe)
    p = subprocess.run([sys.executable, "-c", _PYBIND_CALL.format(repo=REPO, f0=f0, df=DF, nk=nk), str(out), str(fr),
                        str(ft)], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = np.load(out)
    _check(got, H, S)
    assert np.abs(got.astype(np.complex128) - want).max() <= 2e-5 * S.max()


def test_generated_scene_resorted_two_tx(tmp_path):
    """> 1 024 triangles: the live list is re-sorted between bounces; TX segments then come from the binary
    search of the segments kernel"""
    p = str(tmp_path / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
              tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    tr = _tracer(c)
    assert tr.num_tri > 1024
    tr.trace()
    nk = 77
    f0 = _grid(c, nk)
    for _, rxe, txe in _geometries(c):
        got = tr.array_channel(rxe, txe, f0, DF, nk, dt=1e-3, num_times=2).cpu().numpy()
        H, S = _reference(tr, f0, nk, rxe, txe, c["f_ghz"] * 1e9, 0.0, 1e-3, 2)
        _check(got, H, S)
    tr.close()


def test_largest_grid():
    """Nr * Nt * T * K = 2^24 (the largest accepted): 64 pairs, T * K = 2^18; finite, and a slice matches"""
    c = K.small(K.C1, 512)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    lam = _lam(c)
    rxe, txe = _ula(4, lam / 2), _upa(4, 4, lam / 2)
    nk, nt = 1 << 14, 16
    f0 = _grid(c, nk)
    got = tr.array_channel(rxe, txe, f0, DF, nk, dt=1e-3, num_times=nt)
    assert tuple(got.shape) == (1, 1, 4, 16, 2, nt, nk)
    h = got.cpu().numpy()
    assert np.isfinite(h.view(np.float32)).all()
    ks, ms = np.arange(0, nk, 997), np.arange(0, nt, 5)
    sub = np.ascontiguousarray(h[:, :, :, :, :, ms][..., ks])
    H, S = _reference_ft(tr, f0 + ks * DF, ms * 1e-3, rxe, txe, c["f_ghz"] * 1e9)
    tr.close()
    _check(sub, H, S)
