"""Channel frequency responses formed on the device (Tracer.channel, hrt_channel, hermespy_rt.compute_channel)
against float64 numpy sums over the same float inputs:

    H[rx, tx, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)),  f_k = f0 + k df, t_m = t0 + m dt.

Tolerance per (rx, tx, pol), over all (m, k): |H - H64| <= 1e-5 * sum_p |a_p^pol|."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi
from oracle import oracle

from . import configs as K
from . import scenes_gen as G
from .pathsum_util import DF, _cfg, _grid, _tracer

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _phase_sum(H, S, rx, tx, a_te, a_tm, tau, nu, f, t, chunk=1024):
    """H[rx, tx] += float64 sums of the given paths (float32 inputs), S[rx, tx] += sum |a|"""
    for i in range(0, tau.size, chunk):
        ta, nv = tau[i:i + chunk].astype(np.float64), nu[i:i + chunk].astype(np.float64)
        ph = nv[:, None, None] * t[None, :, None] - f[None, None, :] * ta[:, None, None]
        e = np.exp(2j * np.pi * (ph - np.rint(ph)))
        H[rx, tx, 0] += np.tensordot(a_te[i:i + chunk].astype(np.complex128), e, axes=1)
        H[rx, tx, 1] += np.tensordot(a_tm[i:i + chunk].astype(np.complex128), e, axes=1)
    S[rx, tx, 0] += np.abs(a_te.astype(np.complex128)).sum()
    S[rx, tx, 1] += np.abs(a_tm.astype(np.complex128)).sum()


def _los_sum(H, S, los, f, t):
    nrx, ntx = los.shape[:2]
    for rx in range(nrx):
        for tx in range(ntx):
            L = los[rx, tx]
            status = int(L[0:1].view(np.uint32)[0])
            if status == 0:
                a, tau, nu = 1.0, 0.0, 0.0
            elif status == 2:
                a, tau, nu = float(L[1]), float(L[2]), float(L[6])
            else:
                continue
            ph = nu * t[:, None] - f[None, :] * tau
            H[rx, tx, :] += a * np.exp(2j * np.pi * (ph - np.rint(ph)))
            S[rx, tx, :] += abs(a)


def _reference(tr, f0, nk, t0=0.0, dt=0.0, nt=1, los=True, scatter=True):
    """float64 channel from Tracer.paths(nonzero_only=False) + Tracer.los() (both bit-equal to the oracle)"""
    f = f0 + np.arange(nk, dtype=np.float64) * DF
    t = t0 + np.arange(nt, dtype=np.float64) * dt
    H = np.zeros((tr.nrx, tr.ntx, 2, nt, nk), np.complex128)
    S = np.zeros((tr.nrx, tr.ntx, 2))
    if scatter:
        P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
        ub = P["unblocked"]
        assert not np.any(P["a_te"][~ub]) and not np.any(P["a_tm"][~ub])   # blocked records: exact zeros
        for rx in range(tr.nrx):
            for tx in range(tr.ntx):
                s = (P["rx"] == rx) & (P["tx"] == tx) & ub
                _phase_sum(H, S, rx, tx, P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s], f, t)
    if los and tr.shard.rank == 0:
        _los_sum(H, S, tr.los(), f, t)
    return H, S


def _check(got, H, S):
    got = np.asarray(got)
    assert got.shape == H.shape and got.dtype == np.complex64
    assert np.isfinite(got.view(np.float32)).all()
    err = np.abs(got.astype(np.complex128) - H).reshape(H.shape[0], H.shape[1], 2, -1).max(axis=-1)
    bound = 1e-5 * S + 1e-30
    assert (err <= bound).all(), (err / np.maximum(S, 1e-30)).max()


CASES = [
    ("C1", None, 1, [1, 7, 1000, 4096]),
    ("C3", 20000, 1, [7, 1000]),
    ("C4_DOPPLER", 4000, 4, [1, 1000]),
    ("TEST_PY", None, 1, [7, 4096]),
    ("COINCIDENT", 8000, 1, [1000]),
    ("IN_PLANE_canyon", None, 1, [7, 1000]),
]


@pytest.mark.parametrize("name,n,nt,ks", CASES, ids=[c[0] for c in CASES])
def test_channel_matches_numpy_over_paths(name, n, nt, ks):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    dt = 1e-3 if nt > 1 else 0.0
    for nk in ks:
        f0 = _grid(c, nk)
        got = tr.channel(f0, DF, nk, t0=0.0, dt=dt, num_times=nt).cpu().numpy()
        H, S = _reference(tr, f0, nk, 0.0, dt, nt)
        _check(got, H, S)
    tr.close()


@pytest.mark.parametrize("name,n", [("C1", None), ("C3", 20000), ("TEST_PY", None)])
def test_scatter_matches_dense_oracle(name, n):
    """single TX: the scatter part against the oracle's dense arrays (written, unblocked slots)"""
    c = _cfg(name, n)
    ref = oracle.compute_paths(*K.args(c))
    sc = ref["scat"]
    ub = abi.written(sc["directions_rx"][..., 0])
    tr = _tracer(c)
    tr.trace()
    nk = 257
    f0 = _grid(c, nk)
    got = tr.channel(f0, DF, nk, los=False).cpu().numpy()
    f = f0 + np.arange(nk) * DF
    t = np.zeros(1)
    H = np.zeros(got.shape, np.complex128)
    S = np.zeros(got.shape[:3])
    for rx in range(tr.nrx):
        s = ub[rx, 0]
        a_te = sc["a_te_re"][rx, 0][s] + 1j * sc["a_te_im"][rx, 0][s].astype(np.float64)
        a_tm = sc["a_tm_re"][rx, 0][s] + 1j * sc["a_tm_im"][rx, 0][s].astype(np.float64)
        _phase_sum(H, S, rx, 0, a_te, a_tm, sc["tau"][rx, 0][s], sc["freq_shift"][rx, 0][s], f, t)
    _check(got, H, S)
    tr.close()


def test_parts_add_up_and_los_closed_form():
    c = K.small(K.C4_DOPPLER, 3000)
    tr = _tracer(c)
    tr.trace()
    nk, nt, dt = 100, 3, 2e-3
    f0 = _grid(c, nk)
    both = tr.channel(f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    los = tr.channel(f0, DF, nk, dt=dt, num_times=nt, scatter=False).cpu().numpy()
    scat = tr.channel(f0, DF, nk, dt=dt, num_times=nt, los=False).cpu().numpy()
    H, S = _reference(tr, f0, nk, 0.0, dt, nt)
    _check(los + scat, H, S)
    HL, SL = _reference(tr, f0, nk, 0.0, dt, nt, scatter=False)
    _check(los, HL, SL)
    assert np.array_equal(los[:, :, 0], los[:, :, 1])   # TE = TM for LoS
    np.testing.assert_allclose(both, los + scat, rtol=0, atol=1e-5 * S.max())
    tr.close()


def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nk, f0 = 300, _grid(c, 300)
    tr = _tracer(c)
    tr.trace()
    whole = tr.channel(f0, DF, nk)
    again = tr.channel(f0, DF, nk)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.channel(f0, DF, nk, out=out, accumulate=True)
    tr.channel(f0, DF, nk, out=out, accumulate=True)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    H, S = _reference(tr, f0, nk)
    w = whole.cpu().numpy()
    _check(w, H, S)
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.channel(f0, DF, nk, out=acc, accumulate=acc is not None)
            ts.close()
        # LoS counted once: the sum of the shards is the whole channel
        _check(acc.cpu().numpy(), H, S)


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
H = hermespy_rt.compute_channel(c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
                                np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"],
                                len(c["rx_pos"]), len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {f0!r}, {df!r},
                                {nk})
np.save(sys.argv[1], H)
st = lib.Stats()
H2 = abi.run_compute_channel(lib.load(), *K.args(c), abi.channel_spec({f0!r}, {df!r}, {nk}), stats=st)
assert np.array_equal(H.view(np.float32), H2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_channel_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C) agrees with Tracer.channel on C3 at 20 k rays, also when a small
    workspace budget cuts the call into several batches"""
    c = K.small(K.C3, 20000)
    nk = 1024
    f0 = _grid(c, nk)
    tr = _tracer(c)
    tr.trace()
    want = tr.channel(f0, DF, nk).cpu().numpy()
    H, S = _reference(tr, f0, nk)
    _check(want, H, S)
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    out = tmp_path / "h.npy"
    p = subprocess.run([sys.executable, "-c", _PYBIND_CALL.format(repo=REPO, f0=f0, df=DF, nk=nk), str(out)],
                       env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = np.load(out)
    _check(got, H, S)
    assert np.abs(got.astype(np.complex128) - want).max() <= 2e-5 * S.max()


def test_generated_scene_resorted_two_tx(tmp_path):
    """> 1 024 triangles: the live list is re-sorted between bounces.  The kernel finds the TX segments of a hit
    block by binary search, so the blocks must stay TX-major -- pinned here -- and the channel must match."""
    import torch
    p = str(tmp_path / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
              tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    tr = _tracer(c)
    assert tr.num_tri > 1024
    tr.trace()
    counts = tr.counts()
    for b in range(tr.nb):
        n = int(counts[b + 1])
        if n:
            tx = (tr.hits(b, n)["ray"].to(torch.int64) & 0xFFFFFFFF) // tr.num_local
            assert bool((tx[1:] >= tx[:-1]).all()), "hit block %d is not TX-major" % b
    nk = 333
    f0 = _grid(c, nk)
    got = tr.channel(f0, DF, nk, dt=1e-3, num_times=2).cpu().numpy()
    H, S = _reference(tr, f0, nk, 0.0, 1e-3, 2)
    _check(got, H, S)
    tr.close()


def test_eight_by_eight_at_the_largest_grid():
    """C5 endpoints (8 TX x 8 RX), few rays, num_freqs * num_times = 2^20 (the largest accepted)"""
    c = K.small(K.C5, 256)
    c["num_bounces"] = 2
    tr = _tracer(c)
    tr.trace()
    nk, nt = 1 << 16, 16
    f0 = _grid(c, nk)
    got = tr.channel(f0, DF, nk, dt=1e-3, num_times=nt)
    assert tuple(got.shape) == (8, 8, 2, nt, nk)
    # check a slice of the grid (the whole float64 reference would be 2^20 points x every path)
    sub = got[:, :, :, ::5, ::997].cpu().numpy()
    f = f0 + np.arange(0, nk, 997) * DF
    t = np.arange(0, nt, 5) * 1e-3
    H = np.zeros(sub.shape, np.complex128)
    S = np.zeros(sub.shape[:3])
    P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=True).items()}
    for rx in range(8):
        for tx in range(8):
            s = (P["rx"] == rx) & (P["tx"] == tx)
            _phase_sum(H, S, rx, tx, P["a_te"][s], P["a_tm"][s], P["tau"][s], P["freq_shift"][s], f, t)
    _los_sum(H, S, tr.los(), f, t)
    _check(sub, H, S)
    tr.close()


def test_scratch_too_small_is_refused():
    import ctypes as C
    import torch
    c = K.small(K.C1, 2000)
    tr = _tracer(c)
    tr.trace()
    spec = abi.channel_spec(3e9, DF, 64)
    need = C.c_uint64(0)
    assert tr.L.hrt_channel_scratch_bytes(tr.problem, C.byref(tr.shard), C.byref(spec), C.byref(need)) == 0
    scratch = torch.empty(int(need.value), dtype=torch.uint8, device=tr.device)
    out = torch.empty((1, 1, 2, 1, 64), dtype=torch.complex64, device=tr.device)
    rc = tr.L.hrt_channel(tr.problem, C.byref(tr.shard), C.c_void_p(tr.ws.data_ptr()), C.byref(spec),
                          C.c_void_p(scratch.data_ptr()), C.c_uint64(int(need.value) - 1), C.c_void_p(out.data_ptr()),
                          0, None)
    assert rc == -1 and b"scratch" in tr.L.hrt_last_error()
    tr.close()
