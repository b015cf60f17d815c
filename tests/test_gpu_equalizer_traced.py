"""The per-point equalizers of traced channels (Tracer.channel_equalizer, Tracer.equalizer,
hrt_compute_channel_equalizer, hermespy_rt.compute_channel_equalizer) on the smallest test scene, with 4 x 2 and 8 x 8
elements, 2 times x 8 frequencies: the composition with array_channel to the bit, the drop-in entries, the SINR against
the one read from Tracer.svd under the sum of both families' bounds, and antenna patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import equalize
from hermespy_rt_amd import patterns as P

from . import configs as K
from . import equalizer_util as U
from . import patterns_util as PU
from . import svd_util as SU
from .pathsum_util import DF, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DT = 8, 2, 1e-3
CONFIG = K.small(K.C1, 2000)


def _geometries(c):
    """(Nr, Nt) = (4, 2): g = 1;  (8, 8): g = 4"""
    lam = _lam(c)
    return [(_ula(4, lam / 2), _ula(2, lam / 2, axis=0)), (_upa(2, 4, lam / 2), _ula(8, lam / 2, axis=0))]


@pytest.fixture(scope="module")
def traced():
    tr = _tracer(CONFIG)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIG
    tr.close()


def _noise(H):
    """a quarter of the largest |H|_F^2 of any point: the factored matrix [H; sqrt(N0) I] of every point then has
    kappa^2 = (sigma_0^2 + N0) / N0 <= 5"""
    return float((H.abs() ** 2).sum((2, 3)).max()) / 4


def test_channel_equalizer_is_equalizer_of_array_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        n0 = _noise(H)
        assert n0 > 0
        for kind in ("lmmse", "zf"):
            for weights in (True, False):
                a = tr.equalizer(H, n0, kind, weights)
                b = tr.channel_equalizer(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0, kind=kind,
                                         weights=weights)
                assert torch.equal(a["buffer"], b["buffer"])
                assert (a["W"] is None) == (not weights) and (b["W"] is None) == (not weights)
        nr, nt = rxe.shape[0], txe.shape[0]
        assert a["sinr"].shape == (tr.nrx, tr.ntx, nt, 2, NT, NK) and a["status"].shape == (tr.nrx, tr.ntx, 2, NT, NK)
        assert b["buffer"].numel() == tr.nrx * tr.ntx * 2 * NT * NK * (nt * 4 + 4)
        lm = tr.equalizer(H, n0, "lmmse")
        assert not lm["status"].any() and float(lm["sinr"].max()) > 0 and lm["W"].shape[2:4] == (nt, nr)


def test_sinr_agrees_with_the_svd_family(traced):
    """sinr against equalize.sinr_from_svd(Tracer.svd(H)) and against the float64 reference.  The equalizer's bound
    is TOL_SINR u kappa (1 + rho) (tests/equalizer_util.py).  The SVD's: its results are the exact decomposition of a
    matrix within E = TOL_CONST u_svd |H|_F of H with vectors orthonormal within TOL_CONST u_svd (tests/svd_util.py);
    dG = -G (E^H H + H^H E) G gives |dG_ii| / G_ii <= 2 |H|_F sigma_0 TOL_CONST u_svd (sigma_0^2 + N0) / N0^2
    <= 2 n TOL_CONST u_svd kappa^4, and the vectors' defect the same again at most: 4 n TOL_CONST u_svd kappa^4 (1 + rho)
    in all, with kappa^2 = (sigma_0^2 + N0) / N0 the squared condition number of [H; sqrt(N0) I]."""
    tr, c = traced
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        nr, nt = rxe.shape[0], txe.shape[0]
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        n0 = _noise(H)
        eq = tr.equalizer(H, n0, "lmmse")
        sv = tr.svd(H)
        Hn = H.cpu().numpy()
        ref = equalize.equalizer_reference(Hn, np.float32(n0), "lmmse")
        assert not ref["status"].any() and not eq["status"].cpu().numpy().any()
        assert ref["cond"].max() ** 2 <= 5.01
        rho = ref["sinr"]
        kappa = ref["cond"][:, :, None]
        got = eq["sinr"].cpu().numpy().astype(np.float64)
        b_eq = U.TOL_SINR * U.unit_roundoff(nr, nt) * kappa * (1 + rho)
        assert (np.abs(got - rho) <= b_eq).all(), (np.abs(got - rho) / b_eq).max()
        from_svd = equalize.sinr_from_svd(sv["sigma"].cpu().numpy(), sv["v"].cpu().numpy(), np.float32(n0), "lmmse")
        b_svd = 4 * min(nr, nt) * SU.TOL_CONST * SU.unit_roundoff(nr, nt) * kappa ** 4 * (1 + rho)
        err = np.abs(got - from_svd)
        print("%dx%d: sinr <= %.3g, |eq - ref| / bound <= %.3g, |eq - svd| / bound <= %.3g"
              % (nr, nt, rho.max(), (np.abs(got - rho) / b_eq).max(), (err / (b_eq + b_svd)).max()))
        assert (err <= b_eq + b_svd).all()
        assert rho.max() > 0.1                       # (the check is not about zeros)


def test_patterns_weigh_the_equalized_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[0]
    plain_H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
    n0 = _noise(plain_H)
    plain = tr.channel_equalizer(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)["buffer"].clone()
    rx, tx = P.tr38901(1.0), PU.pattern_set()["table_7x12"]
    tr.set_patterns(rx, tx, PU.random_rotations(tr.nrx, 61), PU.random_rotations(tr.ntx, 62))
    try:
        tr.trace()
        assert tr.patterned
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        assert not torch.equal(H, plain_H)
        got = tr.channel_equalizer(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)
        assert torch.equal(got["buffer"], tr.equalizer(H, n0)["buffer"])
        assert not torch.equal(got["buffer"], plain)
    finally:
        tr.set_patterns()
        tr.trace()
    assert torch.equal(tr.channel_equalizer(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)["buffer"], plain)


_DROP_IN_CALL = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import torch  # noqa: F401
import hermespy_rt_amd
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from hermespy_rt_amd import patterns as P
from tests import configs as K
from tests import patterns_util as PU
c = K.small(K.C1, 2000)
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
nrx, ntx = len(c["rx_pos"]), len(c["tx_pos"])
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
        c["num_bounces"], {f0!r}, {df!r}, {nk}, rxe, txe)
kw = dict(dt={dt!r}, num_times={nt})
H = hermespy_rt.compute_array_channel(*args, **kw)
n0 = float(np.float32((np.abs(H) ** 2).sum((2, 3)).max() / 4))
spec = abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt})
bufs = []
for kind in ("lmmse", "zf"):
    r = hermespy_rt.compute_channel_equalizer(*args, n0, kind, **kw)
    r2 = abi.run_compute_channel_equalizer(lib.load(), *K.args(c), spec, rxe, txe, n0, kind)
    assert np.array_equal(r["buffer"], r2["buffer"])
    for k in ("W", "sinr", "status"):
        assert r[k].shape == r2[k].shape and r[k].dtype == r2[k].dtype and np.array_equal(r[k], r2[k]), k
    s = hermespy_rt.compute_channel_equalizer(*args, n0, kind, weights=False, **kw)
    assert s["W"] is None and np.array_equal(s["sinr"], r["sinr"]) and np.array_equal(s["status"], r["status"])
    bufs.append(r["buffer"])
pat = dict(rx=P.tr38901(1.0), tx=PU.pattern_set()["table_7x12"], rx_orientation=PU.random_rotations(nrx, 61),
           tx_orientation=PU.random_rotations(ntx, 62))
Hp = hermespy_rt.compute_array_channel(*args, patterns=pat, **kw)
rp = hermespy_rt.compute_channel_equalizer(*args, n0, "lmmse", patterns=pat, **kw)
assert not np.array_equal(Hp, H) and not np.array_equal(rp["buffer"], bufs[0])
again = hermespy_rt.compute_channel_equalizer(*args, n0, "lmmse", **kw)      # the setting is gone after the call
assert np.array_equal(again["buffer"], bufs[0])
np.save(sys.argv[1], H)
np.save(sys.argv[4], bufs[0])
np.save(sys.argv[5], bufs[1])
np.save(sys.argv[6], Hp)
np.save(sys.argv[7], rp["buffer"])
np.save(sys.argv[8], np.float32(n0))
"""


def test_drop_in_entries_equalize_their_own_channel(tmp_path):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return, to the bit, what
    Tracer.equalizer gives for the H that compute_array_channel returns for the same call, with and without patterns"""
    c = CONFIG
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[1]
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "lmmse.npy", "zf.npy", "hp.npy", "lmmse_p.npy",
                                    "n0.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DT, nt=NT)] +
                       [str(x) for x in files], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    H, Hp, n0 = np.load(files[0]), np.load(files[5]), float(np.load(files[7]))
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 8, 8, 2, NT, NK) and np.abs(H).max() > 0
    tr = _tracer(K.small(K.C1, 64))
    try:
        for h, kind, f in ((H, "lmmse", files[3]), (H, "zf", files[4]), (Hp, "lmmse", files[6])):
            got = tr.equalizer(tr.torch.from_numpy(h).to(tr.device), n0, kind)["buffer"].cpu().numpy()
            buf = np.load(f)
            assert buf.dtype == np.uint8 and np.array_equal(got, buf), kind
    finally:
        tr.close()
