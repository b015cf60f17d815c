"""The per-point SVD of traced channels (Tracer.channel_svd, Tracer.svd, hrt_compute_channel_svd,
hermespy_rt.compute_channel_svd) on small problems: the composition with array_channel to the bit, the singular values
against float64 numpy under the derived bound, the Frobenius identity, the rank of a LoS-only channel, the SVD precoder
and combiner through beam_channel, and the drop-in entries."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import mimo

from . import beam_util as BU
from . import configs as K
from . import planted as PL
from . import svd_util as U
from .pathsum_util import DF, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DT = 24, 2, 1e-3
CONFIGS = {"C1": K.small(K.C1, 2000), "C4_DOPPLER": K.small(K.C4_DOPPLER, 4000)}


def _geometries(c):
    """(Nr, Nt) = (4, 6): wide, g = 1;  (16, 8): tall, g = 8"""
    lam = _lam(c)
    return [(_ula(4, lam / 2), _upa(2, 3, lam / 2)), (_upa(4, 4, lam / 2), _ula(8, lam / 2, axis=0))]


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def traced(request):
    tr = _tracer(CONFIGS[request.param])
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIGS[request.param]
    tr.close()


def _np(r):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}


def test_channel_svd_is_svd_of_array_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        for vectors in (True, False):
            H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
            a = tr.svd(H, vectors)
            b = tr.channel_svd(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, vectors=vectors)
            assert torch.equal(a["buffer"], b["buffer"])
            assert float(a["sigma"].max()) > 0
            assert (a["u"] is None) == (not vectors) and (b["v"] is None) == (not vectors)
        nr, nt = rxe.shape[0], txe.shape[0]
        assert a["sigma"].shape == (tr.nrx, tr.ntx, min(nr, nt), 2, NT, NK)


def test_singular_values_against_float64(traced):
    """sigma against numpy on the widened H under the bound of the planted tests, sum sigma^2 against |H|_F^2, and the
    whole of check() on the vectors"""
    tr, c = traced
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        r = _np(tr.svd(H))
        Hn = H.cpu().numpy()
        mats = U.to_batch(Hn)
        s, u, v, sw = U.to_batch_sigma(r["sigma"]), U.to_batch(r["u"]), U.to_batch(r["v"]), r["sweeps"].ravel()
        assert sw.dtype == np.int32 and (sw >= 0).all()
        worst = U.check(mats, s, u, v, sw)
        print("traced %s: measures in u: %s, sweeps <= %d" % (mats.shape[1:], " ".join("%.2f" % w for w in worst),
                                                            int(sw.max())))
        ref = mimo.svd_reference(Hn)["sigma"]
        unit = U.unit_roundoff(*mats.shape[1:])
        assert (np.abs(r["sigma"] - ref) <= U.TOL_CONST * unit * ref[:, :, :1]).all()
        fro = (np.abs(mats.astype(np.complex128)) ** 2).sum((1, 2))
        # sum sigma^2 = |H|_F^2: each sigma within TOL_CONST u sigma_0, so the sum within 2 n TOL_CONST u sigma_0^2 (+ 2nd order)
        n = s.shape[1]
        assert (np.abs((s.astype(np.float64) ** 2).sum(1) - fro) <= 2.1 * n * U.TOL_CONST * unit * fro).all()
        assert fro.max() > 0


def test_line_of_sight_only_has_rank_one(traced):
    tr, c = traced
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[1]
    r = _np(tr.channel_svd(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, scatter=False))
    rank = mimo.rank(r["sigma"], rxe.shape[0], txe.shape[0])
    status = PL.los_status(tr)                                   # 0 coincident, 1 blocked, 2 clear
    want = np.broadcast_to((status != 1).astype(np.int64).reshape(tr.nrx, tr.ntx, 1, 1, 1), rank.shape)
    assert np.array_equal(rank, want), (rank.reshape(tr.nrx, tr.ntx, -1).max(-1), status)
    assert (status != 1).any()
    # the null columns of the long side are exact zeros
    long_ = r["u"] if rxe.shape[0] >= txe.shape[0] else r["v"]
    assert not long_[:, :, :, 1:].any()


def test_svd_precoder_and_combiner_reach_sigma_0(traced):
    """beam_channel with precoder(v, 1) and combiner(u, 1) of one point is sigma_0 at that point.  Tolerance: the
    beam-channel bound 1e-5 |w_rx|_1 |w_tx|_1 sum_p |a_p| (tests/test_gpu_beam_channel.py) for the beam, the same for
    the array channel the vectors were formed from, and 4 TOL_CONST u |H|_F for the decomposition (the reconstruction
    error and twice the orthogonality error on sigma_0)."""
    tr, c = traced
    f0 = _grid(c, NK)
    S = BU.amplitude_sums(BU.terms_of(tr), tr.nrx, tr.ntx)
    for rxe, txe in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
        r = _np(tr.channel_svd(rxe, txe, f0, DF, NK, dt=DT, num_times=NT))
        checked = 0
        for rx, tx, pol, m, k in ((0, 0, 0, 0, 0), (tr.nrx - 1, tr.ntx - 1, 1, NT - 1, NK - 1), (0, tr.ntx - 1, 1, 0, 7)):
            s0 = float(r["sigma"][rx, tx, 0, pol, m, k])
            if s0 == 0.0:
                continue
            wr = mimo.combiner(r["u"][rx, tx, :, :, pol, m, k], 1)
            wt = mimo.precoder(r["v"][rx, tx, :, :, pol, m, k], 1)
            B = tr.beam_channel(rxe, txe, wr, wt, f0, DF, NK, dt=DT, num_times=NT).cpu().numpy()
            got = complex(B[rx, tx, 0, 0, pol, m, k])
            fro = float(np.sqrt((np.abs(H[rx, tx, :, :, pol, m, k].astype(np.complex128)) ** 2).sum()))
            tol = (2e-5 * np.abs(wr).sum() * np.abs(wt).sum() * S[rx, tx, pol]
                   + 4 * U.TOL_CONST * U.unit_roundoff(rxe.shape[0], txe.shape[0]) * fro)
            print("sigma_0 %.6g, beam %.6g%+.3gj, tolerance %.3g" % (s0, got.real, got.imag, tol))
            assert abs(got - s0) <= tol, (rx, tx, pol, m, k, got, s0, tol)
            checked += 1
        assert checked


_DROP_IN_CALL = """
import sys
import numpy as np
sys.path.insert(0, {repo!r})
import torch  # noqa: F401
import hermespy_rt_amd
sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
import hermespy_rt
from hermespy_rt_amd import abi, lib
from tests import configs as K
c = K.small(K.C1, 2000)
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
        len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {f0!r}, {df!r}, {nk}, rxe, txe)
kw = dict(dt={dt!r}, num_times={nt})
r = hermespy_rt.compute_channel_svd(*args, **kw)
H = hermespy_rt.compute_array_channel(*args, **kw)
spec = abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt})
r2 = abi.run_compute_channel_svd(lib.load(), *K.args(c), spec, rxe, txe)
assert np.array_equal(r["buffer"], r2["buffer"])
for k in ("sigma", "u", "v", "sweeps"):
    assert r[k].shape == r2[k].shape and r[k].dtype == r2[k].dtype and np.array_equal(r[k], r2[k]), k
s = hermespy_rt.compute_channel_svd(*args, vectors=False, **kw)
assert s["u"] is None and s["v"] is None and np.array_equal(s["sigma"], r["sigma"])
assert np.array_equal(s["sweeps"], r["sweeps"])
np.save(sys.argv[1], H)
np.save(sys.argv[4], r["buffer"])
"""


def test_drop_in_entries_decompose_their_own_channel(tmp_path):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return, to the bit, the
    decomposition Tracer.svd gives for the H that compute_array_channel returns for the same call"""
    c = CONFIGS["C1"]
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[1]
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "svd.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DT, nt=NT)] +
                       [str(x) for x in files], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    H, buf = np.load(files[0]), np.load(files[3])
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 16, 8, 2, NT, NK) and np.abs(H).max() > 0
    tr = _tracer(K.small(K.C1, 64))
    r = tr.svd(tr.torch.from_numpy(H).to(tr.device))
    got = r["buffer"].cpu().numpy()
    tr.close()
    assert buf.dtype == np.uint8 and np.array_equal(got, buf)
