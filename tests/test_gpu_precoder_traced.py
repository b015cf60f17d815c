"""The per-point precoders of traced channels (Tracer.channel_precoder, Tracer.precoder, hrt_compute_channel_precoder,
hermespy_rt.compute_channel_precoder) on the smallest test scene, with 2 x 8 and 4 x 8 elements, 2 times x 8
frequencies: the composition with array_channel to the bit, the drop-in entries, a two-user downlink through
equalize.stack_users(H, "rx") against the float64 reference, zero-forcing's diagonal effective channel, RZF against the
equalizer family's LMMSE weights, and antenna patterns."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import equalize, precode
from hermespy_rt_amd import patterns as P

from . import configs as K
from . import equalizer_util as EU
from . import patterns_util as PU
from . import precoder_util as U
from .pathsum_util import DF, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DT = 8, 2, 1e-3
CONFIG = K.small(K.C1, 2000)
# the same scene and transmitter with a second receiver: the two users of the downlink.  (The box gives one path a link,
# so the array channel of ONE link has rank one, and zero-forcing more than one stream to it is singular.)
CONFIG_2RX = dict(CONFIG, rx_pos=CONFIG["rx_pos"] + [[1.0, 2.0, 1.0]], rx_vel=CONFIG["rx_vel"] * 2)
KINDS, NORMS = ("mrt", "zf", "rzf"), ("total", "stream")


def _geometries(c):
    """(Nr, Nt) = (2, 8): g = 1;  (4, 8): g = 2"""
    lam = _lam(c)
    return [(_ula(2, 3 * lam), _ula(8, lam / 2, axis=0)), (_ula(4, 2 * lam), _upa(2, 4, lam / 2))]


@pytest.fixture(scope="module")
def traced():
    tr = _tracer(CONFIG)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIG
    tr.close()


@pytest.fixture(scope="module")
def traced_2rx():
    tr = _tracer(CONFIG_2RX)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIG_2RX
    tr.close()


def _noise(H):
    """a quarter of the largest |H|_F^2 of any point, rounded to float32: with Ptot = 1 the SINRs are of order one"""
    return float(np.float32(float((H.abs() ** 2).sum((2, 3)).max()) / 4))


def test_channel_precoder_is_precoder_of_array_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        n0 = _noise(H)
        assert n0 > 0
        nr, nt = rxe.shape[0], txe.shape[0]
        assert U.form(nr, nt) == (1 if nr == 2 else 2)
        for kind in KINDS:
            for norm in NORMS:
                for weights in (True, False):
                    a = tr.precoder(H, n0, kind, 1.5, None, norm, weights)
                    b = tr.channel_precoder(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0, kind=kind, power=1.5,
                                            normalize=norm, weights=weights)
                    assert torch.equal(a["buffer"], b["buffer"])
                    assert (a["P"] is None) == (not weights) and (b["P"] is None) == (not weights)
        assert a["sinr"].shape == (tr.nrx, tr.ntx, nr, 2, NT, NK) and a["status"].shape == (tr.nrx, tr.ntx, 2, NT, NK)
        assert b["buffer"].numel() == tr.nrx * tr.ntx * 2 * NT * NK * (nr * 4 + 4)
        rz = tr.precoder(H, n0)
        assert not rz["status"].any() and float(rz["sinr"].max()) > 0 and rz["P"].shape[2:4] == (nt, nr)
        # the default regularization, and an explicit one
        assert torch.equal(rz["buffer"], tr.precoder(H, n0, "rzf", 1.0, precode.default_regularization(nr, n0))["buffer"])
        assert not torch.equal(rz["buffer"], tr.precoder(H, n0, "rzf", 1.0, n0)["buffer"])


def _two_users(tr, c):
    """two single-antenna users at the two receivers, served by 8 transmit elements: their two 1 x 8 links stacked
    along Nr by equalize.stack_users -> the 2 x 8 downlink tensor [1, ntx, 2, 8, 2, T, K]"""
    torch = tr.torch
    f0 = _grid(c, NK)
    links = tr.array_channel(np.zeros((1, 3)), _ula(8, _lam(c) / 2, axis=0), f0, DF, NK, dt=DT, num_times=NT)
    assert tuple(links.shape) == (2, tr.ntx, 1, 8, 2, NT, NK) and tr.nrx == 2
    H = equalize.stack_users(links, "rx")
    assert tuple(H.shape) == (1, tr.ntx, 2, 8, 2, NT, NK)
    assert torch.equal(H[0, :, 1], links[1, :, 0]) and torch.equal(H[0, :, 0], links[0, :, 0])
    return H


def test_two_user_downlink_against_the_reference(traced_2rx):
    tr, c = traced_2rx
    H = _two_users(tr, c)
    n0 = _noise(H)
    Hn = H.cpu().numpy()
    mats = U.to_batch(Hn)
    for kind, k in (("rzf", U.RZF), ("mrt", U.MRT)):
        for norm, nm in (("total", U.TOTAL), ("stream", U.STREAM)):
            r = tr.precoder(H, n0, kind, normalize=norm)
            got = (U.to_batch(r["P"].cpu().numpy()), U.to_batch_vec(r["sinr"].cpu().numpy()),
                   r["status"].cpu().numpy().astype(np.uint32).ravel())
            alpha = precode.default_regularization(2, n0) if k == U.RZF else 0.0
            worst = U.check(mats, n0, k, nm, 1.0, alpha, *got)
            print("two users %s %s: sinr <= %.3g, measures %s" % (kind, norm, got[1].max(),
                                                                   " ".join("%.3g" % w for w in worst)))
            assert got[1].max() > 0.1                       # (the check is not about zeros)
            # the SINR each user sees is sinr_of the stored P through the channel
            s = precode.sinr_of(Hn, r["P"].cpu().numpy(), n0)
            assert np.allclose(s, r["sinr"].cpu().numpy(), rtol=1e-3, atol=1e-5)
    assert precode.sum_rate(r["sinr"].cpu().numpy()).shape == (1, tr.ntx, 2, NT, NK)


def test_zero_forcing_leaves_no_interference(traced, traced_2rx):
    """under ZF, where a point is not flagged, E = H P of the stored P is diagonal within the precoder's bound:
    | E_ij | <= | h_i | | P^ - P |_F <= | h_i | TOL_P u kappa | P |_F for i != j, and sinr_i = s_i^2 / N0 with s_i = E_ii
    of the float64 reference, within TOL_SINR u kappa (1 + sinr_i).  The two-user downlink is regular at every point;
    the links of one receiver have rank one here, and whatever they flag is zero"""
    tr, c = traced
    f0 = _grid(c, NK)
    seen = 0
    tensors = [_two_users(*traced_2rx)] + [tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
                                           for rxe, txe in _geometries(c)]
    for n, H in enumerate(tensors):
        n0 = _noise(H)
        Hn = H.cpu().numpy()
        nr, nt = Hn.shape[2], Hn.shape[3]
        for norm in NORMS:
            r = traced_2rx[0].precoder(H, n0, "zf", normalize=norm)
            ref = precode.precoder_reference(Hn, n0, "zf", normalize=norm)
            st = r["status"].cpu().numpy()
            flagged = st != 0
            assert not r["P"].cpu().numpy()[:, :, :, :, flagged[0, 0]].any()
            assert not r["sinr"].cpu().numpy()[:, :, :, flagged[0, 0]].any()
            if n == 0:
                assert not flagged.any() and not ref["status"].any()
            ok = (~flagged & (ref["status"] == 0)).ravel()
            print("zf %dx%d %s: %d of %d points regular" % (nr, nt, norm, ok.sum(), ok.size))
            if not ok.any():
                continue
            seen += int(ok.sum())
            A = U.to_batch(Hn).astype(np.complex128)[ok]
            Pd = U.to_batch(r["P"].cpu().numpy()).astype(np.complex128)[ok]
            Pr = U.to_batch(ref["P"])[ok]
            kappa = ref["cond"].ravel()[ok]
            u = U.unit_roundoff(nr, nt)
            E = A @ Pd
            off = np.abs(E * (1 - np.eye(nr)))
            rows = np.sqrt((np.abs(A) ** 2).sum(2))                              # | h_i |
            fro = np.sqrt((np.abs(Pr) ** 2).sum((1, 2)))
            bound = rows[:, :, None] * (U.TOL_P * u * kappa * fro)[:, None, None]
            assert (off <= bound).all(), (off / bound).max()
            s2 = np.abs(np.diagonal(A @ Pr, axis1=1, axis2=2)) ** 2
            got = U.to_batch_vec(r["sinr"].cpu().numpy()).astype(np.float64)[ok]
            b = U.TOL_SINR * u * kappa[:, None] * (1 + s2 / n0)
            assert (np.abs(got - s2 / n0) <= b).all(), (np.abs(got - s2 / n0) / b).max()
            print("    kappa <= %.3g, off-diagonal / bound <= %.3g, sinr error / bound <= %.3g"
                  % (kappa.max(), (off / bound).max(), (np.abs(got - s2 / n0) / b).max()))
    assert seen >= 2 * 2 * NT * NK


def test_rzf_direction_is_the_equalizers_lmmse_weights(traced):
    """P0 = H^H (H H^H + alpha I)^-1 = (H^H H + alpha I)^-1 H^H is the LMMSE W of the same H with lambda = alpha, so
    P / |P|_F (TOTAL) and W / |W|_F agree within the sum of both families' bounds: the two kernels factor different
    matrices, [H^H; sqrt(alpha) I] and [H; sqrt(alpha) I].  (Normalising two vectors that differ by d moves them no
    further apart than 2 |d| / (|x| + |y|), Dunkl and Williams: the relative bounds carry over, to a factor 1.001.)"""
    tr, c = traced
    f0 = _grid(c, NK)
    for rxe, txe in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        n0 = _noise(H)
        nr, nt = rxe.shape[0], txe.shape[0]
        alpha = float(np.float32(precode.default_regularization(nr, n0)))
        pc = tr.precoder(H, n0, "rzf", 1.0, alpha)
        eq = tr.equalizer(H, alpha, "lmmse")
        assert not pc["status"].any() and not eq["status"].any()
        Pd = U.to_batch(pc["P"].cpu().numpy()).astype(np.complex128)
        Wd = U.to_batch(eq["W"].cpu().numpy()).astype(np.complex128)
        assert Pd.shape == Wd.shape == (Pd.shape[0], nt, nr)
        fro = lambda X: np.sqrt((np.abs(X) ** 2).sum((1, 2)))
        Hn = H.cpu().numpy()
        k_pc = precode.precoder_reference(Hn, n0, "rzf", 1.0, alpha)["cond"].ravel()
        k_eq = equalize.equalizer_reference(Hn, alpha, "lmmse")["cond"].ravel()
        bound = 1.001 * (U.TOL_P * U.unit_roundoff(nr, nt) * k_pc + EU.TOL_W * EU.unit_roundoff(nr, nt) * k_eq)
        err = fro(Pd / fro(Pd)[:, None, None] - Wd / fro(Wd)[:, None, None])
        print("%dx%d: kappa %.3g and %.3g, |P/|P| - W/|W|| / bound <= %.3g" % (nr, nt, k_pc.max(), k_eq.max(),
                                                                                (err / bound).max()))
        assert (err <= bound).all()
        assert fro(Wd).min() > 0


def test_patterns_weigh_the_precoded_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[0]
    plain_H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
    n0 = _noise(plain_H)
    plain = tr.channel_precoder(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)["buffer"].clone()
    rx, tx = P.tr38901(1.0), PU.pattern_set()["table_7x12"]
    tr.set_patterns(rx, tx, PU.random_rotations(tr.nrx, 61), PU.random_rotations(tr.ntx, 62))
    try:
        tr.trace()
        assert tr.patterned
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        assert not torch.equal(H, plain_H)
        got = tr.channel_precoder(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)
        assert torch.equal(got["buffer"], tr.precoder(H, n0)["buffer"])
        assert not torch.equal(got["buffer"], plain)
    finally:
        tr.set_patterns()
        tr.trace()
    assert torch.equal(tr.channel_precoder(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, noise=n0)["buffer"], plain)


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
for kind, norm, power, alpha in (("rzf", "total", 1.0, None), ("zf", "stream", 2.0, None), ("mrt", "total", 0.5, None),
                                 ("rzf", "stream", 1.0, 3.0 * n0)):
    r = hermespy_rt.compute_channel_precoder(*args, n0, kind, power, alpha, norm, **kw)
    r2 = abi.run_compute_channel_precoder(lib.load(), *K.args(c), spec, rxe, txe, n0, kind, power, alpha, norm)
    assert np.array_equal(r["buffer"], r2["buffer"])
    for k in ("P", "sinr", "status"):
        assert r[k].shape == r2[k].shape and r[k].dtype == r2[k].dtype and np.array_equal(r[k], r2[k]), k
    s = hermespy_rt.compute_channel_precoder(*args, n0, kind, power, alpha, norm, weights=False, **kw)
    assert s["P"] is None and np.array_equal(s["sinr"], r["sinr"]) and np.array_equal(s["status"], r["status"])
    bufs.append(r["buffer"])
pat = dict(rx=P.tr38901(1.0), tx=PU.pattern_set()["table_7x12"], rx_orientation=PU.random_rotations(nrx, 61),
           tx_orientation=PU.random_rotations(ntx, 62))
Hp = hermespy_rt.compute_array_channel(*args, patterns=pat, **kw)
rp = hermespy_rt.compute_channel_precoder(*args, n0, "rzf", patterns=pat, **kw)
assert not np.array_equal(Hp, H) and not np.array_equal(rp["buffer"], bufs[0])
again = hermespy_rt.compute_channel_precoder(*args, n0, "rzf", **kw)      # the setting is gone after the call
assert np.array_equal(again["buffer"], bufs[0])
np.save(sys.argv[1], H)
for f, b in zip(sys.argv[4:8], bufs):
    np.save(f, b)
np.save(sys.argv[8], Hp)
np.save(sys.argv[9], rp["buffer"])
np.save(sys.argv[10], np.float32(n0))
"""


def test_drop_in_entries_precode_their_own_channel(tmp_path):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return, to the bit, what
    Tracer.precoder gives for the H that compute_array_channel returns for the same call, with and without patterns"""
    c = CONFIG
    f0 = _grid(c, NK)
    rxe, txe = _geometries(c)[1]
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "rzf.npy", "zf.npy", "mrt.npy", "rzf_a.npy", "hp.npy",
                                    "rzf_p.npy", "n0.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DT, nt=NT)] +
                       [str(x) for x in files], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    H, Hp, n0 = np.load(files[0]), np.load(files[7]), float(np.load(files[9]))
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 4, 8, 2, NT, NK) and np.abs(H).max() > 0
    tr = _tracer(K.small(K.C1, 64))
    try:
        for h, kind, norm, power, alpha, f in ((H, "rzf", "total", 1.0, None, files[3]),
                                               (H, "zf", "stream", 2.0, None, files[4]),
                                               (H, "mrt", "total", 0.5, None, files[5]),
                                               (H, "rzf", "stream", 1.0, 3.0 * n0, files[6]),
                                               (Hp, "rzf", "total", 1.0, None, files[8])):
            got = tr.precoder(tr.torch.from_numpy(h).to(tr.device), n0, kind, power, alpha, norm)["buffer"].cpu().numpy()
            buf = np.load(f)
            assert buf.dtype == np.uint8 and np.array_equal(got, buf), (kind, norm)
    finally:
        tr.close()
