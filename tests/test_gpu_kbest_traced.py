"""The K-best detection on traced channels (Tracer.channel_kbest, Tracer.kbest, hrt_compute_channel_kbest,
hermespy_rt.compute_channel_kbest) on box with a few thousand rays: the traced form against kbest(array_channel(...))
to the byte and against the emulation to the bit, a 4 x 4 16-QAM link at high SNR that decodes what was sent, the
line-of-sight link whose channel is close to rank one (deficient points, finite output), and the drop-in entries (one
batch and several) against Tracer.kbest to the byte."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import detect as DT

from . import configs as K
from . import kbest_util as U
from .detect_util import send
from .pathsum_util import DF, _grid, _lam, _tracer, _ula

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DTIME = 5, 3, 1e-3
CONFIG = K.small(K.C1, 2000)
CLIP = 40.0


@pytest.fixture(scope="module")
def traced():
    tr = _tracer(CONFIG)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIG
    tr.close()


def _numpy(r):
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}
    for k in ("index", "status"):
        out[k] = out[k].view(np.uint32)
    return out


def _elements(c, n):
    """n elements in general position (no two columns of H equal by symmetry)"""
    lam = _lam(c)
    return _ula(n, 2 * lam) + np.outer(np.arange(n), [0.31, 0.17, 0.53]) * lam


def test_channel_kbest_is_kbest_of_the_array_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    for nr, nt, B, k, srt in ((2, 2, 4, 4, True), (4, 2, 2, 2, False), (4, 4, 4, 16, True)):
        rxe, txe = _elements(c, nr), _elements(c, nt)[::-1].copy()
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT)
        assert float(H.abs().max()) > 0
        Hn = H.cpu().numpy()
        Y, S, sent, n0 = send(Hn, B, 23 + nr, snr=1e3)
        d_Y = torch.from_numpy(Y).to(tr.device)
        for llr in (True, False):
            a = tr.kbest(H, d_Y, S, n0, k, CLIP, srt, llr)
            b = tr.channel_kbest(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT, Y=d_Y, constellation=S, noise=n0, k=k,
                                 clip=CLIP, sorted=srt, llr=llr)
            assert torch.equal(a["buffer"], b["buffer"])
            dev = _numpy(a)
            assert dev["index"].shape == (tr.nrx, tr.ntx, 2, NT, NK) and (dev["status"] != U.NONFINITE).all()
            assert (dev["llr"] is None) == (not llr)
            if llr:
                assert dev["llr"].shape == (tr.nrx, tr.ntx, nt, B, 2, NT, NK)
            assert U.same(dev, U.emulate(Hn, Y, S, n0, k, CLIP, srt, llr)) is None


def test_a_4x4_16qam_link_at_high_snr_decodes_what_was_sent(traced):
    """the scattered part of the box channel (the line of sight alone is of rank one: the next test), elements eight
    wavelengths apart, noise 120 dB below the received power: what limits the decision is float32, not the noise"""
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    lam = _lam(c)
    rxe = _ula(4, 8 * lam) + np.outer(np.arange(4), [0.31, 0.17, 0.53]) * lam
    txe = rxe[::-1].copy()
    H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT, los=False)
    Hn = H.cpu().numpy()
    sv = np.linalg.svd(np.moveaxis(Hn, (2, 3), (-2, -1)).astype(np.complex128), compute_uv=False)
    print("condition numbers: median %.3g, largest %.3g" % (np.median(sv[..., 0] / sv[..., -1]),
                                                           (sv[..., 0] / sv[..., -1]).max()))
    Y, S, sent, n0 = send(Hn, 4, 41, snr=1e12)
    k = 64
    dev = _numpy(tr.kbest(H, torch.from_numpy(Y).to(tr.device), S, n0, k, CLIP))
    ref = U.reference(Hn, Y, S, n0, k, CLIP)
    # decided wherever the float64 search decides it beyond rounding
    clear = (ref["index"] == sent) & (ref["lead"] > 2.0 * U.METRIC_BOUND * U.unit(4, 4)) & U.sturdy(ref, 4, 4, True)
    print("clear %.3f, decoded %.3f, deficient %.3f" % (clear.mean(), (dev["index"] == sent).mean(),
                                                        (dev["status"] == U.DEFICIENT).mean()))
    assert clear.any(), "no point of the scene decodes in float64: the test geometry ties the hypotheses"
    assert np.array_equal(dev["index"][clear], sent[clear].astype(np.uint32))
    bits = DT.hard_bits(dev["index"], 4, 4)
    assert DT.bit_errors(bits[clear], DT.hard_bits(sent, 4, 4)[clear]) == 0
    # the signs of the LLRs there are the sent bits
    L = np.moveaxis(dev["llr"], (2, 3), (-2, -1))[clear]
    assert ((L > 0) == (bits[clear] == 1))[L != 0].all()
    assert U.same(dev, U.emulate(Hn, Y, S, n0, k, CLIP)) is None


def test_the_line_of_sight_link_is_deficient_and_still_detected(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    rxe, txe = _elements(c, 4), _elements(c, 4)[::-1].copy()
    H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT, scatter=False)   # one path: rank one
    Hn = H.cpu().numpy()
    assert np.abs(Hn).max() > 0
    Y, S, sent, n0 = send(Hn, 2, 43, snr=1e3)
    dev = _numpy(tr.kbest(H, torch.from_numpy(Y).to(tr.device), S, n0, 8, CLIP))
    seen = np.abs(Hn).sum((2, 3)) > 0
    print("deficient %.3f of %d points with a path" % ((dev["status"][seen] == U.DEFICIENT).mean(), seen.sum()))
    assert (dev["status"] == U.DEFICIENT)[seen].any() and (dev["status"] != U.NONFINITE).all()
    assert np.isfinite(dev["metric"]).all() and np.isfinite(dev["llr"]).all() and (dev["index"] < 256).all()
    assert (np.abs(dev["llr"]) <= np.float32(CLIP)).all()
    assert U.same(dev, U.emulate(Hn, Y, S, n0, 8, CLIP)) is None


def test_kbest_refuses_tensors_of_the_wrong_kind(traced):
    tr, c = traced
    torch = tr.torch
    H = torch.zeros((1, 1, 2, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    Y = torch.zeros((1, 1, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    S = DT.qam(2)
    for args, what in (((H.cpu(), Y, S, 1.0, 4, 8.0), "H must be"), ((H, Y.cpu(), S, 1.0, 4, 8.0), "Y must be"),
                       ((H, Y[:, :, :1], S, 1.0, 4, 8.0), "expected"), ((H, Y, S[:3], 1.0, 4, 8.0), "2\\^B"),
                       ((H, Y, S, 0.0, 4, 8.0), "noise"), ((H, Y, S, float("nan"), 4, 8.0), "noise"),
                       ((H, Y, S, 1.0, 3, 8.0), "k = 3"), ((H, Y, S, 1.0, 0, 8.0), "k = 0"),
                       ((H, Y, S, 1.0, 128, 8.0), "k = 128"), ((H, Y, S, 1.0, -1, 8.0), "k = -1"),
                       ((H, Y, S, 1.0, 4, 0.0), "clip"), ((H, Y, S, 1.0, 4, float("inf")), "clip")):
        with pytest.raises(ValueError, match=what):
            tr.kbest(*args)
    H17 = torch.zeros((1, 1, 2, 17, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    with pytest.raises(ValueError, match="1 <= nt <= 16"):
        tr.kbest(H17, Y, DT.qam(1), 1.0, 4, 8.0)
    with pytest.raises(ValueError, match="needs Y"):
        tr.channel_kbest(_ula(2, 0.1), _ula(2, 0.1), 3.5e9, DF, 3)


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
from tests import detect_util as U
c = K.small(K.C3, {rays})
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
nrx, ntx = len(c["rx_pos"]), len(c["tx_pos"])
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
        c["num_bounces"], {f0!r}, {df!r}, {nk}, rxe, txe)
kw = dict(dt={dt!r}, num_times={nt})
H = hermespy_rt.compute_array_channel(*args, **kw)
Y, S, sent, n0 = U.send(H, {bits}, 5, snr=1e3)
spec = abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt})
st = lib.Stats()
bufs = []
for llr, srt in ((True, True), (False, False)):
    r = hermespy_rt.compute_channel_kbest(*args, Y, S, n0, {k}, {clip!r}, llr=llr, sorted=srt, **kw)
    r2 = abi.run_compute_channel_kbest(lib.load(), *K.args(c), spec, rxe, txe, Y, S, n0, {k}, {clip!r}, srt, llr,
                                       stats=st)
    assert np.array_equal(r["buffer"], r2["buffer"])
    for key in ("index", "metric", "status", "llr"):
        assert (r[key] is None) == (r2[key] is None), key
        if r[key] is not None:
            assert r[key].shape == r2[key].shape and r[key].dtype == r2[key].dtype and np.array_equal(r[key], r2[key])
    assert (r["llr"] is None) == (not llr)
    bufs.append(r["buffer"])
np.save(sys.argv[1], H)
np.save(sys.argv[4], Y)
np.save(sys.argv[5], bufs[0])
np.save(sys.argv[6], bufs[1])
np.save(sys.argv[7], np.float32(n0))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_drop_in_entries_detect_on_their_own_channel(tmp_path, batched):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return, to the byte, what
    Tracer.kbest gives for the H that compute_array_channel returns for the same call -- in one batch and when a small
    workspace budget cuts the trace into several: detection runs once, on the accumulated H"""
    rays = 20000 if batched else 3000         # (large enough for the batch loop to split)
    c = K.small(K.C3, rays)
    f0 = _grid(c, NK)
    lam = _lam(c)
    rxe = _ula(4, 2 * lam) + np.outer(np.arange(4), [0.31, 0.0, 0.53]) * lam
    txe = np.array([[0, 0, 0], [2.1, 0.8, 1.3]]) * lam
    B, k = 4, 8
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        tr = _tracer(c)
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
        tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "y.npy", "a.npy", "b.npy", "n0.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DTIME, nt=NT,
                                                                   bits=B, rays=rays, k=k, clip=CLIP)]
                       + [str(x) for x in files], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    H, Y, n0 = np.load(files[0]), np.load(files[3]), float(np.load(files[6]))
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 4, 2, 2, NT, NK) and np.abs(H).max() > 0
    S = DT.qam(B).astype(np.complex64)
    tr = _tracer(K.small(K.C1, 64))
    try:
        d_H, d_Y = tr.torch.from_numpy(H).to(tr.device), tr.torch.from_numpy(Y).to(tr.device)
        for (llr, srt), f in (((True, True), files[4]), ((False, False), files[5])):
            got = tr.kbest(d_H, d_Y, S, n0, k, CLIP, srt, llr)["buffer"].cpu().numpy()
            buf = np.load(f)
            assert buf.dtype == np.uint8 and np.array_equal(got, buf), (llr, srt)
    finally:
        tr.close()
