"""The maximum-likelihood detection on traced channels (Tracer.channel_detect, Tracer.detect,
hrt_compute_channel_detect, hermespy_rt.compute_channel_detect) on box and simple_reflector with a few thousand rays,
2 x 2 and 4 x 2 elements: symbols sent from a fixed seed, Y built on the host from the traced H, Tracer.detect
against the float64 reference under the derived bounds and against the emulation to the bit, the traced form and the
drop-in entries (one batch and several) against it to the byte, and the sent hypothesis decided where the float64
margin is positive."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import detect as DT

from . import configs as K
from . import detect_util as U
from .pathsum_util import DF, _grid, _lam, _tracer, _ula

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DTIME = 5, 3, 1e-3
CONFIG = K.small(K.C1, 2000)
REFLECTOR = K.small(K.C2, 3000)         # simple_reflector


def _traced(c):
    tr = _tracer(c)
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    return tr


@pytest.fixture(scope="module")
def traced():
    tr = _traced(CONFIG)
    yield tr, CONFIG
    tr.close()


def _numpy(r):
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}
    for k in ("index", "status"):
        out[k] = out[k].view(np.uint32)
    return out


def _geometries(c):
    """(rx elements, tx elements, B): 2 x 2 with 16-QAM (Q = 256), 4 x 2 with QPSK (Q = 16).  The elements lie in
    general position: two transmit elements on a line perpendicular to every path (a reflector seen broadside) have
    equal columns in H, and then x_0 + x_1 is all the receiver sees -- hypotheses tie and no margin is positive."""
    lam = _lam(c)
    skew = np.outer(np.arange(4), [0.31, 0.0, 0.53]) * lam
    return [(np.array([[0, 0, 0], [1.1, 2.3, 0.7]]) * lam, np.array([[0, 0, 0], [0.9, 1.7, 2.9]]) * lam, 4),
            (_ula(4, 2 * lam) + skew, np.array([[0, 0, 0], [2.1, 0.8, 1.3]]) * lam, 2)]


@pytest.mark.parametrize("scene", ("box", "reflector"))
def test_channel_detect_against_the_reference(traced, scene):
    tr, c = traced if scene == "box" else (_traced(REFLECTOR), REFLECTOR)
    try:
        torch = tr.torch
        f0 = _grid(c, NK)
        decided = 0
        for rxe, txe, B in _geometries(c):
            H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT)
            assert float(H.abs().max()) > 0
            Hn = H.cpu().numpy()
            nr, nt = rxe.shape[0], txe.shape[0]
            Y, S, sent, n0 = U.send(Hn, B, 17 + nr)
            d_Y = torch.from_numpy(Y).to(tr.device)
            a = tr.detect(H, d_Y, S, n0)
            b = tr.channel_detect(rxe, txe, f0, DF, NK, dt=DTIME, num_times=NT, Y=d_Y, constellation=S, noise=n0)
            assert torch.equal(a["buffer"], b["buffer"])
            dev, ref, us = _numpy(a), DT.ml_reference(Hn, Y, S, n0, table=True), U.scale(Hn, Y, S)
            assert dev["index"].shape == (tr.nrx, tr.ntx, 2, NT, NK) and not dev["status"].any()
            assert dev["llr"].shape == (tr.nrx, tr.ntx, nt, B, 2, NT, NK)
            live = us > 0
            safe = np.where(live, us, 1.0)
            metric = U.metric_error(dev["metric"], ref, safe, dev["index"])
            llr = U.llr_error(dev["llr"], ref, safe, n0)
            ok, second = U.index_check(dev["index"], ref, us)
            # the sent hypothesis is decided wherever its float64 margin over every other one is positive beyond rounding
            d = ref["distances"]
            mine = np.take_along_axis(d, sent[..., None], -1)[..., 0]
            rest = np.where(np.arange(d.shape[-1]) == sent[..., None], np.inf, d).min(-1)
            clear = rest - mine > 2.0 * U.METRIC_BOUND * us
            print("%s %dx%d B %d: metric %.3f llr %.3f second rule %.3f clear %.3f"
                  % (scene, nr, nt, B, metric, llr, second, clear.mean()))
            assert metric <= U.METRIC_BOUND and llr <= U.LLR_BOUND and ok
            assert np.array_equal(dev["index"][clear], sent[clear].astype(np.uint32))
            decided += int(clear.sum())
            assert U.same(dev, U.emulate(Hn, Y, S, n0)) is None
            # without LLRs: the same decision, no llr region
            bare = tr.detect(H, d_Y, S, n0, llr=False)
            assert bare["llr"] is None and torch.equal(bare["index"], a["index"]) and torch.equal(bare["metric"], a["metric"])
        assert decided > 0, "no point of the scene has a positive margin: the test geometry ties the hypotheses"
    finally:
        if scene != "box":
            tr.close()


def test_detect_refuses_tensors_of_the_wrong_kind(traced):
    tr, c = traced
    torch = tr.torch
    H = torch.zeros((1, 1, 2, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    Y = torch.zeros((1, 1, 2, 2, 1, 3), dtype=torch.complex64, device=tr.device)
    S = DT.qam(2)
    for args, what in (((H.cpu(), Y, S, 1.0), "H must be"), ((H, Y.cpu(), S, 1.0), "Y must be"),
                       ((H, Y[:, :, :1], S, 1.0), "expected"), ((H, Y, S[:3], 1.0), "2\\^B"),
                       ((H, Y, DT.qam(7), 1.0), "nt \\* bits"), ((H, Y, S, 0.0), "noise"),
                       ((H, Y, S, float("nan")), "noise")):
        with pytest.raises(ValueError, match=what):
            tr.detect(*args)
    with pytest.raises(ValueError, match="needs Y"):
        tr.channel_detect(_ula(2, 0.1), _ula(2, 0.1), 3.5e9, DF, 3)


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
Y, S, sent, n0 = U.send(H, {bits}, 5)
spec = abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt})
st = lib.Stats()
bufs = []
for llr in (True, False):
    r = hermespy_rt.compute_channel_detect(*args, Y, S, n0, llr=llr, **kw)
    r2 = abi.run_compute_channel_detect(lib.load(), *K.args(c), spec, rxe, txe, Y, S, n0, llr, stats=st)
    assert np.array_equal(r["buffer"], r2["buffer"])
    for k in ("index", "metric", "status", "llr"):
        assert (r[k] is None) == (r2[k] is None), k
        if r[k] is not None:
            assert r[k].shape == r2[k].shape and r[k].dtype == r2[k].dtype and np.array_equal(r[k], r2[k]), k
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
    Tracer.detect gives for the H that compute_array_channel returns for the same call -- in one batch and when a small
    workspace budget cuts the trace into several: detection runs once, on the accumulated H"""
    rays = 20000 if batched else 3000         # (large enough for the batch loop to split)
    c = K.small(K.C3, rays)
    f0 = _grid(c, NK)
    rxe, txe, B = _geometries(c)[1]
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        tr = _tracer(c)
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
        tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "y.npy", "a.npy", "b.npy", "n0.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DTIME, nt=NT,
                                                                   bits=B, rays=rays)] + [str(x) for x in files],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    H, Y, n0 = np.load(files[0]), np.load(files[3]), float(np.load(files[6]))
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 4, 2, 2, NT, NK) and np.abs(H).max() > 0
    S = DT.qam(B).astype(np.complex64)
    tr = _tracer(K.small(K.C1, 64))
    try:
        d_H, d_Y = tr.torch.from_numpy(H).to(tr.device), tr.torch.from_numpy(Y).to(tr.device)
        for llr, f in ((True, files[4]), (False, files[5])):
            got = tr.detect(d_H, d_Y, S, n0, llr)["buffer"].cpu().numpy()
            buf = np.load(f)
            assert buf.dtype == np.uint8 and np.array_equal(got, buf), llr
    finally:
        tr.close()
