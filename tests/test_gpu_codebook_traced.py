"""The codebook selection on traced channels (Tracer.channel_codebook_select, Tracer.codebook_select,
hrt_compute_codebook_select, hermespy_rt.compute_codebook_select) on box and simple_reflector with a few thousand
rays: the composition with array_channel to the bit and against the float64 reference under the derived bounds, the
drop-in entries in one batch and in several, the equalizer on the effective channel, the DFT beam of a line-of-sight
link against beams.gains, and the rank report on a two-user stacked channel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import beams, equalize
from hermespy_rt_amd import codebook as CB

from . import codebook_util as U
from . import configs as K
from . import equalizer_util as EU
from .pathsum_util import DF, _grid, _lam, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NK, NT, DT, S = 8, 2, 1e-3, 3
CONFIG = K.small(K.C1, 2000)
CONFIG_2RX = dict(CONFIG, rx_pos=CONFIG["rx_pos"] + [[1.0, 2.0, 1.0]], rx_vel=CONFIG["rx_vel"] * 2)
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


@pytest.fixture(scope="module")
def traced_2rx():
    tr = _traced(CONFIG_2RX)
    yield tr, CONFIG_2RX
    tr.close()


def _noise(H, part=4.0):
    return float(np.float32(float((H.abs() ** 2).sum((2, 3)).max()) / part))


def _numpy(r):
    out = {k: (None if v is None else v.cpu().numpy()) for k, v in r.items()}
    for k in ("index", "status"):
        out[k] = out[k].view(np.uint32)
    return out


def _geometries(c):
    """(rx elements, tx elements, codebook): 2 x 8 dual-polarised rank 1; 4 x 8 random rank 3"""
    lam = _lam(c)
    rng = np.random.default_rng(8)
    return [(_ula(2, 3 * lam), _ula(8, lam / 2, axis=0), CB.dual_polarised(4, 4, 1).astype(np.complex64)),
            (_ula(4, 2 * lam), _upa(2, 4, lam / 2), U.random_codebook(rng, 70, 8, 3))]


@pytest.mark.parametrize("scene", ("box", "reflector"))
def test_channel_codebook_select_against_the_reference(traced, scene):
    tr, c = traced if scene == "box" else (_traced(REFLECTOR), REFLECTOR)
    try:
        torch = tr.torch
        f0 = _grid(c, NK)
        for rxe, txe, W in _geometries(c):
            H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
            assert float(H.abs().max()) > 0
            n0 = _noise(H)
            nr, nt = rxe.shape[0], txe.shape[0]
            for metric in ("power", "capacity"):
                a = tr.codebook_select(H, W, metric, n0, S, True, True)
                b = tr.channel_codebook_select(rxe, txe, f0, DF, NK, dt=DT, num_times=NT, codebook=W, metric=metric,
                                               noise=n0, subband=S, table=True, effective=True)
                assert torch.equal(a["buffer"], b["buffer"])
                Hn = H.cpu().numpy()
                dev, ref = _numpy(a), CB.select_reference(Hn, W, metric, n0, S)
                assert dev["index"].shape == (tr.nrx, tr.ntx, 2, NT, 3) and not dev["status"].any()
                mu = U.mu_error(dev["table"], ref["table"], nr, nt)
                eff = U.eff_error(dev["effective"], ref, Hn, W, dev["index"])
                ok, second = U.index_check(dev["index"], ref, nr, nt)
                print("%s %dx%d %s: mu %.3f effective %.3f second rule %.3f" % (scene, nr, nt, metric, mu, eff, second))
                assert mu <= U.MU_BOUND and eff <= U.EFF_BOUND and ok
                assert U.same(dev, U.emulate(Hn, W, U.POWER if metric == "power" else U.CAPACITY, n0, S)) is None
            # wideband is subband = K, and the bare call returns no optional region
            wide = tr.codebook_select(H, W, "power")
            assert tuple(wide["index"].shape) == (tr.nrx, tr.ntx, 2, NT, 1) and wide["table"] is None
            assert torch.equal(wide["buffer"], tr.codebook_select(H, W, "power", subband=NK)["buffer"])
    finally:
        if scene != "box":
            tr.close()


def test_equalizer_takes_the_effective_channel(traced):
    tr, c = traced
    torch = tr.torch
    f0 = _grid(c, NK)
    for rxe, txe, W in _geometries(c):
        H = tr.array_channel(rxe, txe, f0, DF, NK, dt=DT, num_times=NT)
        if W.shape[2] > rxe.shape[0]:
            continue
        n0 = _noise(H)
        r = tr.codebook_select(H, W, "capacity", n0, S, effective=True)
        eq = tr.equalizer(r["effective"], n0, "lmmse")
        # H W[c*] formed in torch, per subband
        idx = r["index"].to(torch.int64).repeat_interleave(S, dim=-1)[..., :NK]              # [nrx, ntx, 2, T, K]
        Wt = torch.from_numpy(W).to(tr.device)[idx]                                          # [.., K, Nt, L]
        E = torch.einsum("abitpmk,abpmktl->abilpmk", H, Wt).contiguous()
        assert tuple(E.shape) == tuple(r["effective"].shape)
        worst = EU.check(EU.to_batch(E.cpu().numpy()), n0, EU.LMMSE, EU.to_batch(eq["W"].cpu().numpy()),
                         EU.to_batch_vec(eq["sinr"].cpu().numpy()), eq["status"].cpu().numpy().ravel())
        print("equalizer on effective, L = %d: measures %s" % (W.shape[2], " ".join("%.3g" % w for w in worst)))
        assert torch.equal(CB.cqi_sinr(tr, r["effective"], n0), eq["sinr"])
        assert float(eq["sinr"].max()) > 0


def test_dft_beam_of_a_line_of_sight_link_is_the_one_beams_gains_ranks_first(traced):
    tr, c = traced
    n = 8
    txe = _ula(n, _lam(c) / 2, axis=0)
    f0 = _grid(c, NK)
    H = tr.array_channel(np.zeros((1, 3)), txe, f0, DF, NK, los=True, scatter=False)
    assert float(H.abs().max()) > 0, "no line of sight in the test scene"
    W = CB.dft(n, 4)
    r = _numpy(tr.codebook_select(H, W, "power"))
    fa = c["f_ghz"] * 1e9
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            u = np.asarray(c["rx_pos"][rx], np.float64) - np.asarray(c["tx_pos"][tx], np.float64)
            g = np.abs(beams.gains(txe, W[:, :, 0], u / np.linalg.norm(u), fa)[:, 0]) ** 2
            order = np.argsort(g)
            got = int(r["index"][rx, tx, 0, 0, 0])
            assert g[order[-1]] - g[order[-2]] > 1e-4 * g[order[-1]], "the test geometry ties two beams"
            assert got == order[-1] == int(r["index"][rx, tx, 1, 0, 0]), (got, order[-3:])


def test_select_rank_on_a_two_user_stacked_channel(traced_2rx):
    tr, c = traced_2rx
    f0 = _grid(c, NK)
    links = tr.array_channel(np.zeros((1, 3)), _ula(8, _lam(c) / 2, axis=0), f0, DF, NK, dt=DT, num_times=NT)
    H = equalize.stack_users(links, "rx").contiguous()
    assert tuple(H.shape) == (1, tr.ntx, 2, 8, 2, NT, NK)
    books = {1: CB.dual_polarised(4, 2, 1).astype(np.complex64), 2: CB.dual_polarised(4, 2, 2).astype(np.complex64)}
    Hn = H.cpu().numpy()
    seen = set()
    for part in (1e4, 1e-2):            # a high and a low signal-to-noise ratio
        n0 = _noise(H, part)
        got = CB.select_rank(tr, H, books, n0, S)
        caps = np.stack([CB.select_reference(Hn, books[L], "capacity", n0, S)["metric"] for L in (1, 2)])
        want = 1 + np.argmax(caps, 0)
        clear = np.abs(caps[0] - caps[1]) > 2 * U.MU_BOUND * (2 + 8) * 2.0 ** -24 * (1 + caps.max(0))
        rank = got["rank"].cpu().numpy()
        assert clear.mean() >= 0.9 and np.array_equal(rank[clear], want[clear])
        for L in (1, 2):
            sel = got["selections"][L]["index"].cpu().numpy().astype(np.int64)
            assert np.array_equal(got["index"].cpu().numpy()[rank == L], sel[rank == L])
        seen |= set(want[clear].tolist())
    assert seen == {1, 2}               # rank 2 at the high ratio, rank 1 at the low one


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
c = K.small(K.C3, {rays})
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
W = np.load(sys.argv[4])
nrx, ntx = len(c["rx_pos"]), len(c["tx_pos"])
args = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
        c["num_bounces"], {f0!r}, {df!r}, {nk}, rxe, txe)
kw = dict(dt={dt!r}, num_times={nt})
H = hermespy_rt.compute_array_channel(*args, **kw)
n0 = float(np.float32((np.abs(H) ** 2).sum((2, 3)).max() / 4))
spec = abi.channel_spec({f0!r}, {df!r}, {nk}, 0.0, {dt!r}, {nt})
st = lib.Stats()
bufs = []
for metric, table, effective in (("capacity", True, True), ("power", False, True), ("capacity", False, False)):
    r = hermespy_rt.compute_codebook_select(*args, W, metric, n0, {s}, table=table, effective=effective, **kw)
    r2 = abi.run_compute_codebook_select(lib.load(), *K.args(c), spec, rxe, txe, W, metric, n0, {s}, table, effective,
                                         stats=st)
    assert np.array_equal(r["buffer"], r2["buffer"])
    for k in ("index", "metric", "status", "table", "effective"):
        assert (r[k] is None) == (r2[k] is None), k
        if r[k] is not None:
            assert r[k].shape == r2[k].shape and r[k].dtype == r2[k].dtype and np.array_equal(r[k], r2[k]), k
    assert (r["table"] is None) == (not table) and (r["effective"] is None) == (not effective)
    bufs.append(r["buffer"])
np.save(sys.argv[1], H)
for f, b in zip(sys.argv[5:8], bufs):
    np.save(f, b)
np.save(sys.argv[8], np.float32(n0))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_drop_in_entries_select_on_their_own_channel(tmp_path, batched):
    """the drop-in entries (pybind and C, bitwise equal; a fresh child process runs them) return, to the bit, what
    Tracer.codebook_select gives for the H that compute_array_channel returns for the same call -- in one batch and when
    a small workspace budget cuts the trace into several: the selection runs once, on the accumulated H"""
    rays = 20000 if batched else 3000         # (large enough for the batch loop to split)
    c = K.small(K.C3, rays)
    f0 = _grid(c, NK)
    rxe, txe, W = _geometries(c)[1]
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        tr = _tracer(c)
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
        tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "w.npy", "a.npy", "b.npy", "c.npy", "n0.npy")]
    np.save(files[1], rxe)
    np.save(files[2], txe)
    np.save(files[3], W)
    p = subprocess.run([sys.executable, "-c", _DROP_IN_CALL.format(repo=REPO, f0=f0, df=DF, nk=NK, dt=DT, nt=NT, s=S,
                                                                   rays=rays)] + [str(x) for x in files],
                       env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    H, n0 = np.load(files[0]), float(np.load(files[7]))
    assert H.shape == (len(c["rx_pos"]), len(c["tx_pos"]), 4, 8, 2, NT, NK) and np.abs(H).max() > 0
    tr = _tracer(K.small(K.C1, 64))
    try:
        d_H = tr.torch.from_numpy(H).to(tr.device)
        for metric, table, effective, f in (("capacity", True, True, files[4]), ("power", False, True, files[5]),
                                            ("capacity", False, False, files[6])):
            got = tr.codebook_select(d_H, W, metric, n0, S, table, effective)["buffer"].cpu().numpy()
            buf = np.load(f)
            assert buf.dtype == np.uint8 and np.array_equal(got, buf), (metric, table, effective)
    finally:
        tr.close()
