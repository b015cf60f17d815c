"""Beamformed (codebook) channel responses formed on the device (Tracer.beam_channel, hrt_beam_channel,
hermespy_rt.compute_beam_channel) against float64 numpy sums over the same float32 inputs (tests/beam_util.py):

    B[rx, tx, a, b, pol, m, k] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_k tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)

Tolerance per (link, a, b, pol), over all (m, k): |B - B64| <= 1e-5 ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol|, the
array tolerance per element pair summed over the pairs.  tests/test_beams_host.py shows that this bound sees an
unconjugated combiner, a conjugated precoder and swapped beam axes."""
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_util as BU
from . import configs as K
from . import scenes_gen as G
from .pathsum_util import ARRAY_CASES as CASES
from .pathsum_util import C0, DF, _cfg, _grid, _lam, _random, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETILE = 32   # csrc/hrt_beam_channel.h HRT_BM_ETILE: elements whose phase factors are in LDS at a time


def _combos(c):
    """(name, rx_elements, tx_elements, W_rx, W_tx): the (Br, Bt) cases straddle the 16-row MFMA tile and the 32-pair
    block; the element counts are 1 (a single complex weight != 1), 7 random, 15 (a 3 x 5 UPA), and the kernel's
    element tile and tile + 1"""
    lam = _lam(c)
    one = np.zeros((1, 3))
    r7, u15 = _random(7, 4 * lam, 11), _upa(3, 5, lam / 2)
    e32, e33 = _random(ETILE, 6 * lam, 5), _upa(3, 11, lam / 2)
    assert e33.shape[0] == ETILE + 1
    return [
        ("1x1_single", one, one, np.array([[0.6 - 0.8j]], np.complex64) * 1.5, np.array([[-0.3 + 0.4j]], np.complex64)),
        ("3x5", r7, u15, BU.random_weights(3, 7, 1), BU.random_weights(5, 15, 2)),
        ("4x8", u15, r7, BU.random_weights(4, 15, 3), BU.random_weights(8, 7, 4)),
        ("1x17_tile", e32, e33, BU.random_weights(1, ETILE, 5), BU.random_weights(17, ETILE + 1, 6)),
        ("17x2_tile", e33, e32, BU.random_weights(17, ETILE + 1, 7), BU.random_weights(2, ETILE, 8)),
    ]


def _ft(c, nk, nt, dt):
    f0 = _grid(c, nk)
    return f0, f0 + np.arange(nk, dtype=np.float64) * DF, np.arange(nt, dtype=np.float64) * dt


def _check_combos(tr, c, nk, nt, dt, combos, what):
    f0, f, t = _ft(c, nk, nt, dt)
    fa = c["f_ghz"] * 1e9
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    want = BU.beam_direct(T, tr.nrx, tr.ntx, None, None, [x[1:] for x in combos], fa, f, t)
    for (name, rxe, txe, wr, wt), B in zip(combos, want):
        got = tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
        BU.check(got, B, S, wr, wt, what="%s %s" % (what, name))


@pytest.mark.parametrize("name,n,nt,nk", CASES, ids=[c[0] for c in CASES])
def test_beam_channel_matches_float64(name, n, nt, nk):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    _check_combos(tr, c, nk, nt, 1e-3 if nt > 1 else 0.0, _combos(c), name)
    tr.close()


def test_more_tx_beams_than_a_pair_block():
    """Bt = 40 > 32: a pair block no longer touches every TX beam; its TX slots are the beams of its own pairs, which
    wrap around within a block (pairs 32 .. 63 are b = 32 .. 39 of a = 0 and b = 0 .. 23 of a = 1)"""
    c = _cfg("C4_DOPPLER", 4000)
    tr = _tracer(c)
    tr.trace()
    lam = _lam(c)
    combo = ("2x40", _ula(2, lam / 2), _random(7, 4 * lam, 11), BU.random_weights(2, 2, 9), BU.random_weights(40, 7, 10))
    _check_combos(tr, c, 50, 2, 1e-3, [combo], "C4_DOPPLER")
    tr.close()


def test_identity_codebooks_are_the_array_channel():
    """W = I on both sides: beam (a, b) is element pair (i, j), within twice the per-pair bound"""
    c = _cfg("C3", 20000)
    tr = _tracer(c)
    tr.trace()
    lam = _lam(c)
    rxe, txe = _ula(2, lam / 2), _upa(3, 5, lam / 2)
    nk, nt, dt = 257, 2, 1e-3
    f0, _, _ = _ft(c, nk, nt, dt)
    got = tr.beam_channel(rxe, txe, np.eye(2), np.eye(15), f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    want = tr.array_channel(rxe, txe, f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    S = BU.amplitude_sums(BU.terms_of(tr), tr.nrx, tr.ntx)
    tr.close()
    assert got.shape == want.shape
    err = np.abs(got.astype(np.complex128) - want).reshape(*got.shape[:5], -1).max(axis=-1)
    assert (err <= 2e-5 * S[:, :, None, None, :] + 1e-30).all(), (err / np.maximum(S[:, :, None, None, :], 1e-30)).max()


@pytest.mark.parametrize("name,n", [("C3", 20000), ("C4_DOPPLER", 4000), ("COINCIDENT", 8000)])
def test_single_unit_beam_is_the_channel(name, n):
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    nk, nt, dt = 300, 2, 1e-3
    f0, _, _ = _ft(c, nk, nt, dt)
    one = np.zeros((1, 3))
    got = tr.beam_channel(one, one, [[1.0]], [[1.0]], f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    want = tr.channel(f0, DF, nk, dt=dt, num_times=nt).cpu().numpy()
    S = BU.amplitude_sums(BU.terms_of(tr), tr.nrx, tr.ntx)
    tr.close()
    assert got.shape == (want.shape[0], want.shape[1], 1, 1, 2, nt, nk)
    err = np.abs(got[:, :, 0, 0].astype(np.complex128) - want).reshape(*want.shape[:3], -1).max(axis=-1)
    assert (err <= 2e-5 * S + 1e-30).all(), (err / np.maximum(S, 1e-30)).max()


# a clear LoS of 30 m in the street canyon (TX above the cars): the SIGN_CFG of tests/test_gpu_array_channel.py
SIGN_CFG = K.cfg("simple_street_canyon_with_cars.hrt", [[-10.0, 1.0, 3.0]], [[-40.0, 0.0, 5.0]], 3.5, 2000, 1)


@pytest.mark.parametrize("side", ["rx", "tx"])
def test_conjugation_on_the_line_of_sight(side):
    """LoS only, an 8-element lambda / 2 ULA oblique to the LoS: steering weights matched in the convention of the
    definition collect |B| = 8 a; the mirrored (conjugate) weights lose more than half"""
    c = dict(SIGN_CFG)
    tr = _tracer(c)
    tr.trace()
    L = tr.los()[0, 0]
    assert int(L[0:1].view(np.uint32)[0]) == 2 and L[2] * C0 >= 20.0
    a = float(L[1])
    u_tx = L[3:6].astype(np.float64)   # TX -> RX
    u = -u_tx if side == "rx" else u_tx
    fa = c["f_ghz"] * 1e9
    # the axis at 60 degrees to x in the x-y plane (the LoS runs along x within a few degrees): r . u is about a
    # quarter wavelength per element, and the mirrored weights see the array factor at twice that phase step
    axis = np.array([0.5, np.sqrt(0.75), 0.0])
    ula = np.arange(8)[:, None] * (_lam(c) / 2) * axis[None, :]
    step = abs(float(axis @ u)) / 2   # revolutions per element
    mirrored = abs(np.sum(np.exp(2j * np.pi * 2 * step * np.arange(8))))
    assert step > 0.15 and mirrored < 3.0, (step, mirrored)
    s = beams.steering(ula.astype(np.float32), u, fa)[None, :]
    one, w1 = np.zeros((1, 3)), np.ones((1, 1))
    # the combiner is applied conjugated, so it matches with W_rx = s; the precoder as it is, so with W_tx = conj(s)
    match, mirror = (s, np.conj(s)) if side == "rx" else (np.conj(s), s)
    out = []
    for w in (match, mirror):
        args = (ula, one, w, w1) if side == "rx" else (one, ula, w1, w)
        out.append(tr.beam_channel(*args, fa, DF, 1, scatter=False, array_frequency=fa).cpu().numpy()[0, 0, 0, 0, :, 0, 0])
    tr.close()
    bound = 1e-5 * 8 * a
    assert (np.abs(np.abs(out[0]) - 8 * a) <= bound).all(), (out[0], 8 * a)
    assert (np.abs(out[1]) < 4 * a).all(), (out[1], 4 * a)


def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nk = 200
    f0, f, t = _ft(c, nk, 1, 0.0)
    _, rxe, txe, wr, wt = _combos(c)[1]
    fa = c["f_ghz"] * 1e9
    tr = _tracer(c)
    tr.trace()
    whole = tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk)
    again = tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk, out=out, accumulate=True)
    tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk, out=out, accumulate=True)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    B, = BU.beam_direct(T, tr.nrx, tr.ntx, rxe, txe, [(wr, wt)], fa, f, t)
    BU.check(whole.cpu().numpy(), B, S, wr, wt, what="whole")
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.beam_channel(rxe, txe, wr, wt, f0, DF, nk, out=acc, accumulate=acc is not None)
            ts.close()
        BU.check(acc.cpu().numpy(), B, S, wr, wt, what="world %d" % world)   # LoS counted once


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
rxe, txe = np.load(sys.argv[2]).astype(np.float32), np.load(sys.argv[3]).astype(np.float32)
wr, wt = np.load(sys.argv[4]), np.load(sys.argv[5])
B = hermespy_rt.compute_beam_channel(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                     np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                     np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
                                     len(c["tx_pos"]), c["num_paths"], c["num_bounces"], {f0!r}, {df!r}, {nk},
                                     rxe, txe, wr, wt)
np.save(sys.argv[1], B)
st = lib.Stats()
B2 = abi.run_compute_beam_channel(lib.load(), *K.args(c), abi.channel_spec({f0!r}, {df!r}, {nk}), rxe, txe, wr, wt,
                                  stats=st)
assert np.array_equal(B.view(np.float32), B2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_beam_channel_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C, bitwise equal) agrees with Tracer.beam_channel on C3 at 20 k rays, also when a
    small workspace budget cuts the call into several batches (a fresh child process runs the drop-ins)"""
    c = K.small(K.C3, 20000)
    nk = 256
    f0, f, t = _ft(c, nk, 1, 0.0)
    _, rxe, txe, wr, wt = _combos(c)[1]
    tr = _tracer(c)
    tr.trace()
    want = tr.beam_channel(rxe, txe, wr, wt, f0, DF, nk).cpu().numpy()
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    B, = BU.beam_direct(T, tr.nrx, tr.ntx, rxe, txe, [(wr, wt)], c["f_ghz"] * 1e9, f, t)
    BU.check(want, B, S, wr, wt, what="tracer")
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    files = [tmp_path / n for n in ("b.npy", "rx.npy", "tx.npy", "wr.npy", "wt.npy")]
    for p, x in zip(files[1:], (rxe, txe, wr, wt)):
        np.save(p, x)
    p = subprocess.run([sys.executable, "-c", _PYBIND_CALL.format(repo=REPO, f0=f0, df=DF, nk=nk)] +
                       [str(x) for x in files], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = np.load(files[0])
    BU.check(got, B, S, wr, wt, what="drop-in")
    assert np.abs(got.astype(np.complex128) - want).max() <= 2e-5 * S.max()


def test_generated_scene_resorted_two_tx(tmp_path):
    """> 1 024 triangles: the live list is re-sorted between bounces; two TX with velocities, T = 2"""
    p = str(tmp_path / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    c = G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
              tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])
    tr = _tracer(c)
    assert tr.num_tri > 1024
    tr.trace()
    _check_combos(tr, c, 77, 2, 1e-3, _combos(c)[1:3], "room")
    tr.close()
