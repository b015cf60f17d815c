"""Beamformed (codebook) sampled impulse responses formed on the device (Tracer.beam_taps, hrt_beam_taps,
hermespy_rt.compute_beam_taps) against float64 numpy sums over the same float32 inputs (tests/beam_taps_util.py):

    h[rx, tx, a, b, pol, m, l] = sum_p a_p^pol exp(j 2 pi (nu_p t_m - f_c tau_p)) g_rx[a](u_p^rx) g_tx[b](u_p^tx)
                                       * sinc(l_min + l - f_s tau_p)

Tolerance per (link, a, b, pol), over all (m, l): |h - h64| <= 1e-5 ||W_rx[a]||_1 ||W_tx[b]||_1 sum_p |a_p^pol|
(|sinc| <= 1, so the bound of the beamformed channel carries over), and twice that where the other side is another
device family.  tests/test_beam_taps_design.py shows that this bound sees an unconjugated combiner, a conjugated
precoder, swapped beam axes and a gain added to the phase.  Then the identities of the contract, the parts and the LoS
classes, the exact-tap LoS, and the structure (shards, accumulate, determinism) and the drop-in entries."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from hermespy_rt_amd import beams

from . import beam_taps_util as BT
from . import beam_util as BU
from . import configs as K
from .pathsum_util import ARRAY_CASES as CASES
from .pathsum_util import C0, FS, PARTS, _cfg, _force_los_classes, _lam, _random, _tracer, _ula, _upa

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETILE = 32   # csrc/hrt_beam_channel.h HRT_BM_ETILE: elements whose phase factors are in LDS at a time
ONE = np.zeros((1, 3))


def _combos(c):
    """(name, rx_elements, tx_elements, W_rx, W_tx): the element and beam shapes of tests/test_gpu_beam_channel.py: 1
    element (a single complex weight != 1), 7 random, 15 (a 3 x 5 UPA), the kernel's element tile and tile + 1"""
    lam = _lam(c)
    r7, u15 = _random(7, 4 * lam, 11), _upa(3, 5, lam / 2)
    e32, e33 = _random(ETILE, 6 * lam, 5), _upa(3, 11, lam / 2)
    return [
        ("1x1_single", ONE, ONE, np.array([[0.6 - 0.8j]], np.complex64) * 1.5, np.array([[-0.3 + 0.4j]], np.complex64)),
        ("3x5", r7, u15, BU.random_weights(3, 7, 1), BU.random_weights(5, 15, 2)),
        ("4x8", u15, r7, BU.random_weights(4, 15, 3), BU.random_weights(8, 7, 4)),
        ("1x17_tile", e32, e33, BU.random_weights(1, ETILE, 5), BU.random_weights(17, ETILE + 1, 6)),
        ("17x2_tile", e33, e32, BU.random_weights(17, ETILE + 1, 7), BU.random_weights(2, ETILE, 8)),
    ]


def _direct(tr, T, combos, nl, l_min, t, fs=FS, fa=None, fc=None):
    f = tr.f_ghz * 1e9
    return BT.beam_taps_direct(T, tr.nrx, tr.ntx, None, None, [x[1:] for x in combos], f if fa is None else fa, fs,
                               f if fc is None else fc, nl, l_min, t)


def _check_combos(tr, nl, l_min, nt, dt, combos, what):
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    want = _direct(tr, T, combos, nl, l_min, dt * np.arange(nt))
    for (name, rxe, txe, wr, wt), h in zip(combos, want):
        got = tr.beam_taps(rxe, txe, wr, wt, FS, nl, l_min, dt=dt, num_times=nt).cpu().numpy()
        BU.check(got, h, S, wr, wt, what="%s %s" % (what, name))


# ------------------------------------------------------------------ 1. float64 reference
@pytest.mark.parametrize("name,n,nt,nk", CASES, ids=[c[0] for c in CASES])
def test_beam_taps_match_float64(name, n, nt, nk):
    """both forms: 1x1 with T = 1 or 4 is the <1, 4, 1> form, the others the <4, 4, 4> form; L = 40 is two and a half
    column tiles, l_min < 0"""
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    _check_combos(tr, 40, -3, nt, 1e-4 if nt > 1 else 0.0, _combos(c), name)
    tr.close()


# ------------------------------------------------------------------ 2. identities
@pytest.mark.parametrize("name,n", [("C3", 20000), ("C4_DOPPLER", 4000), ("COINCIDENT", 8000)])
def test_identities_with_the_other_families(name, n):
    """beams.apply of Tracer.array_taps; identity codebooks give array_taps; a single unit beam on one element at the
    origin gives taps -- each within twice the bound"""
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    lam = _lam(c)
    S = BU.amplitude_sums(BU.terms_of(tr), tr.nrx, tr.ntx)
    nl, l_min, nt, dt = 50, -3, 2, 1e-4
    kw = dict(l_min=l_min, dt=dt, num_times=nt)
    rxe, txe = _ula(2, lam / 2), _upa(3, 5, lam / 2)
    ha = tr.array_taps(rxe, txe, FS, nl, **kw).cpu().numpy()
    wr, wt = BU.random_weights(3, 2, 1), BU.random_weights(5, 15, 2)
    got = tr.beam_taps(rxe, txe, wr, wt, FS, nl, **kw).cpu().numpy()
    want = beams.apply(ha.astype(np.complex128), wr.astype(np.complex128), wt.astype(np.complex128))
    BU.check(got, want, S, wr, wt, 2e-5, name + " apply(array_taps)")
    eye_r, eye_t = np.eye(2, dtype=np.complex64), np.eye(15, dtype=np.complex64)
    got = tr.beam_taps(rxe, txe, eye_r, eye_t, FS, nl, **kw).cpu().numpy()
    BU.check(got, ha.astype(np.complex128), S, eye_r, eye_t, 2e-5, name + " identity codebooks")
    for nt1, nl1 in ((2, 150), (16, 40)):   # (T = 16: the <4, 4, 4> form)
        w1 = np.ones((1, 1), np.complex64)
        got = tr.beam_taps(ONE, ONE, w1, w1, FS, nl1, l_min=l_min, dt=dt, num_times=nt1).cpu().numpy()
        want = tr.taps(FS, nl1, l_min=l_min, dt=dt, num_times=nt1).cpu().numpy()
        assert got.shape == (tr.nrx, tr.ntx, 1, 1, 2, nt1, nl1)
        BU.check(got, want.astype(np.complex128)[:, :, None, None], S, w1, w1, 2e-5, name + " single unit beam")
    tr.close()


@pytest.mark.parametrize("nt", [1, 2])
def test_dtft_of_the_beam_taps_is_the_beam_channel(nt):
    """single TX, every delay at least M taps inside the window: the DTFT of the taps at |f| <= f_s / 4 is
    Tracer.beam_channel at f_c + f with the same f_a, elements and codebooks (as tests/test_gpu_array_taps.py does it
    for the array taps: the sinc tails cut at M taps, plus twice the float bound)"""
    c = K.small(K.C3_DOPPLER, 20000)
    tr = _tracer(c)
    assert tr.ntx == 1
    tr.trace()
    lam = _lam(c)
    rxe, txe = _ula(2, lam / 2), _upa(2, 2, lam / 2)
    wr, wt = BU.random_weights(2, 2, 1), BU.random_weights(3, 4, 2)
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    fs, M = FS, 2000
    x = T["tau"] * fs
    lo, hi = int(np.floor(x.min())), int(np.ceil(x.max()))
    l_min, nl = lo - M, (hi - lo) + 2 * M
    fc, dt = tr.f_ghz * 1e9, 1e-4
    h = tr.beam_taps(rxe, txe, wr, wt, fs, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy().astype(np.complex128)
    nk = 33
    f = -fs / 4 + np.arange(nk) * (fs / 2 / (nk - 1))
    H = tr.beam_channel(rxe, txe, wr, wt, fc - fs / 4, fs / 2 / (nk - 1), nk, dt=dt, num_times=nt).cpu().numpy()
    tr.close()
    l = l_min + np.arange(nl, dtype=np.float64)
    dtft = h @ np.exp(-2j * np.pi * np.outer(l, f) / fs)
    scale = 2 * math.sqrt(2) / (math.pi * (M - 1)) + 2e-5
    assert scale <= 2e-3
    err = np.abs(dtft - H).reshape(*H.shape[:5], -1).max(axis=-1)
    lim = BU.bound(S, wr, wt, scale)
    assert (err <= lim).all(), (err / lim).max()


# ------------------------------------------------------------------ 3. parts, polarisations, LoS classes
@pytest.mark.parametrize("name,n", [("C3", 20000), ("C4_DOPPLER", 4000), ("COINCIDENT", 8000)])
def test_parts_and_los_classes(name, n):
    """LoS + scatter, LoS only, scatter only, with a blocked and a coincident LoS entry forced where the trace has
    none; both polarisations are checked by the bound (it is per polarisation)"""
    c = _cfg(name, n)
    tr = _tracer(c)
    tr.trace()
    _force_los_classes(tr)
    combos = _combos(c)[:2]
    nl, l_min, nt, dt = 24, -2, 2, 1e-4
    t = dt * np.arange(nt)
    for los, scatter in PARTS:
        T = BU.terms_of(tr, los, scatter)
        S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
        for (cname, rxe, txe, wr, wt), h in zip(combos, _direct(tr, T, combos, nl, l_min, t)):
            got = tr.beam_taps(rxe, txe, wr, wt, FS, nl, l_min, dt=dt, num_times=nt, los=los,
                               scatter=scatter).cpu().numpy()
            BU.check(got, h, S, wr, wt, what="%s %s %s" % (name, cname, (los, scatter)))
            if los and not scatter:   # TE = TM on the LoS
                assert np.array_equal(got[:, :, :, :, 0], got[:, :, :, :, 1])
    tr.close()


# a clear LoS of 30 m in the street canyon (TX above the cars): the SIGN_CFG of tests/test_gpu_beam_channel.py
SIGN_CFG = K.cfg("simple_street_canyon_with_cars.hrt", [[-10.0, 1.0, 3.0]], [[-40.0, 0.0, 5.0]], 3.5, 2000, 1)


def test_exact_tap_line_of_sight():
    """LoS only at a sampling rate with f_s tau_LoS an integer (tau is a float32 M 2^e: f_s = 2^-e, f_s tau = M
    exactly): one tap holds a e^{j phase} G, every other tap is exactly zero"""
    tr = _tracer(dict(SIGN_CFG))
    tr.trace()
    L = tr.los()[0, 0]
    assert int(L[0:1].view(np.uint32)[0]) == 2 and L[2] * C0 >= 20.0
    mant, exp = math.frexp(float(L[2]))
    M, fs = int(mant * (1 << 24)), 2.0 ** (24 - exp)
    assert fs * float(L[2]) == float(M) and 0 < M <= 1 << 24
    lam = _lam(SIGN_CFG)
    rxe, txe = _random(7, 4 * lam, 11), _upa(3, 5, lam / 2)
    wr, wt = BU.random_weights(3, 7, 1), BU.random_weights(5, 15, 2)
    nl, l_min, nt, dt = 5, M - 4, 2, 1e-4
    got = tr.beam_taps(rxe, txe, wr, wt, fs, nl, l_min, dt=dt, num_times=nt, scatter=False).cpu().numpy()
    T = BU.terms_of(tr, True, False)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    h, = BT.beam_taps_direct(T, 1, 1, rxe, txe, [(wr, wt)], tr.f_ghz * 1e9, fs, tr.f_ghz * 1e9, nl, l_min,
                             dt * np.arange(nt))
    tr.close()
    BU.check(got, h, S, wr, wt, what="exact-tap LoS")
    assert (np.abs(h[..., 4]) > 0).any() and (got[..., :4] == 0).all() and (h[..., :4] == 0).all()
    assert (np.abs(got[..., 4]) > 0).any()


# ------------------------------------------------------------------ 4. structure
def test_shards_sum_accumulate_and_determinism():
    import torch
    c = K.small(K.C3, 30000)
    nl, l_min, nt, dt = 60, -3, 2, 1e-4
    combo = _combos(c)[1]
    _, rxe, txe, wr, wt = combo
    kw = dict(l_min=l_min, dt=dt, num_times=nt)
    tr = _tracer(c)
    tr.trace()
    whole = tr.beam_taps(rxe, txe, wr, wt, FS, nl, **kw)
    again = tr.beam_taps(rxe, txe, wr, wt, FS, nl, **kw)
    assert torch.equal(whole.view(torch.float32), again.view(torch.float32))   # bit-identical
    out = torch.zeros_like(whole)
    tr.beam_taps(rxe, txe, wr, wt, FS, nl, out=out, accumulate=True, **kw)
    tr.beam_taps(rxe, txe, wr, wt, FS, nl, out=out, accumulate=True, **kw)
    assert torch.equal(out.view(torch.float32), (2 * whole).view(torch.float32))
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    h, = _direct(tr, T, [combo], nl, l_min, dt * np.arange(nt))
    BU.check(whole.cpu().numpy(), h, S, wr, wt, what="whole")
    tr.close()
    for world in (2, 3):
        acc = None
        for r in range(world):
            ts = _tracer(c, rank=r, world=world, chunk=64)
            ts.trace()
            acc = ts.beam_taps(rxe, txe, wr, wt, FS, nl, out=acc, accumulate=acc is not None, **kw)
            ts.close()
        BU.check(acc.cpu().numpy(), h, S, wr, wt, what="world %d" % world)   # LoS counted once


# ------------------------------------------------------------------ 5. drop-in entries
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
h = hermespy_rt.compute_beam_taps(c["scene_path"], np.array(c["rx_pos"], np.float32),
                                  np.array(c["tx_pos"], np.float32), np.array(c["rx_vel"], np.float32),
                                  np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]), len(c["tx_pos"]),
                                  c["num_paths"], c["num_bounces"], {fs!r}, {nl}, rxe, txe, wr, wt, l_min={l_min},
                                  dt={dt!r}, num_times={nt})
np.save(sys.argv[1], h)
st = lib.Stats()
spec = abi.taps_spec({fs!r}, {nl}, {l_min}, c["f_ghz"] * 1e9, 0.0, {dt!r}, {nt})
h2 = abi.run_compute_beam_taps(lib.load(), *K.args(c), spec, rxe, txe, wr, wt, stats=st)
assert np.array_equal(h.view(np.float32), h2.view(np.float32))
print("batches", int(st.num_batches))
"""


@pytest.mark.parametrize("batched", [False, True], ids=["one_batch", "batched"])
def test_compute_beam_taps_matches_tracer(tmp_path, batched):
    """the drop-in entry (pybind and C, bitwise equal) agrees with Tracer.beam_taps on C3 at 20 k rays, also when a
    small workspace budget cuts the call into several batches (a fresh child process runs the drop-ins)"""
    c = K.small(K.C3, 20000)
    nl, l_min, nt, dt = 40, -7, 2, 1e-4
    combo = _combos(c)[1]
    _, rxe, txe, wr, wt = combo
    tr = _tracer(c)
    tr.trace()
    want = tr.beam_taps(rxe, txe, wr, wt, FS, nl, l_min=l_min, dt=dt, num_times=nt).cpu().numpy()
    T = BU.terms_of(tr)
    S = BU.amplitude_sums(T, tr.nrx, tr.ntx)
    h, = _direct(tr, T, [combo], nl, l_min, dt * np.arange(nt))
    BU.check(want, h, S, wr, wt, what="tracer")
    env = dict(os.environ)
    if batched:   # a budget below one workspace of the whole launch set
        env["HRT_WORKSPACE_BYTES"] = str(int(tr.ws.numel()) * 2 // 3)
    tr.close()
    files = [tmp_path / n for n in ("h.npy", "rx.npy", "tx.npy", "wr.npy", "wt.npy")]
    for p, x in zip(files[1:], (rxe, txe, wr, wt)):
        np.save(p, x)
    code = _PYBIND_CALL.format(repo=REPO, fs=FS, nl=nl, l_min=l_min, dt=dt, nt=nt)
    p = subprocess.run([sys.executable, "-c", code] + [str(x) for x in files], env=env, capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    batches = int(p.stdout.split()[-1])
    assert batches >= 2 if batched else batches == 1
    got = np.load(files[0])
    BU.check(got, h, S, wr, wt, what="drop-in")
    BU.check(got, want.astype(np.complex128), S, wr, wt, 2e-5, "drop-in against the tracer")
