"""Received signals of traced channels (Tracer.propagate, hrt_compute_received_signal,
hermespy_rt.compute_received_signal) on small problems: the composition with the taps families to the bit, the float64
per-path sum over Tracer.paths(), ray shards accumulated into one output, and the drop-in entries."""
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib
from hermespy_rt_amd import propagate as pg

from . import configs as K
from .pathsum_util import C0, _lam, _thin, _tracer, _ula
from .test_gpu_array_taps import _reference_lt

pytestmark = pytest.mark.gpu

FS = 30.72e6
L_TAPS, N = 16, 48
T_START = 1e-3
CONFIGS = {"C1": K.small(K.C1, 2000), "C4_DOPPLER": K.small(K.C4_DOPPLER, 4000)}


def _signal(ntx, nt, seed=1):
    rng = np.random.RandomState(seed)
    return (rng.standard_normal((ntx, nt, N)) + 1j * rng.standard_normal((ntx, nt, N))).astype(np.complex64)


def _elements(c):
    return _ula(2, _lam(c) / 2), _ula(3, _lam(c) / 2, axis=0)


def _l_min(c):
    """a window of taps that begins four taps before the shortest line of sight of the links"""
    d = min(np.linalg.norm(np.subtract(r, t)) for r in c["rx_pos"] for t in c["tx_pos"])
    return int(np.floor(FS * d / C0)) - 4


@pytest.fixture(scope="module", params=sorted(CONFIGS))
def traced(request):
    tr = _tracer(CONFIGS[request.param])
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    yield tr, CONFIGS[request.param]
    tr.close()


@pytest.mark.parametrize("S", [None, 1, 16])
def test_propagate_is_apply_taps_of_the_taps_family(traced, S):
    tr, c = traced
    torch = tr.torch
    l_min = _l_min(c)
    rxe, txe = _elements(c)
    n_out = pg.default_num_out(N, L_TAPS, l_min)
    M = pg.num_blocks(n_out, S)
    t0, dt = pg.block_times(FS, S, T_START)
    assert M == (1 if S is None else -(-n_out // S))
    assert (t0, dt) == ((T_START, 0.0) if S is None else (T_START + (S - 1) / (2 * FS), S / FS))
    kw = dict(l_min=l_min, t0=t0, dt=dt, num_times=M)
    wr = np.exp(2j * np.pi * np.outer(np.arange(2), np.arange(2)) / 2).astype(np.complex64)      # 2 RX beams
    wt = np.exp(2j * np.pi * np.outer(np.arange(2), np.arange(3)) / 3).astype(np.complex64)      # 2 TX beams
    for what in ("taps", "array_taps", "beam_taps"):
        if what == "taps":
            x = torch.from_numpy(_signal(tr.ntx, 1)[:, 0]).to(tr.device)
            h = tr.taps(FS, L_TAPS, **kw)
            y = tr.propagate(x, FS, L_TAPS, l_min, S, T_START)
            assert y.shape == (tr.nrx, 1, 2, n_out)
        elif what == "array_taps":
            x = torch.from_numpy(_signal(tr.ntx, 3)).to(tr.device)
            h = tr.array_taps(rxe, txe, FS, L_TAPS, **kw)
            y = tr.propagate(x, FS, L_TAPS, l_min, S, T_START, rx_elements=rxe, tx_elements=txe)
            assert y.shape == (tr.nrx, 2, 2, n_out)
        else:
            x = torch.from_numpy(_signal(tr.ntx, 2)).to(tr.device)
            h = tr.beam_taps(rxe, txe, wr, wt, FS, L_TAPS, **kw)
            y = tr.propagate(x, FS, L_TAPS, l_min, S, T_START, rx_elements=rxe, tx_elements=txe, rx_weights=wr,
                             tx_weights=wt)
            assert y.shape == (tr.nrx, 2, 2, n_out)
        want = tr.apply_taps(h, x, l_min, S, n_out)
        assert torch.equal(y.view(torch.float32), want.view(torch.float32)), what
        assert float(y.abs().max()) > 0, what


def test_per_sample_channel_matches_the_float64_path_sum(traced):
    """S = 1 on links thinned to a handful of records: y against the float64 sum over the paths, the phase taken per
    output sample and the sinc per tap.  Tolerance: the 1e-5 sum_p |a_p^pol| that tests/test_gpu_array_taps.py grants
    every tap, carried through sum |x| over the tap window of every TX port, plus error_bound of the propagation."""
    tr, c = traced
    torch = tr.torch
    _thin(tr, 6)
    l_min = _l_min(c)
    rxe, txe = _elements(c)
    x = _signal(tr.ntx, 3, seed=2)
    n_out = pg.default_num_out(N, L_TAPS, l_min)
    t0, dt = pg.block_times(FS, 1, T_START)
    t = t0 + np.arange(n_out) * dt
    h64, A = _reference_lt(tr, FS, l_min + np.arange(L_TAPS), t, rxe, txe)
    # every compared link has the LoS term or a record, and is heard
    P = {k: v.cpu().numpy() for k, v in tr.paths(nonzero_only=False).items()}
    for rx in range(tr.nrx):
        for tx in range(tr.ntx):
            records = int(((P["rx"] == rx) & (P["tx"] == tx) & P["unblocked"]).sum())
            los = int(tr.los()[rx, tx][0:1].view(np.uint32)[0]) in (0, 2)
            assert los or records >= 1, (rx, tx)
            assert (A[rx, tx] > 0).all()
    ref = pg.apply_taps_reference(h64, x, l_min, 1, n_out)
    assert (np.abs(ref).reshape(tr.nrx, -1).max(axis=1) > 0).all()
    y = tr.propagate(torch.from_numpy(x).to(tr.device), FS, L_TAPS, l_min, 1, T_START, rx_elements=rxe,
                     tx_elements=txe).cpu().numpy().astype(np.complex128)
    # |h - h64| <= 1e-5 A[rx, tx, pol] per tap -> sum_tx sum_j 1e-5 A sum_l |x[tx, j, n - l_min - l]|
    ones = np.ones((tr.nrx, tr.ntx, 2, 3, 2, 1, L_TAPS)) * (1e-5 * A)[:, :, None, None, :, None, None]
    tol = pg.apply_taps_reference(ones, np.abs(x), l_min, None, n_out).real
    tol = tol + pg.error_bound(h64, x, l_min, 1, n_out)
    err = np.maximum(np.abs(y.real - ref.real), np.abs(y.imag - ref.imag))
    live = tol > 0
    assert live.any() and not ref[~live].any() and not y[~live].any()
    print("largest error / tolerance: %.3f" % (err[live] / tol[live]).max())
    assert (err[live] <= tol[live]).all()


def test_two_ray_shards_accumulate_into_one_output():
    c = CONFIGS["C4_DOPPLER"]
    rxe, txe = _elements(c)
    x = _signal(2, 3, seed=3)
    whole = _tracer(c)
    whole.trace()
    torch = whole.torch
    l_min = _l_min(c)
    xd = torch.from_numpy(x).to(whole.device)
    kw = dict(rx_elements=rxe, tx_elements=txe)
    y = whole.propagate(xd, FS, L_TAPS, l_min, 16, T_START, **kw)
    n_out = y.shape[-1]
    M = pg.num_blocks(n_out, 16)
    t0, dt = pg.block_times(FS, 16, T_START)
    acc = None
    for r in range(2):
        ts = _tracer(c, rank=r, world=2, chunk=64)
        ts.trace()
        acc = ts.propagate(xd, FS, L_TAPS, l_min, 16, T_START, out=acc, accumulate=acc is not None, **kw)
        ts.close()
    # the taps are linear in the shards (the LoS term is rank 0's alone): what differs is float32 rounding
    hw = whole.array_taps(rxe, txe, FS, L_TAPS, l_min=l_min, t0=t0, dt=dt, num_times=M).cpu().numpy()
    bound = pg.error_bound(hw, x, l_min, 16, n_out)
    a, b = acc.cpu().numpy().astype(np.complex128), y.cpu().numpy().astype(np.complex128)
    err = np.maximum(np.abs(a.real - b.real), np.abs(a.imag - b.imag))
    live = bound > 0
    print("largest shard difference / error_bound: %.4f" % (err[live] / bound[live]).max())
    assert np.abs(b).max() > 0 and (err[live] <= bound[live]).all() and not err[~live].any()
    whole.close()


def _pybind():
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


@pytest.mark.parametrize("S", [None, 16])
def test_drop_in_entries_agree_with_the_tracer(S):
    c = CONFIGS["C4_DOPPLER"]
    rxe, txe = (e.astype(np.float32) for e in _elements(c))
    x = _signal(2, 3, seed=4)
    tr = _tracer(c)
    tr.trace()
    l_min = _l_min(c)
    want = tr.propagate(tr.torch.from_numpy(x).to(tr.device), FS, L_TAPS, l_min, S, T_START, rx_elements=rxe,
                        tx_elements=txe).cpu().numpy()
    tr.close()
    n_out = want.shape[-1]
    t0, dt = pg.block_times(FS, S, T_START)
    spec = abi.taps_spec(FS, L_TAPS, l_min, c["f_ghz"] * 1e9, t0, dt, pg.num_blocks(n_out, S))
    st = lib.Stats()
    got_c = abi.run_compute_received_signal(lib.load(), *K.args(c), spec, rxe, txe, x, samples_per_block=S, stats=st)
    got_py = _pybind().compute_received_signal(
        c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
        np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], len(c["rx_pos"]),
        len(c["tx_pos"]), c["num_paths"], c["num_bounces"], FS, L_TAPS, rxe, txe, x, l_min=l_min, samples_per_block=S,
        t_start=T_START)
    assert got_c.shape == want.shape == got_py.shape
    assert np.array_equal(got_c.view(np.uint32), got_py.view(np.uint32))   # the two drop-in entries: the same call
    assert int(st.num_batches) == 1
    assert np.array_equal(got_c.view(np.uint32), want.view(np.uint32))     # one batch: the tracer's records
    assert np.abs(want).max() > 0
