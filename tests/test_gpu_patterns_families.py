"""The path-sum families on a workspace weighted by antenna patterns (hrt_apply_patterns), and the routes that apply them:
Tracer.set_patterns / apply_patterns and hrt_compute_set_patterns.

  a. constant tables (0.5 on RX, 2^-3 on TX: every live amplitude times exactly 2^-4): each of the nine families and
     propagate() returns exactly 2^-4 times its unweighted result, power sums and covariances 2^-8 times, bit for bit
     (scaling every term by a power of two scales every float product and sum exactly); the order of the dominant paths
     is unchanged.
  b. TR 38.901 elements with random orientations on the planted two-TX C4: channel and array_channel against the
     float64 sums of tests/planted.py over terms weighted by patterns.weight(); the tolerance those tests use
     (UNIT_TOL = 0.05) plus the weight tolerance times sum |a| of the link.
  c. traced workspaces: set_patterns + trace equals trace + apply_patterns to the bit; removing the patterns restores
     the unweighted bits; a second apply raises.
  d. drop-ins: hrt_compute_array_taps and compute_power_profiles under hrt_compute_set_patterns equal the Tracer route to
     the bit; compute_paths under the same setting equals its result without it, byte for byte."""
import sys

import numpy as np
import pytest

from hermespy_rt_amd import abi, lib
from hermespy_rt_amd import patterns as P

from . import configs as K
from . import patterns_util as U
from . import planted as PL
from .pathsum_util import _bits, _tracer

pytestmark = pytest.mark.gpu

UNIT_TOL = 0.05   # tests/test_gpu_pathsum_planted.py: float32 direct sums of unit-sized planted terms
RAYS = 3000
RXE = np.array([[0, 0, 0], [0, 0.002, 0], [0.001, 0, 0.002]], np.float32)
TXE = np.array([[0, 0, 0], [0.002, 0, 0]], np.float32)
HALF, EIGHTH = P.table(np.full((181, 360), 0.5, np.float32)), P.table(np.full((2, 1), 2.0 ** -3, np.float32))


@pytest.fixture(scope="module")
def planted():
    tr = _tracer(K.small(K.C4_DOPPLER, RAYS))
    tr.trace()
    T = PL.plant(tr)
    before = U.snapshot(tr)
    yield tr, T, before
    tr.close()


def _families(tr):
    """every family (and propagate) on the workspace as it is -> name -> device tensor"""
    torch = tr.torch
    wr = np.array([[1, 1j, -1], [0.5, 0, 0.25j]], np.complex64)
    wt = np.array([[1, -1j]], np.complex64)
    x = torch.from_numpy((np.arange(2 * 2 * 40).reshape(2, 2, 40) % 7 - 3 + 1j).astype(np.complex64)).to(tr.device)
    kw = dict(t0=0.0, dt=PL.DT, num_times=2)
    out = {
        "channel": tr.channel(PL.FC, PL.FS / 64, 64, **kw),
        "array_channel": tr.array_channel(RXE, TXE, PL.FC, PL.FS / 64, 16, **kw),
        "beam_channel": tr.beam_channel(RXE, TXE, wr, wt, PL.FC, PL.FS / 64, 16, **kw),
        "taps": tr.taps(PL.FS, 96, -3, fc=PL.FC, **kw),
        "array_taps": tr.array_taps(RXE, TXE, PL.FS, 48, -3, fc=PL.FC, **kw),
        "beam_taps": tr.beam_taps(RXE, TXE, wr, wt, PL.FS, 48, -3, fc=PL.FC, **kw),
        "propagate": tr.propagate(x, PL.FS, 48, l_min=-3, samples_per_block=50, rx_elements=RXE, tx_elements=TXE, fc=PL.FC),
    }
    pw = tr.power_profiles(-0.5 / PL.FS, 1.0 / PL.FS, 128, 3, 5)
    out.update(power_moments=pw["moments"].clone(), power_pdp=pw["pdp"].clone(), power_arrival=pw["arrival"].clone(),
               power_departure=pw["departure"].clone())
    cv = tr.array_covariance(RXE, TXE)
    out.update(cov_rx=cv["rx"].clone(), cov_tx=cv["tx"].clone())
    dm = tr.dominant_paths(16)
    out.update({"dominant_" + k: dm[k].clone() for k in ("kept", "eligible", "power", "path", "bounce", "tri", "a_te", "a_tm",
                                                         "tau", "freq_shift", "u_rx", "u_tx")})
    torch.cuda.synchronize(tr.device)
    return out


# ------------------------------------------------------------------ a. constant tables: exact powers of two
def _scaled(x, s):
    """x times the real s, part by part (a complex product would add b * 0 to the real part and lose the sign of a zero)"""
    import torch
    return torch.view_as_real(x) * s if x.is_complex() else x * s


def test_every_family_scales_by_exactly_two_to_the_minus_four(planted):
    tr, T, before = planted
    U.restore(tr, before)
    base = _families(tr)
    R_rx, R_tx = U.random_rotations(tr.nrx, 31), U.random_rotations(tr.ntx, 32)
    after = U.apply(tr, HALF, EIGHTH, R_rx, R_tx)
    U.check_applied(tr, before, after, T, HALF, EIGHTH, R_rx, R_tx, exact=2.0 ** -4)
    got = _families(tr)
    s4, s8 = 2.0 ** -4, 2.0 ** -8
    for name in ("channel", "array_channel", "beam_channel", "taps", "array_taps", "beam_taps", "propagate",
                 "dominant_a_te", "dominant_a_tm"):
        assert bool(base[name].abs().max() > 0), name
        assert tr.torch.equal(_bits(got[name]), _bits(_scaled(base[name], s4))), name
    for name in ("power_pdp", "power_arrival", "power_departure", "cov_rx", "cov_tx", "dominant_power"):
        assert bool(base[name].abs().max() > 0), name
        assert tr.torch.equal(_bits(got[name]), _bits(_scaled(base[name], s8))), name
    m0, m1 = base["power_moments"], got["power_moments"]
    assert tr.torch.equal(m1[..., abi.POWER_COUNT], m0[..., abi.POWER_COUNT])
    rest = [f for f in range(abi.POWER_FIELDS) if f != abi.POWER_COUNT]
    assert tr.torch.equal(_bits(m1[..., rest]), _bits(m0[..., rest] * s8))
    # the dominant paths: the same paths in the same order
    for name in ("kept", "eligible", "path", "bounce", "tri", "tau", "freq_shift", "u_rx", "u_tx"):
        assert tr.torch.equal(_bits(got["dominant_" + name]), _bits(base["dominant_" + name])), name
    assert bool((base["dominant_kept"] > 1).any())


# ------------------------------------------------------------------ b. sector antennas against float64
def test_channel_and_array_channel_sum_the_weighted_terms(planted):
    tr, T, before = planted
    rx, tx = P.tr38901(), P.tr38901(-2.0)
    R_rx, R_tx = U.random_rotations(tr.nrx, 41), U.random_rotations(tr.ntx, 42)
    U.restore(tr, before)
    U.apply(tr, rx, tx, R_rx, R_tx)
    W, wtol = U.weighted_terms(tr, T, before, rx, tx, R_rx, R_tx)
    link = PL.link_of(T, tr.ntx)
    extra = float(np.bincount(link, weights=wtol * np.maximum(np.abs(T["a_te"]), np.abs(T["a_tm"]))).max())
    # (0.07 here: some 1600 terms a link, each weight known to 1.6e-4 of max(F, g 10^-3) per side)
    nk, nt, df = 16, 2, PL.FS / 4096
    f, t = PL.FC + np.arange(nk) * df, np.arange(nt) * PL.DT
    got = tr.channel(PL.FC, df, nk, 0.0, PL.DT, nt).cpu().numpy()
    e1 = PL.check_close(got, PL.channel_direct(W, tr.nrx, tr.ntx, f, t), UNIT_TOL + extra, "weighted channel", W, tr.ntx)
    fa = tr.f_ghz * 1e9
    got = tr.array_channel(RXE, TXE, PL.FC, df, nk, 0.0, PL.DT, nt).cpu().numpy()
    e2 = PL.check_close(got, PL.array_direct(W, tr.nrx, tr.ntx, RXE, TXE, fa, f, t), UNIT_TOL + extra, "weighted array",
                        W, tr.ntx)
    print("weighted channel / array: max |err|", e1, e2, "weight slack", extra)
    # the unweighted terms do not pass: the patterns matter by far more than the tolerance
    with pytest.raises(AssertionError):
        PL.check_close(got, PL.array_direct(T, tr.nrx, tr.ntx, RXE, TXE, fa, f, t), UNIT_TOL + extra, "unweighted")
    # nor do the terms with one record's weight left out
    k = PL.control_records(T)[0][1]
    one = {key: v.copy() for key, v in W.items()}
    one["a_te"][k], one["a_tm"][k] = T["a_te"][k], T["a_tm"][k]
    if abs(W["a_te"][k] - T["a_te"][k]) > 2 * (UNIT_TOL + extra):
        with pytest.raises(AssertionError):
            PL.check_close(got, PL.array_direct(one, tr.nrx, tr.ntx, RXE, TXE, fa, f, t), UNIT_TOL + extra, "one")


# ------------------------------------------------------------------ c. traced workspaces: the Tracer's two routes
def _taps(tr):
    return _bits(tr.taps(122.88e6, 64, -4, dt=1e-4, num_times=2))


def test_trace_applies_the_patterns_and_apply_patterns_does_the_same():
    c = K.small(K.C4_DOPPLER, RAYS)
    tr = _tracer(c)
    rx, tx = P.tr38901(1.0), U.pattern_set()["table_181x360"]
    R_rx, R_tx = U.random_rotations(tr.nrx, 51), U.random_rotations(tr.ntx, 52)
    tr.trace()
    plain = _taps(tr)
    assert not tr.patterned
    # route 1: patterns set, trace() applies them (timed and untimed, and the retrace inside counts())
    tr.set_patterns(rx, tx, R_rx, R_tx)
    assert not tr.patterned
    tr.trace()
    assert tr.patterned
    one = _taps(tr)
    ws1 = U.snapshot(tr)
    tr.trace(timed=True)
    assert tr.patterned and tr.torch.equal(_taps(tr), one)
    with pytest.raises(RuntimeError, match="already weighted"):
        tr.apply_patterns()
    # route 2: a plain trace, then apply_patterns()
    tr.set_patterns()
    tr.trace()
    assert not tr.patterned and tr.torch.equal(_taps(tr), plain)   # removing the patterns restores the unweighted bits
    tr.set_patterns(rx, tx, R_rx, R_tx)
    tr.apply_patterns()
    assert tr.patterned
    assert np.array_equal(U.snapshot(tr), ws1)
    assert tr.torch.equal(_taps(tr), one) and not tr.torch.equal(one, plain)
    with pytest.raises(RuntimeError, match="already weighted"):
        tr.apply_patterns()
    tr.set_patterns()
    tr.trace()
    assert tr.torch.equal(_taps(tr), plain)
    tr.close()


# ------------------------------------------------------------------ d. the drop-in entries
def _pybind():
    import hermespy_rt_amd
    sys.path.insert(0, hermespy_rt_amd.LIB_DIR)
    import hermespy_rt
    return hermespy_rt


def test_drop_ins_under_set_patterns_equal_the_tracer_route():
    c = K.small(K.C4_DOPPLER, RAYS)
    L = lib.load()
    rx, tx = P.tr38901(1.0), U.pattern_set()["table_7x12"]
    nrx, ntx = len(c["rx_pos"]), len(c["tx_pos"])
    R_rx, R_tx = U.random_rotations(nrx, 61), U.random_rotations(ntx, 62)
    # the Tracer with the drop-ins' launch tables (generated on the device): one batch, the same hit order
    tr = _tracer(c, device_dirs=True)
    tr.set_patterns(rx, tx, R_rx, R_tx)
    tr.trace()
    fc = c["f_ghz"] * 1e9
    want_taps = tr.array_taps(RXE, TXE, 122.88e6, 40, -4, fc=fc, dt=1e-4, num_times=2).cpu().numpy()
    want_pw = tr.power_profiles(0.0, 5e-9, 64, 3, 4)["buffer"].cpu().numpy()
    tr.set_patterns()
    tr.trace()
    plain_taps = tr.array_taps(RXE, TXE, 122.88e6, 40, -4, fc=fc, dt=1e-4, num_times=2).cpu().numpy()
    tr.close()
    spec = abi.taps_spec(122.88e6, 40, -4, fc, 0.0, 1e-4, 2)
    st = lib.Stats()
    with abi.compute_patterns(L, rx, tx, R_rx, R_tx):
        got = abi.run_compute_array_taps(L, *K.args(c), spec, RXE, TXE, stats=st)
    assert int(st.num_batches) == 1
    assert np.array_equal(got.view(np.float32), want_taps.view(np.float32))
    assert not np.array_equal(want_taps, plain_taps)
    # outside the block the setting is gone
    again = abi.run_compute_array_taps(L, *K.args(c), spec, RXE, TXE)
    assert np.array_equal(again.view(np.float32), plain_taps.view(np.float32))
    hermespy_rt = _pybind()
    a = (c["scene_path"], np.array(c["rx_pos"], np.float32), np.array(c["tx_pos"], np.float32),
         np.array(c["rx_vel"], np.float32), np.array(c["tx_vel"], np.float32), c["f_ghz"], nrx, ntx, c["num_paths"],
         c["num_bounces"])
    pat = dict(rx=rx, tx=tx, rx_orientation=R_rx, tx_orientation=R_tx)
    pw = hermespy_rt.compute_power_profiles(*a, 0.0, 5e-9, 64, 3, 4, patterns=pat)
    assert np.array_equal(pw["buffer"], want_pw)
    h = hermespy_rt.compute_array_taps(*a, 122.88e6, 40, RXE, TXE, l_min=-4, dt=1e-4, num_times=2, patterns=pat)
    assert np.array_equal(h.view(np.float32), want_taps.view(np.float32))
    h = hermespy_rt.compute_array_taps(*a, 122.88e6, 40, RXE, TXE, l_min=-4, dt=1e-4, num_times=2)
    assert np.array_equal(h.view(np.float32), plain_taps.view(np.float32))


def test_compute_paths_never_sees_the_setting():
    c = K.small(K.C4_DOPPLER, RAYS)
    L = lib.load()
    plain = abi.run_compute_paths(L, *K.args(c))
    plain_list = abi.run_compute_paths_list(L, *K.args(c))
    with abi.compute_patterns(L, P.tr38901(), P.dipole(), U.random_rotations(2, 71), U.random_rotations(2, 72)):
        under = abi.run_compute_paths(L, *K.args(c))
        under_list = abi.run_compute_paths_list(L, *K.args(c))
    def arrays(d, prefix=""):
        out = {}
        for k, v in d.items():
            if isinstance(v, dict):
                out.update(arrays(v, prefix + k + "."))
            elif isinstance(v, np.ndarray):
                out[prefix + k] = np.ascontiguousarray(v).view(np.uint8)
        return out

    for a, b in ((arrays(plain), arrays(under)), (arrays(plain_list), arrays(under_list))):
        assert len(a) >= 10 and a.keys() == b.keys()
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    assert (plain["scat"]["a_te_re"].view(np.uint32) != abi.SENTINEL_U32).any()
