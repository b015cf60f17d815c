"""The sinc weights of the three taps families (Tracer.taps, array_taps, beam_taps), read off the device tap by tap.

csrc/hrt_sinc.h produces every weight of the families, at six call sites: the MFMA partial kernel (the scatter route)
and the reduce kernel's LoS term (the LoS route) of each.  PL.plant_single leaves one live record per link with
amplitude 1 and, with fc = 0 and nu = 0, phase exactly 0: U = a, the MFMA adds 1 * w to zeros and the reduce adds
zeros, so out[rx, tx, 0, m, i].real is the bits of sinc_tap(l_min + i, sinc_prep(fs, tau)).  The 8 x 8 links of one
trace carry the delays of one entry of tests/sinc_util.py cases() at a time; every weight is held to
|got - ref| <= B 2^-24 |ref| + 2^-126 against the float64 reference (B: tests/sinc_util.py, derived from the floor
of a faithful emulation in tests/test_sinc_design.py), the six routes and num_times = 1 / 13 (K->rt == 1 / 4) to the
same bits.

Through the LoS route the amplitude a is real and TE = TM; through the scatter route a_tm = a_te / 2 and TM is half
of TE (exactly; below 2^-125 within one smallest normal float, where the half is a denormal)."""
import numpy as np
import pytest

from . import configs as K
from . import planted as PL
from . import sinc_util as S
from .pathsum_util import _tracer

pytestmark = pytest.mark.gpu

NL = 64
E0 = np.zeros((1, 3))
W1 = np.ones((1, 1), np.complex64)
ROUTES = ("scatter", "los")
FAMILIES = ("taps", "array_taps", "beam_taps")
CASES = S.cases()


def _trace():
    c = K.small(K.C5, 4096)
    c["num_bounces"] = 2
    tr = _tracer(c)
    assert tr.nrx * tr.ntx == NL
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    return tr, c


@pytest.fixture(scope="module")
def planted():
    tr, c = _trace()
    st = PL.plant_single(tr, np.zeros(NL, np.float32))
    yield tr, st, c
    tr.close()


def _call(tr, fs, l_min, L, T, route, fc=0.0, t0=0.0, dt=0.0):
    """the three families' outputs as numpy [NL, 2, T, L] complex64"""
    kw = dict(fs=fs, num_taps=L, l_min=l_min, fc=fc, t0=t0, dt=dt, num_times=T, los=route == "los",
              scatter=route == "scatter")
    out = (tr.taps(**kw), tr.array_taps(E0, E0, **kw)[:, :, 0, 0], tr.beam_taps(E0, E0, W1, W1, **kw)[:, :, 0, 0])
    return [o.cpu().numpy().reshape(NL, 2, T, L) for o in out]


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _weights(tr, st, fs, l_min, L, tag):
    """the weights [NL, L] float32 of one window: the six routes and both num_times to the same bits (the scatter
    route on the covered links), TM against TE, zero imaginary parts"""
    w = {}
    for route in ROUTES:
        links = st["covered"] if route == "scatter" else np.ones(NL, bool)
        for T in (1, 13):
            got = _call(tr, fs, l_min, L, T, route)
            te = got[0][:, 0].real
            for name, g in zip(FAMILIES, got):
                what = "%s %s %s T = %d" % (tag, name, route, T)
                assert np.array_equal(_bits(g[:, 0].real), _bits(te)), what + ": TE differs from taps'"
                assert (g.imag == 0).all(), what + ": imaginary part"
                tm = g[:, 1].real
                if route == "los":
                    assert np.array_equal(_bits(tm), _bits(te)), what + ": TM != TE"
                else:
                    big = np.abs(te) >= 2 * S.TINY
                    assert np.array_equal(tm[big], (0.5 * te)[big]), what + ": TM != TE / 2"
                    assert (np.abs(tm - 0.5 * te.astype(np.float64)) <= S.TINY).all(), what + ": TM != TE / 2"
                assert (g[~links] == 0).all(), what + ": a link without a live record"
            assert np.array_equal(_bits(te), _bits(np.broadcast_to(te[:, :1], te.shape))), \
                "%s %s T = %d: the rows differ" % (tag, route, T)
            w[route, T] = te[:, 0]
        assert np.array_equal(_bits(w[route, 1]), _bits(w[route, 13])), "%s %s: T = 1 and T = 13 differ" % (tag, route)
    c = st["covered"]
    assert np.array_equal(_bits(w["scatter", 1][c]), _bits(w["los", 1][c])), tag + ": scatter and LoS routes differ"
    return w["los", 1]


def test_the_live_records_are_spread(planted):
    """the condition of the scatter route: at least 48 of the 64 links have a live record; they lie in more than one
    hit block, at many positions of the 32-record batch and in all four kq groups (position mod 4)"""
    tr, st, c = planted
    cov = st["covered"]
    print("links with a live scatter record: %d of %d" % (cov.sum(), NL))
    assert cov.sum() >= 48
    assert np.unique(st["block"][cov]).size >= 2
    assert np.unique(st["ordinal"][cov] % 32).size >= 16
    assert np.unique(st["ordinal"][cov] % 4).size == 4
    assert np.unique(st["ordinal"][cov] // 512).size >= 4   # (spread over the link's records: over its chunks)


@pytest.mark.parametrize("cls", S.CLASSES)
def test_weights(planted, cls):
    tr, st, c = planted
    worst = 0.0
    for k, fs, tau, windows in CASES:
        if k != cls:
            continue
        tl = S.by_link(tau, NL)
        assert np.unique(np.arange(NL)[st["covered"]] % tau.size).size == tau.size   # every delay on a covered link
        PL.retau_single(tr, st, tl)
        for l_min, L in windows:
            tag = "class %s fs %.17g window (%d, %d)" % (cls, fs, l_min, L)
            w = _weights(tr, st, fs, l_min, L, tag)
            worst = max(worst, S.check(w, fs, tl, l_min + np.arange(L), S.B, what=tag))
    print("class %s: largest error of a weight %.2f x 2^-24 |w| (six routes, bound %d)" % (cls, worst, S.B))


def test_a_batch_of_one_record():
    """plant_single's second mode: the live record's mask bit alone, so that it is staged as a batch of one"""
    tr, c = _trace()
    k, fs, tau, windows = [e for e in CASES if e[0] == "a"][0]
    tl = S.by_link(tau, NL)
    st = PL.plant_single(tr, tl, only_live_bit=True)
    assert st["covered"].sum() >= 48
    for l_min, L in windows[:3]:
        for T in (1, 13):
            got = _call(tr, fs, l_min, L, T, "scatter")
            te = got[0][:, 0].real
            for g in got:
                assert np.array_equal(_bits(g[:, 0].real), _bits(te)) and (g.imag == 0).all()
                assert np.array_equal(g[:, 1].real, 0.5 * te)
            assert np.array_equal(_bits(te), _bits(np.broadcast_to(te[:, :1], te.shape)))
            S.check(te[st["covered"], 0], fs, tl[st["covered"]], l_min + np.arange(L), S.B, what="a batch of one")
    tr.close()


def test_phase_on(planted):
    """fc = the carrier, nu from PL.NUS, t = -5 DT + m DT: a cis(nu t - fc tau) w within (B + P) 2^-24 |a| |w|"""
    tr, st, c = planted
    fc = c["f_ghz"] * 1e9
    nu, t = S.phase_inputs(NL)
    worst = 0.0
    for cls, fs, tau, windows in CASES:
        if cls not in S.PHASE_CLASSES:
            continue
        tl = S.by_link(tau, NL)
        PL.retau_single(tr, st, tl, nu)
        e = S.phase_ref(nu, t, fc, tl)                               # [NL, T]
        for l_min, L in windows:
            w = S.sinc_ref(fs, tl, l_min + np.arange(L))                 # [NL, L]
            for route in ROUTES:
                links = st["covered"] if route == "scatter" else np.ones(NL, bool)
                got = _call(tr, fs, l_min, L, t.size, route, fc=fc, t0=t[0], dt=PL.DT)
                for pol, a in enumerate((1.0, 0.5 if route == "scatter" else 1.0)):
                    ref = a * e[:, :, None] * w[:, None, :]
                    tol = (S.B + S.P) * S.U * np.abs(ref) + S.TINY
                    for name, g in zip(FAMILIES, got):
                        err = np.abs(g[:, pol].astype(np.complex128) - ref)[links]
                        assert np.isfinite(err).all() and (err <= tol[links]).all(), \
                            ("class %s fs %r window (%d, %d) %s %s pol %d" % (cls, fs, l_min, L, name, route, pol),
                             float((err / tol[links]).max()))
                        big = np.abs(ref[links]) > 2.0 ** -100
                        worst = max(worst, float((err[big] / (S.U * np.abs(ref[links][big]))).max(initial=0.0)))
    print("phase on: largest error of a term %.2f x 2^-24 |a| |w| (bound %d)" % (worst, S.B + S.P))


def test_negative_controls_on_the_device_output(planted):
    """the device's weights fail the check against a reference scaled by 1 + 2^-19, against one with one link's
    delay moved by one float32 ulp, and against one with two links' delays exchanged"""
    tr, st, c = planted
    cls, fs, tau, windows = [e for e in CASES if e[0] == "c"][0]
    tl = S.by_link(tau, NL)
    PL.retau_single(tr, st, tl)
    l_min, L = windows[0]
    l = l_min + np.arange(L)
    got = _call(tr, fs, l_min, L, 1, "scatter")[0][:, 0, 0].real
    cov = st["covered"]
    S.check(got[cov], fs, tl[cov], l, S.B)
    with pytest.raises(AssertionError):
        S.check(got[cov], fs, tl[cov], l, S.B, ref_scale=1 + 2.0 ** -19)
    k = int(np.nonzero(cov & (np.arange(NL) % tau.size == 3))[0][0])   # (n = 105: the first delay past the switch)
    moved = tl.copy()
    moved[k] = np.nextafter(moved[k], np.float32(1.0))
    with pytest.raises(AssertionError):
        S.check(got[cov], fs, moved[cov], l, S.B)
    i, j = [int(np.nonzero(cov & (np.arange(NL) % tau.size == q))[0][0]) for q in (2, 5)]   # (n = 104 and 110)
    swapped = tl.copy()
    swapped[[i, j]] = tl[[j, i]]
    assert swapped[i] != tl[i]
    with pytest.raises(AssertionError):
        S.check(got[cov], fs, swapped[cov], l, S.B)
