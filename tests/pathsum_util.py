"""What the GPU tests of the path-sum families (channel, array channel, taps, array taps, power profiles) share:
the tracer and configuration helpers, the grids and array geometries, the planted-workspace fixtures' helpers and
the float64 reference of the power statistics.  (Helpers about planted workspaces themselves are tests/planted.py.)"""
import numpy as np
import pytest

from hermespy_rt_amd import abi

from . import configs as K
from . import planted as PL
from . import scenes_gen as G

DF = 30e3
FS = 122.88e6
C0 = 299792458.0
F = abi.POWER_FIELDS
PARTS = ((True, True), (True, False), (False, True))


def _tracer(c, **kw):
    from hermespy_rt_amd.device import Tracer
    return Tracer(c["scene_path"], c["rx_pos"], c["tx_pos"], c["rx_vel"], c["tx_vel"], c["f_ghz"],
                  c["num_paths"], c["num_bounces"], **kw)


def _grid(c, nk):
    return c["f_ghz"] * 1e9 - (nk // 2) * DF   # f0: an OFDM grid of nk subcarriers around the carrier


def _cfg(name, n):
    c = K.IN_PLANE["canyon"] if name == "IN_PLANE_canyon" else K.ALL[name]
    return K.small(c, n) if n else c


def _los_status(L):
    return int(L[0:1].view(np.uint32)[0])


def _lam(c):
    return C0 / (c["f_ghz"] * 1e9)


def _ula(n, d, axis=1):
    e = np.zeros((n, 3))
    e[:, axis] = np.arange(n) * d
    return e


def _upa(n1, n2, d):
    e = np.zeros((n1 * n2, 3))
    e[:, 0] = np.repeat(np.arange(n1), n2) * d
    e[:, 2] = np.tile(np.arange(n2), n1) * d
    return e


def _random(n, radius, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-radius, radius, (n, 3)) / np.sqrt(3.0)


def _geometries(c):
    lam = _lam(c)
    return [("ula2_upa3x5", _ula(2, lam / 2), _upa(3, 5, lam / 2)),
            ("random7_ula2", _random(7, 4 * lam, 11), _ula(2, lam / 2, axis=0))]


ARRAY_CASES = [
    ("C1", None, 1, 100),
    ("C3", 20000, 1, 257),
    ("C4_DOPPLER", 4000, 4, 100),
    ("COINCIDENT", 8000, 1, 64),
    ("IN_PLANE_canyon", None, 1, 100),
]


def _room(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("planted") / "room.hrt")
    G.room_with_clutter(p, 120, seed=5)
    return G.cfg(p, [[3.0, 2.0, 1.5], [-5.0, 4.0, 2.0]], [[-10.0, -6.0, 3.0], [12.0, 5.0, 4.0]], 6000, 3,
                 tx_vel=[[1.0, 0.0, 0.0], [0.0, -2.0, 0.0]])


CONFIGS = {"C3": lambda f: K.small(K.C3, 20000), "C4_DOPPLER": lambda f: K.small(K.C4_DOPPLER, 4000),
           "COINCIDENT": lambda f: K.small(K.COINCIDENT, 8000), "room": _room}


def _traced(name, tmp_path_factory, **kw):
    c = CONFIGS[name](tmp_path_factory)
    tr = _tracer(c, **kw)
    if name == "room":
        assert tr.num_tri > 1024   # the live list is re-sorted between bounces
    tr.trace()
    tr.torch.cuda.synchronize(tr.device)
    return tr, c


def _expect_failure(check, T, what, records=None):
    """negative controls: check(T') must fail for T' = T changed in one record (`records`: (name, term index) pairs,
    default PL.control_records; x PL.MUTATIONS)"""
    for name, k in PL.control_records(T) if records is None else records:
        for how in PL.MUTATIONS:
            with pytest.raises(AssertionError):
                check(PL.mutate(T, k, how))
                print("%s: the check passed with record %s (%d) %s" % (what, name, k, how))


def _thin(tr, per_link, seed=3):
    """clear unblocked bits of tr's last trace until every link has at most about per_link unblocked records; the last
    unblocked record of every (block, rx) stays (PL.control_records picks it)"""
    torch = tr.torch
    counts = tr.counts()
    rng = np.random.default_rng(seed)
    blocks = []
    for b in range(tr.nb):
        n = int(counts[b + 1])
        if n == 0:
            continue
        ray = tr.hit_block(b)[PL.HIT_RAY, :n].cpu().numpy().astype(np.int64) & 0xFFFFFFFF
        tx, _ = tr.global_path(ray)
        ub = PL._mask_bits(tr, b, n)
        blocks.append((b, n, tx, ub))
    per = np.zeros((tr.nrx, tr.ntx), np.int64)
    for b, n, tx, ub in blocks:
        for rx in range(tr.nrx):
            per[rx] += np.bincount(tx[ub[rx]], minlength=tr.ntx)
    p = min(1.0, per_link / max(int(per.max()), 1))
    for b, n, tx, ub in blocks:
        keep = ub & (rng.random(ub.shape) < p)
        for rx in range(tr.nrx):
            i = np.nonzero(ub[rx])[0]
            if i.size:
                keep[rx, i[-1]] = True
        pad = (-n) % 64
        bits = np.pad(keep, ((0, 0), (0, pad))).reshape(tr.nrx, -1, 64).astype(np.uint64)
        words = (bits << np.arange(64, dtype=np.uint64)).sum(axis=-1, dtype=np.uint64)   # [nrx, ceil(n / 64)]
        m = tr.mask_block(b).view(torch.int64)   # [nrx, cap / 64]
        if n % 64:   # the bits at and beyond n of the last word stay as they are
            old = m[:, words.shape[1] - 1].cpu().numpy().view(np.uint64)
            words[:, -1] |= old & ~np.uint64((1 << (n % 64)) - 1)
        m[:, :words.shape[1]] = torch.from_numpy(words.view(np.int64)).to(tr.device)
    torch.cuda.synchronize(tr.device)


# ------------------------------------------------------------------ a. poison
def _bits(x):
    import torch
    x = torch.view_as_real(x) if x.is_complex() else x
    return x.contiguous().view(torch.uint8).clone()


def _force_los_classes(tr):
    """give the poison a blocked and a coincident LoS entry where the trace has none (changing a clear entry's status
    before the clean run: the kernels must then read nothing but that status)"""
    st = PL.los_status(tr)
    clear = [tuple(ix) for ix in np.argwhere(st == 2)]
    S = PL.los_view(tr).view(tr.torch.int32)
    for want in (1, 0):
        if not (st == want).any() and clear:
            rx, tx = clear.pop()
            S[int(rx), int(tx), PL.LOS_STATUS] = want
    tr.torch.cuda.synchronize(tr.device)


def _zen(u, n):
    x = np.arccos(np.clip(u[:, 2], -1.0, 1.0)) / np.pi * n
    return np.minimum(np.floor(x), n - 1).astype(np.int64), x


def _azi(u, n):
    x = (np.arctan2(u[:, 1], u[:, 0]) + np.pi) / (2 * np.pi) * n
    i = np.floor(x).astype(np.int64)
    return np.where(i >= n, 0, i), x


def _near_edge(x):
    return np.abs(x - np.rint(x)) < 1e-6


def power_reference(T, tau0, dtau, ld, nth, nph):
    """moments [L, 2, F], |moments| [L, 2, F], pdp [L, 2, ld], arrival / departure [L, 2, nth, nph], the count N
    [L] and the edge slack of arrival / departure [L, 2]"""
    nl, link, p = T["nlinks"], T["link"], T["p"]
    tau, nu, urx, utx = T["tau"], T["nu"], T["urx"], T["utx"]
    M = np.zeros((nl, 2, F))
    A = np.zeros((nl, 2, F))
    N = np.bincount(link, minlength=nl).astype(np.float64)

    def add(dst, w, idx=link, n=nl):
        return dst + np.bincount(idx, weights=w, minlength=n)

    for pol in range(2):
        q = p[:, pol]
        M[:, pol, abi.POWER_COUNT] = N
        A[:, pol, abi.POWER_COUNT] = N
        fields = {abi.POWER_P: q, abi.POWER_P_TAU: q * tau, abi.POWER_P_TAU2: q * tau * tau, abi.POWER_P_NU: q * nu,
                  abi.POWER_P_NU2: q * nu * nu, abi.POWER_P_LOS: q * T["los"]}
        for c in range(3):
            fields[abi.POWER_P_URX_X + c] = q * urx[:, c]
            fields[abi.POWER_P_UTX_X + c] = q * utx[:, c]
        for f, w in fields.items():
            M[:, pol, f] = add(0.0, w)
            A[:, pol, f] = add(0.0, np.abs(w))
    pdp = np.zeros((nl, 2, ld))
    if ld:
        x = (tau - tau0) / dtau
        ok = (x >= 0) & (x < ld)
        b = np.floor(x[ok]).astype(np.int64)
        for pol in range(2):
            pdp[:, pol] = np.bincount(link[ok] * ld + b, weights=p[ok, pol], minlength=nl * ld).reshape(nl, ld)
    arr = np.zeros((nl, 2, nth, nph))
    dep = np.zeros((nl, 2, nth, nph))
    slack = np.zeros((2, nl, 2))
    if nth:
        for k, (u, H) in enumerate(((urx, arr), (utx, dep))):
            zi, zx = _zen(u, nth)
            ai, ax = _azi(u, nph)
            edge = _near_edge(zx) | _near_edge(ax)
            for pol in range(2):
                H[:, pol] = np.bincount(link * nth * nph + zi * nph + ai, weights=p[:, pol],
                                        minlength=nl * nth * nph).reshape(nl, nth, nph)
                slack[k, :, pol] = np.bincount(link[edge], weights=p[edge, pol], minlength=nl)
    return M, A, pdp, arr, dep, N, slack


def power_check(got, ref, tag=""):
    """got against power_reference within float64 rounding.  The edge slack (the whole power of every term whose bin
    coordinate lies within 1e-6 of an edge) is for TRACED directions, where numpy's and the device's libm may fall on
    either side of an edge; it waives the rule at the edge itself.  tests/test_gpu_power_edges.py pins the edges: it
    plants records on them and compares every bin at tolerance 0."""
    M, A, pdp, arr, dep, N, slack = ref
    nl = M.shape[0]
    m = np.asarray(got["moments"]).reshape(nl, 2, F)
    P = M[:, :, abi.POWER_P]
    tol = 1e-9 * A + 1e-300
    tol[:, :, abi.POWER_P_UTX_X:abi.POWER_P_UTX_Z + 1] += 2.0 ** -22 * P[:, :, None]
    err = np.abs(m - M)
    assert (err <= tol).all(), (tag, "moments", np.unravel_index(np.argmax(err / tol), err.shape), (err / tol).max())
    hb = ((1e-12 + N * 2.0 ** -61)[:, None] * P)   # [L, 2]
    g = np.asarray(got["pdp"]).reshape(pdp.shape)
    e = np.abs(g - pdp).reshape(nl, 2, -1).max(axis=-1, initial=0.0)
    assert (e <= hb + 1e-300).all(), (tag, "pdp", (e / np.maximum(hb, 1e-300)).max())
    for k, (name, H) in enumerate((("arrival", arr), ("departure", dep))):
        g = np.asarray(got[name]).reshape(H.shape)
        e = np.abs(g - H).reshape(nl, 2, -1).max(axis=-1, initial=0.0)
        assert (e <= hb + slack[k] + 1e-300).all(), (tag, name, e.max(), (hb + slack[k]).max())
