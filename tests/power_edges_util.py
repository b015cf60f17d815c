"""Bin-edge planting for the power profiles (Tracer.power_profiles): what tests/test_power_edges_design.py (no device)
and tests/test_gpu_power_edges.py share.

After PL.plant, plant_edges() overwrites the delay and the arrival direction of every unblocked scatter record, and
the delay and the direction of every clear LoS entry, with values that stand ON the bin edges of include/hermespy_rt.h
(hrt_compute_power_profiles), and returns the terms with tau, urx (and utx of LoS terms) updated.  Amplitudes and nu
stay as planted, so every power is dyadic and every histogram bin is an exact sum.  A record's classes are functions
of PL.mix(rx, tx, path, bounce, salt): every link gets every class, and the shards of one launch set plant what the
whole plants.  Only plant_edges() needs a device.

Delay classes (DELAY_CLASSES; tau = tau0 + k dtau, then `step` float32 neighbours up or down).  dtau = 49 2^-39 s:
k dtau is exact in float32 for 49 k < 2^24, the IEEE quotient (tau - tau0) / dtau is exactly k, and the product
(tau - tau0) (1 / dtau) falls below k for every k used here.  tau0 is 0 or 16 dtau (TAU0S).

Direction classes (DIRS): float32 components written as they are, not renormalised: the axes and poles with both
signs of every zero, u_z beyond +-1, u_z = +-0, u_z = +-1/2, the diagonals of the xy plane, directions 2^-30 rad
inside the azimuth wrap and beside the equator (float64 tells them from the edge by 2^20 ulps, float32 does not), and
generic directions well inside their bins on every grid of GRIDS.

References: edge_reference() applies the header's rules in float64 numpy; its `variant` argument applies one of the
wrong rules of VARIANTS instead (the negative controls)."""
import math

import numpy as np

from hermespy_rt_amd import abi

from . import planted as PL
from .pathsum_util import _azi, _zen

DTAU = 49 * 2.0 ** -39
TAU0S = (0.0, 16 * DTAU)
GRIDS = ((1, 1), (2, 4), (3, 5), (8, 8), (128, 128))
LDS = (1, 3, 64)
LD_GLOBAL = 6000            # 2 (Ld + 2 Nth Nph) 8 B is beyond the hist kernel's LDS budget on every grid
SMALL_K = (1, 2, 3, 4, 6, 7)   # k dtau (1 / dtau) < k

# (name, k as a function of Ld, float32 steps, kept in the window for Ld >= 1)
DELAY_CLASSES = (
    ("first", lambda ld: 0, 0),
    ("middle", lambda ld: ld // 2, 0),
    ("last", lambda ld: ld - 1, 0),
    ("end", lambda ld: ld, 0),               # x = Ld: outside
    ("first-", lambda ld: 0, -1),            # x in (-1, 0): outside
    ("first+", lambda ld: 0, +1),            # bin 0
    ("end-", lambda ld: ld, -1),             # bin Ld - 1
    ("end+", lambda ld: ld, +1),             # outside
    ("small", None, 0),                      # k from SMALL_K (mod Ld), by the hash
)

_E = 1.0 + 2.0 ** -23
_Z = (0.0, -0.0)


def _dirs():
    d = []
    for ax in range(3):                       # the axes and poles, every sign of the zeros
        for s in (1.0, -1.0):
            for z1 in _Z:
                for z2 in _Z:
                    u = [z1, z2]
                    u.insert(ax, s)
                    d.append(("axis", tuple(u)))
    for s in (1.0, -1.0):                     # |u_z| > 1: the clamp
        d += [("clamp", (0.0, 0.0, s * _E)), ("clamp", (0.25, -0.5, s * _E))]
    for z in _Z:                              # u_z = +-0: theta / pi Nth = Nth / 2
        d += [("equator", (0.75, 0.5, z)), ("equator", (-0.5, 0.75, z))]
    for s in (0.5, -0.5):                     # theta = pi / 3, 2 pi / 3
        d += [("third", (0.75, 0.25, s)), ("third", (-0.25, -0.75, s))]
    for sx in (1.0, -1.0):                    # phi = +-pi / 4, +-3 pi / 4
        for sy in (1.0, -1.0):
            for z in _Z:
                d.append(("diagonal", (sx, sy, z)))
    t = 2.0 ** -30                            # within 2^-30 rad of the wrap and of the equator: float32 cannot tell
    d += [("near", (-1.0, t, 0.0)), ("near", (-1.0, -t, 0.0)), ("near", (0.75, 0.5, t)), ("near", (0.75, 0.5, -t))]
    q = 2.0 ** -10                            # generic: multiples of 2^-10, well inside their bins on every grid
    d += [("generic", (301 * q, -590 * q, 781 * q)), ("generic", (289 * q, -589 * q, -787 * q)),
          ("generic", (238 * q, 556 * q, 826 * q)), ("generic", (377 * q, 521 * q, -797 * q))]
    return d


DIRS = _dirs()
DIR_U = np.array([u for _, u in DIRS], np.float32)      # [ND, 3]
assert np.array_equal(DIR_U.astype(np.float64), np.array([u for _, u in DIRS]))   # exact in float32


# ------------------------------------------------------------------ the planted values (pure)
def classes(T, salt=0):
    """(delay class, direction class, small-k pick) of every term, from the hash of its global identity"""
    h = PL.mix(T["rx"], T["tx"], T["path"], T["bounce"], salt)
    return ((h >> np.uint64(8)) % np.uint64(len(DELAY_CLASSES))).astype(np.int64), \
        ((h >> np.uint64(20)) % np.uint64(len(DIRS))).astype(np.int64), \
        ((h >> np.uint64(40)) % np.uint64(len(SMALL_K))).astype(np.int64)


def delay_k(dc, pick, ld):
    """the k of delay class dc (arrays)"""
    k = np.zeros(dc.shape, np.int64)
    for i, (_, fk, _) in enumerate(DELAY_CLASSES):
        k[dc == i] = fk(ld) if fk else 0
    small = np.asarray(SMALL_K)[pick] % ld
    return np.where(dc == len(DELAY_CLASSES) - 1, small, k)


def delay_value(k, step, tau0):
    """tau0 + k dtau as a float32 (exact), moved `step` float32 neighbours"""
    tau = np.asarray(tau0 + k * DTAU)
    t32 = tau.astype(np.float32)
    assert np.array_equal(t32.astype(np.float64), tau), "tau0 + k dtau not exact in float32"
    up = np.nextafter(t32, np.float32(np.inf))
    dn = np.nextafter(t32, np.float32(-np.inf))
    return np.where(step > 0, up, np.where(step < 0, dn, t32)).astype(np.float32)


def edge_values(T, ld, tau0, salt=0, neighbours=True, fixed=None):
    """T with tau and urx (LoS terms: utx, urx = -utx in float64, signed zeros as they fall) replaced by the edge
    classes; `fixed` marks terms left as they are (coincident LoS entries); neighbours=False sends the float32
    neighbour classes to their class without the step.  Returns (U, delay class, direction class)."""
    dc, ac, pick = classes(T, salt)
    k = delay_k(dc, pick, ld)
    step = np.asarray([c[2] for c in DELAY_CLASSES])[dc] * (1 if neighbours else 0)
    tau = delay_value(k, step, tau0).astype(np.float64)
    u = DIR_U[ac].astype(np.float64)
    keep = np.zeros(dc.shape, bool) if fixed is None else np.asarray(fixed, bool)
    los = T["los"] & ~keep
    U = {key: v.copy() for key, v in T.items()}
    U["tau"] = np.where(keep, T["tau"], tau)
    U["urx"] = np.where(keep[:, None], T["urx"], np.where(los[:, None], -u, u))
    U["utx"] = np.where(los[:, None], u, T["utx"])
    dc, ac = np.where(keep, -1, dc), np.where(keep, -1, ac)
    return U, dc, ac


def plant_edges(tr, T, ld, tau0, salt=0, neighbours=True):
    """write edge_values into tr's workspace (after PL.plant(tr) returned T); returns (U, delay class, dir class)"""
    torch = tr.torch
    st = PL.los_status(tr)
    rx, tx = np.maximum(T["rx"], 0), np.maximum(T["tx"], 0)
    fixed = T["los"] & (st[rx, tx] != 2)
    U, dc, ac = edge_values(T, ld, tau0, salt, neighbours, fixed)
    sc = ~T["los"]
    for b in np.unique(T["bounce"][sc]):
        s = np.nonzero(sc & (T["bounce"] == b))[0]
        n = int(T["index"][s].max()) + 1
        blk = tr.rec_block(int(b))
        recs = blk[:, :, :n].cpu().numpy().view(np.float32).copy()
        r, i = T["rx"][s], T["index"][s]
        recs[r, PL.REC_TAU, i] = U["tau"][s]
        for q in range(3):
            recs[r, PL.REC_DIRX + q, i] = U["urx"][s, q]
        blk[:, :, :n] = torch.from_numpy(recs.view(np.int32)).to(tr.device)
    L = PL.los_view(tr)
    Lh = L.cpu().numpy().copy()
    for j in np.nonzero(T["los"] & ~fixed)[0]:
        Lh[T["rx"][j], T["tx"][j], PL.LOS_TAU] = U["tau"][j]
        Lh[T["rx"][j], T["tx"][j], PL.LOS_DIRX:PL.LOS_DIRZ + 1] = U["utx"][j]
    L.copy_(torch.from_numpy(Lh).to(tr.device))
    torch.cuda.synchronize(tr.device)
    return U, dc, ac


# ------------------------------------------------------------------ the header's rules, and the wrong ones
VARIANTS = {
    "a": "truncation without x >= 0: x in (-1, 0) lands in delay bin 0",
    "b": "x <= Ld: delay index Ld is kept (the kernel's layout puts it on arrival bin 0)",
    "c": "azimuth index Nph clamped to Nph - 1",
    "d": "no min(.., Nth - 1): zenith index Nth dropped",
    "e": "no clamp of u_z: |u_z| > 1 dropped",
    "f": "x = (tau - tau0) * (1 / dtau)",
    "g": "bin coordinates formed in float32",
}


def delay_coord(tau, tau0, dtau, variant=None):
    if variant == "f":
        return (tau - tau0) * (1.0 / dtau)
    if variant == "g":
        return ((tau.astype(np.float32) - np.float32(tau0)) / np.float32(dtau)).astype(np.float64)
    return (tau - tau0) / dtau


def delay_bins(tau, tau0, dtau, ld, variant=None):
    """(bin, kept) of every delay"""
    x = delay_coord(tau, tau0, dtau, variant)
    if variant == "a":
        return np.trunc(x).astype(np.int64), (x > -1.0) & (x < ld)
    if variant == "b":
        return np.floor(x).astype(np.int64), (x >= 0) & (x <= ld)
    return np.floor(x).astype(np.int64), (x >= 0) & (x < ld)


def angle_bins(u, nth, nph, variant=None):
    """(zenith bin, azimuth bin, kept) of every direction"""
    keep = np.ones(u.shape[0], bool)
    if variant == "g":
        v = u.astype(np.float32)
        pi = np.float32(np.pi)
        zx = np.arccos(np.clip(v[:, 2], np.float32(-1), np.float32(1))) / pi * np.float32(nth)
        ax = (np.arctan2(v[:, 1], v[:, 0]) + pi) / (np.float32(2) * pi) * np.float32(nph)
        assert zx.dtype == np.float32 and ax.dtype == np.float32
        zi = np.minimum(np.floor(zx), nth - 1).astype(np.int64)
        ai = np.floor(ax).astype(np.int64)
        return zi, np.where(ai >= nph, 0, ai), keep
    if variant == "e":
        keep = np.abs(u[:, 2]) <= 1.0
    zi, zx = _zen(u, nth)
    ai, ax = _azi(u, nph)
    if variant == "c":
        ai = np.minimum(np.floor(ax).astype(np.int64), nph - 1)
    if variant == "d":
        keep = np.floor(zx) < nth
    return zi, ai, keep


def powers(T):
    return np.stack([np.abs(T["a_te"]) ** 2, np.abs(T["a_tm"]) ** 2], axis=1)


def edge_reference(T, nrx, ntx, tau0, dtau, ld, nth, nph, variant=None):
    """pdp [nrx, ntx, 2, ld], arrival and departure [nrx, ntx, 2, nth, nph] and outside [nrx, ntx, 2] (the power of
    the terms outside the delay window) by the header's rules in float64, or by VARIANTS[variant]; sums of dyadic
    powers: exact"""
    nl, link, p = nrx * ntx, PL.link_of(T, ntx), powers(T)
    kd, ok = delay_bins(T["tau"], tau0, dtau, ld, variant)
    spill = ok & (kd >= ld)          # (variant b only)
    ok = ok & ~spill
    out = {"pdp": np.zeros((nl, 2, ld)), "outside": np.zeros((nl, 2))}
    for q in range(2):
        out["pdp"][:, q] = np.bincount(link[ok] * ld + kd[ok], weights=p[ok, q], minlength=nl * ld).reshape(nl, ld)
        out["outside"][:, q] = np.bincount(link[~ok], weights=p[~ok, q], minlength=nl)
    for name, u in (("arrival", T["urx"]), ("departure", T["utx"])):
        zi, ai, keep = angle_bins(u, nth, nph, variant)
        H = np.zeros((nl, 2, nth * nph))
        for q in range(2):
            H[:, q] = np.bincount((link * nth * nph + zi * nph + ai)[keep], weights=p[keep, q],
                                  minlength=nl * nth * nph).reshape(nl, nth * nph)
            if name == "arrival":
                H[:, q, 0] += np.bincount(link[spill], weights=p[spill, q], minlength=nl)
        out[name] = H.reshape(nrx, ntx, 2, nth, nph)
    out["pdp"] = out["pdp"].reshape(nrx, ntx, 2, ld)
    out["outside"] = out["outside"].reshape(nrx, ntx, 2)
    return out


def check_edges(got, ref, what, keys=("pdp", "arrival", "departure"), T=None, ntx=None):
    """got[k] == ref[k] exactly for k in keys"""
    for k in keys:
        PL.check_close(np.asarray(got[k], np.float64), ref[k], 0.0, "%s %s" % (what, k), T, ntx)


def differs_per_link(ref, var, keys=("pdp", "arrival")):
    """[nrx, ntx] bool: the variant reference differs from the true one in at least one bin of the link"""
    d = np.zeros(ref["pdp"].shape[:2], bool)
    for k in keys:
        d |= (ref[k] != var[k]).reshape(d.shape + (-1,)).any(axis=-1)
    return d


# ------------------------------------------------------------------ the moments
MOMENTS = {abi.POWER_COUNT: "COUNT", abi.POWER_P: "P", abi.POWER_P_TAU: "P_TAU", abi.POWER_P_TAU2: "P_TAU2",
           abi.POWER_P_NU: "P_NU", abi.POWER_P_NU2: "P_NU2", abi.POWER_P_LOS: "P_LOS",
           abi.POWER_P_URX_X: "P_URX_X", abi.POWER_P_URX_Y: "P_URX_Y", abi.POWER_P_URX_Z: "P_URX_Z"}
TINY = 2.0 ** -140   # below this: the products of the float32 neighbours of tau = 0 (denormals)


def moment_terms(T):
    """{field: [terms, 2]} the summands of every moment that does not depend on u_tx, formed as the kernel forms
    them ((p tau) tau; every product exact in float64)"""
    p, tau, nu = powers(T), T["tau"][:, None], T["nu"][:, None]
    w = {abi.POWER_COUNT: np.ones_like(p), abi.POWER_P: p, abi.POWER_P_TAU: p * tau, abi.POWER_P_TAU2: p * tau * tau,
         abi.POWER_P_NU: p * nu, abi.POWER_P_NU2: p * nu * nu, abi.POWER_P_LOS: p * T["los"][:, None]}
    for c in range(3):
        w[abi.POWER_P_URX_X + c] = p * T["urx"][:, c:c + 1]
    return w


def sum_is_exact(w):
    """True where a float64 sum of w is exact in ANY order: every |w| >= TINY is a multiple of one quantum 2^e and
    sum |w| < 2^(e + 53), so every partial sum is representable; the terms below TINY (at most 2^-147 each, a few
    thousand of them) never reach half an ulp of a partial sum of the others (all above 2^-120 here), and a partial sum
    of them alone is exact, so they leave the rounded result where the others put it"""
    w = np.abs(np.asarray(w, np.float64).ravel())
    w = w[w >= TINY]
    if w.size == 0:
        return True
    m, e = np.frexp(w)
    mi = (m * 2.0 ** 53).astype(np.int64)
    low = e - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)   # exponent of the lowest set bit
    return float(w.sum()) < 2.0 ** (int(low.min()) + 52)   # (one bit of head room for the rounding of w.sum())


def moments_reference(T, nrx, ntx):
    """{field: (sum [nrx, ntx, 2] correctly rounded (math.fsum), exact [nrx, ntx, 2] bool, bound [nrx, ntx, 2])}:
    where `exact` the float64 sum is the same in any order (tolerance 0); elsewhere a float64 sum of N terms in any
    order is within (N - 1) 2^-53 sum |w| of the true sum (Higham, Accuracy and Stability, eq. 4.4), plus the half
    ulp of the rounded reference itself: `bound`"""
    link = PL.link_of(T, ntx)
    out = {}
    for f, w in moment_terms(T).items():
        s, ex, bd = np.zeros((nrx * ntx, 2)), np.zeros((nrx * ntx, 2), bool), np.zeros((nrx * ntx, 2))
        for lk in range(nrx * ntx):
            for q in range(2):
                v = w[link == lk, q]
                s[lk, q] = math.fsum(v)
                ex[lk, q] = sum_is_exact(v)
                bd[lk, q] = 0.0 if ex[lk, q] else v.size * 2.0 ** -53 * math.fsum(np.abs(v))
        out[f] = (s.reshape(nrx, ntx, 2), ex.reshape(nrx, ntx, 2), bd.reshape(nrx, ntx, 2))
    return out


def check_moments(got, T, nrx, ntx, want_exact=()):
    """every moment of MOMENTS within its bound (0 where the sum is exact in any order); the fields named in
    want_exact must be of the exact kind.  Returns the names of the fields that were checked at tolerance 0."""
    m = np.asarray(got["moments"], np.float64).reshape(nrx, ntx, 2, -1)
    exact = []
    for f, (ref, ex, bd) in moments_reference(T, nrx, ntx).items():
        if MOMENTS[f] in want_exact:
            assert ex.all(), "the planted sum of %s is not exact in every order" % MOMENTS[f]
        err = np.abs(m[..., f] - ref)
        err = np.where(np.isnan(err), np.inf, err)
        assert (err <= bd).all(), "power moment %s: off by %g (bound %g) at %s: got %r want %r" % (
            MOMENTS[f], err.max(), bd.max(), np.unravel_index(np.argmax(err - bd), err.shape),
            m[..., f].ravel().tolist(), ref.ravel().tolist())
        if ex.all():
            exact.append(MOMENTS[f])
    return exact
