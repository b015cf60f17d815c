"""What the antenna-pattern tests share (hermespy_rt_amd.patterns, csrc/hrt_patterns.hip).

weight32() is a numpy float32 emulation of the kernel's evaluation sequence, step by step (rotation rows summed left to
right, hypotf / atan2f angles, the dipole from the components, the TR 38.901 element through exp2f, the bilinear table);
patterns.weight() is the float64 definition.  Their largest difference over cases() -- 10^5 random float32 unit
directions under random orientations, plus the poles, the axes and the +-180 degree seam of the local frame under
orientations whose products are exact -- relative to max(F, g 10^-3), is the FLOOR of a float32 evaluation.  The GPU
comparison allows TOL = 4 FLOOR: the margin is for the device's atan2f, hypotf, sinf and exp2f, which are within a few
ulp of the host's.

    FLOOR = 2e-5    (measured 1.46e-5 by tests/test_patterns_design.py, which asserts measured <= FLOOR <= 2 measured;
                     it is reached by the random 7 x 12 table, whose values near 0 are judged relative to g 10^-3; the
                     dipole reaches 3.5e-6, the TR 38.901 element 1.7e-6, the smooth 181 x 360 table 1.5e-6)
    TOL   = 8e-5

A weight is the float product of the two sides: with M = max(F, g 10^-3) >= F per side,
|w - F_rx F_tx| <= (2 TOL + TOL^2 + 2^-23) M_rx M_tx, which weight_tolerance() returns.

The wrong readings of the definition (WRONG) are each caught by the planted cases of wrong_reading_cases()."""
import numpy as np

from hermespy_rt_amd import patterns as P

FLOOR = 2e-5
TOL = 4 * FLOOR
REL_MIN = 1e-3      # errors are relative to max(F, g * REL_MIN)

f32 = np.float32
PI, HALF_PI, INV_PI, INV_2PI = f32(np.pi), f32(np.pi / 2), f32(1 / np.pi), f32(0.5 / np.pi)
DEG = f32(180 / np.pi)
DIPOLE, DIPOLE_POLE = f32(np.sqrt(1.64)), f32(np.sqrt(1.64) * np.pi / 4)
DB_TO_LOG2 = f32(np.log2(10) / 20)


# ------------------------------------------------------------------ the kernel's sequence in float32
def local32(R, u):
    u = np.asarray(u, f32)
    if R is None:
        return u[..., 0], u[..., 1], u[..., 2]
    R = np.asarray(R, f32)
    return tuple((R[..., k, 0] * u[..., 0] + R[..., k, 1] * u[..., 1]) + R[..., k, 2] * u[..., 2] for k in range(3))


def table32(values, theta, phi):
    v = np.asarray(values, f32)
    nz, na = v.shape
    tz = theta * (f32(nz - 1) * INV_PI)
    inside = (tz >= 0) & (tz < f32(nz - 1))
    i0 = np.where(inside, tz.astype(np.int64), np.where(tz >= f32(nz - 1), nz - 2, 0))
    sz = np.minimum(tz - i0.astype(f32), f32(1))
    ta = (phi + PI) * (f32(na) * INV_2PI)
    k0 = np.where((ta >= 0) & (ta < f32(2 * na)), ta.astype(np.int64), 0)
    sa = ta - k0.astype(f32)
    k0 = np.where(k0 >= na, k0 - na, k0)
    k1 = np.where(k0 + 1 == na, 0, k0 + 1)
    a = v[i0, k0] + sa * (v[i0, k1] - v[i0, k0])
    b = v[i0 + 1, k0] + sa * (v[i0 + 1, k1] - v[i0 + 1, k0])
    return a + sz * (b - a)


def weight32(pattern, R, u):
    """F(R u) of one side as the kernel evaluates it (float32 array)"""
    p = P.check(pattern)
    g = P.gain(p)
    x, y, z = local32(R, u)
    assert x.dtype == f32
    if p["kind"] == P.ISOTROPIC:
        return np.full(x.shape, g, f32)
    r = np.hypot(x, y)
    if p["kind"] == P.DIPOLE:
        n = np.hypot(r, z)
        s, c = r / n, np.abs(z) / n
        q = (s * s) / (f32(1) + c)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = ((g * DIPOLE) * np.sin(HALF_PI * q)) / s
        return np.where(s >= f32(P.DIPOLE_SIN_MIN), f, (g * DIPOLE_POLE) * s).astype(f32)
    theta, phi = np.arctan2(r, z), np.arctan2(y, x)
    if p["kind"] == P.TR38901:
        td, pd = theta * DEG, phi * DEG
        a, b = (td - f32(90)) / f32(65), pd / f32(65)
        av, ah = np.minimum(f32(12) * (a * a), f32(30)), np.minimum(f32(12) * (b * b), f32(30))
        A = np.minimum(av + ah, f32(30))
        out = g * np.exp2((f32(8) - A) * DB_TO_LOG2)
    else:
        out = g * table32(p["table"], theta, phi)
    assert out.dtype == f32
    return out


def scale(pattern, F):
    """max(F, g 10^-3): what an error of F is relative to"""
    return np.maximum(np.asarray(F, np.float64), float(P.gain(P.check(pattern))) * REL_MIN)


def weight_tolerance(rx, tx, f_rx, f_tx):
    """the tolerance of a device weight against F_rx F_tx (float64), see the module docstring"""
    return (2 * TOL + TOL * TOL + 2.0 ** -23) * scale(rx, f_rx) * scale(tx, f_tx)


# ------------------------------------------------------------------ patterns, orientations and directions of the tests
def smooth_table(nz=181, na=360):
    """a measured-looking pattern: a main lobe at boresight, side lobes in zenith and a back lobe above a -26 dB
    floor, smooth from node to node (a node-to-node step of s costs s * 1.5e-5 absolute in float32 at 360 nodes: the
    azimuth index itself has that rounding)"""
    th = np.pi * np.arange(nz) / (nz - 1)
    ph = -np.pi + 2 * np.pi * np.arange(na) / na
    t, p = np.meshgrid(th, ph, indexing="ij")
    v = 0.05 + np.sin(t) ** 2 * (0.6 + 0.4 * np.cos(p)) ** 2 * (0.8 + 0.2 * np.cos(6 * t))
    return v.astype(np.float32)


def random_table(nz, na, seed):
    return np.random.default_rng(seed).uniform(0.0, 2.0, (nz, na)).astype(np.float32)


def pattern_set():
    """name -> pattern: every kind, the smallest tables and the largest"""
    return {
        "isotropic": P.isotropic(3.0), "dipole": P.dipole(-2.0), "tr38901": P.tr38901(1.5),
        "table_2x1": P.table(np.array([[0.25], [1.5]], np.float32)), "table_2x3": P.table(random_table(2, 3, 1), 6.0),
        "table_5x1": P.table(random_table(5, 1, 2)), "table_7x12": P.table(random_table(7, 12, 3)),
        "table_181x360": P.table(smooth_table(), -1.0),
    }


def random_rotations(n, seed):
    """n random proper rotations, float32 [n, 3, 3] (QR of a normal matrix)"""
    rng = np.random.default_rng(seed)
    q, r = np.linalg.qr(rng.normal(size=(n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 0] *= np.linalg.det(q)[:, None]
    return np.ascontiguousarray(q.astype(np.float32))


def exact_rotations():
    """the 24 proper signed permutation matrices: R u is exact in float32, so a direction lands exactly on the
    poles, the axes and the seam of the local frame"""
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for sg in range(8):
            m = np.zeros((3, 3))
            for k in range(3):
                m[k, perm[k]] = -1.0 if sg >> k & 1 else 1.0
            if np.linalg.det(m) > 0:
                out.append(m)
    return np.ascontiguousarray(np.array(out, np.float32))


def special_local():
    """local-frame directions on the poles, the axes, the +-180 degree seam and just beside them (float32, not all
    of unit length: the angles are scale-invariant)"""
    e = 2.0 ** -20
    d = [(0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0),
         (-1, e, 0), (-1, -e, 0), (-1, e, 0.5), (-1, -e, -0.5), (-2, 0, 1), (-0.5, 0, -1),
         (e, 0, 1), (0, e, -1), (1, e, e), (3, 0, 4), (0, -3, 4), (1, 1, 1), (-1, -1, 0.25)]
    return np.array(d, np.float32)


def special_cases():
    """(R [n, 3, 3], u [n, 3]): every special local direction under every exact rotation (u = R^T d, exact)"""
    Rs, d = exact_rotations(), special_local()
    R = np.repeat(Rs, d.shape[0], axis=0)
    u = np.einsum("nji,nj->ni", R.astype(np.float64), np.tile(d, (Rs.shape[0], 1)).astype(np.float64))
    return R, u.astype(np.float32)


def random_directions(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    return (u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)


def cases(n=100000, seed=11):
    """(R, u) pairs of the floor: n random unit directions under random orientations, then special_cases()"""
    R0, u0 = random_rotations(n, seed), random_directions(n, seed + 1)
    R1, u1 = special_cases()
    return np.concatenate([R0, R1]), np.concatenate([u0, u1])


def measured_floor(n=100000):
    """name -> the largest |weight32 - weight| / max(F, g 10^-3) over cases(n)"""
    R, u = cases(n)
    out = {}
    for name, p in pattern_set().items():
        ref = P.weight(p, R, u)
        out[name] = float((np.abs(weight32(p, R, u).astype(np.float64) - ref) / scale(p, ref)).max())
    return out


# ------------------------------------------------------------------ wrong readings of the definition
def weight_variant(pattern, R, u, transposed=False, inward=False, power=False, nowrap=False, horizon=False):
    """patterns.weight() written out again (float64), with the wrong readings as switches"""
    p = P.check(pattern)
    g = 10.0 ** (p["gain_db"] / (10.0 if power else 20.0))
    R = np.broadcast_to(np.eye(3), np.shape(u)[:-1] + (3, 3)) if R is None else np.asarray(R, np.float64)
    if transposed:
        R = np.swapaxes(R, -1, -2)
    v = np.einsum("...ij,...j->...i", R, np.asarray(u, np.float64) * (-1.0 if inward else 1.0))
    theta = np.arctan2(np.hypot(v[..., 0], v[..., 1]), v[..., 2])
    phi = np.arctan2(v[..., 1], v[..., 0])
    if horizon:
        theta = np.abs(0.5 * np.pi - theta)
    if p["kind"] == P.ISOTROPIC:
        f = np.ones_like(theta)
    elif p["kind"] == P.DIPOLE:
        s = np.sin(theta)
        with np.errstate(divide="ignore", invalid="ignore"):
            f = np.sqrt(1.64) * np.where(s < 2.0 ** -12, 0.25 * np.pi * s, np.cos(0.5 * np.pi * np.cos(theta)) / s)
    elif p["kind"] == P.TR38901:
        a = np.minimum(np.minimum(12 * ((np.degrees(theta) - 90) / 65) ** 2, 30)
                       + np.minimum(12 * (np.degrees(phi) / 65) ** 2, 30), 30)
        f = 10.0 ** ((8.0 - a) / 20.0)
    else:
        t = np.asarray(p["table"], np.float64)
        nz, na = t.shape
        tz = theta * (nz - 1) / np.pi
        i0 = np.clip(np.floor(tz), 0, nz - 2).astype(int)
        sz = np.minimum(tz - i0, 1.0)
        ta = (phi + np.pi) * na / (2 * np.pi)
        k0 = np.floor(ta).astype(int)
        sa = ta - k0
        k0 = np.minimum(k0, na - 1) if nowrap else k0 % na
        k1 = np.minimum(k0 + 1, na - 1) if nowrap else (k0 + 1) % na
        a = t[i0, k0] + sa * (t[i0, k1] - t[i0, k0])
        b = t[i0 + 1, k0] + sa * (t[i0 + 1, k1] - t[i0 + 1, k0])
        f = a + sz * (b - a)
    return g * (f * f if power else f)


def link_weight(rx, tx, R_rx, R_tx, u_rx, u_tx, **wrong):
    """w = F_rx F_tx in float64; wrong: a switch of weight_variant, or swapped=True (the RX and TX patterns swapped)"""
    wrong = dict(wrong)
    if wrong.pop("swapped", False):
        rx, tx = tx, rx
    return weight_variant(rx, R_rx, u_rx, **wrong) * weight_variant(tx, R_tx, u_tx, **wrong)


WRONG = ("transposed", "inward", "power", "nowrap", "horizon", "swapped")


def wrong_reading_cases():
    """planted (rx, tx, R_rx, R_tx, u_rx, u_tx): a sector antenna against a coarse table with a step at the seam,
    yawed and pitched orientations (not symmetric), directions off the axes and beside the seam"""
    step = np.array([[0.2, 0.4, 0.6, 1.8], [0.3, 0.5, 0.7, 1.9], [0.1, 0.2, 0.9, 1.6]], np.float32)
    rx, tx = P.tr38901(2.0), P.table(step, -3.0)
    R_rx, R_tx = P.rotation(0.7, 0.3, 0.2), P.rotation(-1.1, -0.4, 0.5)
    local = np.array([(1, 0.3, 0.2), (0.5, -0.4, 0.6), (-1, 0.02, 0.3), (-1, -0.05, -0.2), (0.2, 0.9, -0.5)], np.float64)
    u_rx = (local @ R_rx.astype(np.float64)).astype(np.float32)     # R^T d: local direction d
    u_tx = (local[::-1] @ R_tx.astype(np.float64)).astype(np.float32)
    return rx, tx, R_rx, R_tx, u_rx, u_tx


# ------------------------------------------------------------------ planted workspaces on the device (GPU tests)
def c4_rx4(n):
    """the two-TX C4 with four receivers"""
    from . import configs as K
    c = K.small(K.C4, n)
    c["rx_pos"] = [list(p) for p in c["rx_pos"]] + [[-1.0, 3.0, 1.0], [3.0, -4.0, 2.0]]
    c["rx_vel"] = [[0.0, 0.0, 0.0]] * 4
    return c


def snapshot(tr):
    """the whole workspace as host bytes"""
    tr.torch.cuda.synchronize(tr.device)
    return tr.ws.cpu().numpy().copy()


def restore(tr, snap):
    tr.ws.copy_(tr.torch.from_numpy(snap).to(tr.device))
    tr.patterned = False
    tr.torch.cuda.synchronize(tr.device)


def apply(tr, rx=None, tx=None, R_rx=None, R_tx=None):
    """Tracer.set_patterns and Tracer.apply_patterns on the workspace as it is -> its bytes afterwards"""
    tr.set_patterns(rx, tx, R_rx, R_tx)
    tr.patterned = False
    tr.apply_patterns()
    return snapshot(tr)


def _field_index(tr, b, rx, f, i):
    """the float index within the workspace of field f of record (b, rx, i)"""
    L = tr.layout
    return (int(L.off_recs) + b * int(L.rec_block_bytes) + (rx * 9 + f) * tr.cap * 4) // 4 + i


def _per_endpoint(R, e):
    return None if R is None else np.asarray(R)[e] if np.asarray(R).ndim == 3 else np.asarray(R)


def check_applied(tr, before, after, T, rx, tx, R_rx, R_tx, exact=None, what=""):
    """The workspace bytes `after` are `before` with the amplitudes of the scatter terms of T (a term listed m times:
    weighted m times) and of the clear LoS entries weighted per the definition, and NOTHING else changed:

      * the four fields of a record share one w: each non-zero field f gives w = after / before (the planted
        amplitudes are +-1, +-2 or +-1/2: the division is exact), the zero fields stay zero;
      * |w - F_rx F_tx| <= weight_tolerance (exact=c: w == c to the bit instead);
      * every other byte of the workspace -- blocked records, the slots past a block's count, mask words, hit blocks,
        tau, DFS and direction fields, counts, LoS entries that are not clear, the trace's scratch -- is unchanged.

    Returns dict(w, ref, ratio): the device weights and the float64 ones per unique record, LoS entries last, and the
    largest |w - ref| / tolerance."""
    B, A = before.view(np.float32), after.view(np.float32)
    rx_p, tx_p = P.check(rx), P.check(tx)
    s = ~T["los"]
    key = np.stack([T["rx"][s], T["bounce"][s], T["index"][s]], axis=1)
    uk, first, mult = np.unique(key, axis=0, return_index=True, return_counts=True)
    t_rx, t_tx = T["rx"][s][first], T["tx"][s][first]
    R1 = None if R_rx is None else np.asarray(R_rx, np.float32).reshape(-1, 3, 3)[t_rx if np.ndim(R_rx) == 3 else 0 * t_rx]
    R2 = None if R_tx is None else np.asarray(R_tx, np.float32).reshape(-1, 3, 3)[t_tx if np.ndim(R_tx) == 3 else 0 * t_tx]
    f_rx, f_tx = P.weight(rx_p, R1, T["urx"][s][first]), P.weight(tx_p, R2, T["utx"][s][first])
    idx = np.stack([_field_index(tr, uk[:, 1], uk[:, 0], f, uk[:, 2]) for f in range(4)], axis=1)   # [n, 4]
    allowed = np.zeros(B.size, bool)
    allowed[idx.reshape(-1)] = True
    b0, a1 = B[idx].astype(np.float64), A[idx].astype(np.float64)
    nz = b0 != 0
    assert (nz.sum(axis=1) == 2).all(), "planted records have one non-zero part per polarisation"
    assert np.array_equal(a1[~nz], np.zeros((~nz).sum())), what + ": a zero amplitude field did not stay zero"
    with np.errstate(divide="ignore", invalid="ignore"):
        w4 = np.where(nz, a1 / b0, np.nan)
    w = np.nanmax(w4, axis=1)
    assert np.array_equal(np.nanmin(w4, axis=1), w) and np.isfinite(w).all(), \
        what + ": the four fields of a record do not share one weight"
    # the clear LoS entries
    los = (int(tr.layout.off_los) // 4 + np.arange(tr.nrx * tr.ntx) * 8)
    st = B[los].view(np.uint32)
    clear = np.nonzero(st == 2)[0]
    la = los[clear] + 1
    allowed[la] = True
    u = np.stack([B[los[clear] + 3 + k] for k in range(3)], axis=1).astype(np.float64)
    lr1 = _per_endpoint(R_rx, clear // tr.ntx)
    lr2 = _per_endpoint(R_tx, clear % tr.ntx)
    lf_rx, lf_tx = P.weight(rx_p, lr1, -u), P.weight(tx_p, lr2, u)
    with np.errstate(divide="ignore", invalid="ignore"):
        lw = A[la].astype(np.float64) / B[la].astype(np.float64)
    # nothing else changed
    changed = (before.view(np.uint32) != after.view(np.uint32))
    stray = np.nonzero(changed & ~allowed)[0]
    assert stray.size == 0, "%s: %d words outside the live amplitudes changed, first at byte %d" % (
        what, stray.size, 4 * int(stray[0]))
    ref = np.concatenate([(f_rx * f_tx) ** mult, lf_rx * lf_tx])
    tol = np.concatenate([weight_tolerance(rx_p, tx_p, f_rx, f_tx) * mult * np.maximum(f_rx * f_tx, 1.0) ** (mult - 1),
                          weight_tolerance(rx_p, tx_p, lf_rx, lf_tx)])
    got = np.concatenate([w, lw])
    if exact is not None:
        bad = np.nonzero(got != exact)[0]
        assert bad.size == 0, "%s: %d weights are not exactly %r, e.g. %r" % (what, bad.size, exact, got[bad[:4]])
    err = np.abs(got - ref)
    bad = np.nonzero(~(err <= tol))[0]
    assert bad.size == 0, "%s: %d of %d weights off by more than the tolerance, e.g. term %d: got %r want %r (tol %.3g)" % (
        what, bad.size, got.size, bad[0], got[bad[0]], ref[bad[0]], tol[bad[0]])
    return dict(w=got, ref=ref, ratio=float((err / tol).max(initial=0.0)), keys=uk, terms=first, clear=clear)


def weighted_terms(tr, T, before, rx, tx, R_rx, R_tx):
    """the planted terms of T with a_te and a_tm multiplied by the float64 weight() of their directions (the LoS terms
    of clear entries too; a coincident LoS term keeps a = 1), and the per-term tolerance of the weight"""
    rx_p, tx_p = P.check(rx), P.check(tx)
    R1 = None if R_rx is None else np.asarray(R_rx, np.float32).reshape(-1, 3, 3)[T["rx"] if np.ndim(R_rx) == 3 else 0 * T["rx"]]
    R2 = None if R_tx is None else np.asarray(R_tx, np.float32).reshape(-1, 3, 3)[T["tx"] if np.ndim(R_tx) == 3 else 0 * T["tx"]]
    f_rx, f_tx = P.weight(rx_p, R1, T["urx"]), P.weight(tx_p, R2, T["utx"])
    st = before.view(np.uint32)[int(tr.layout.off_los) // 4 + (T["rx"] * tr.ntx + T["tx"]) * 8]
    live = ~T["los"] | (st == 2)
    w = np.where(live, f_rx * f_tx, 1.0)
    U = {k: v.copy() for k, v in T.items()}
    U["a_te"], U["a_tm"] = T["a_te"] * w, T["a_tm"] * w
    return U, np.where(live, weight_tolerance(rx_p, tx_p, f_rx, f_tx), 0.0)
