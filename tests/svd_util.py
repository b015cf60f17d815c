"""What the SVD tests share (hrt_channel_svd, csrc/hrt_svd.{h,hip}): the mirror of hrt_svd_form and of the LDS layout,
a numpy float32 emulation of the kernel's rotation sequence (the same sums in the same order: per-lane partial sums
over the rows r = l + g k, then the butterfly over the g lanes), the case list of the GPU tests, the four error
measures and the checks that the design test proves against wrong results."""
import functools
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

THREADS = 256
WORDS = 64
MAX_SHORT, MAX_LONG = 16, 64
MAX_POINTS = 1 << 24
NOT_CONVERGED = 0xFFFFFFFF
WANT_U, WANT_V = 1, 2

# The sweep cap (csrc/hrt_svd.h HRT_SVD_MAX_SWEEPS): twice the emulation's worst sweep count over the case list, at
# least 16.  test_svd_design.py asserts both this and the constant below against the emulation.
MAX_SWEEPS = 16
# The constant in front of u = max(m, n) 2^-24 in the four bounds of the GPU tests: 4 x the emulation's worst value
# over the GPU tests' own case list (master_cases), rounded up.  The margin is for a device that orders its partial
# sums differently.
TOL_CONST = 14.1

# (Nr, Nt) of the GPU tests: every g, both orientations, rows that do not fill the lane group
SHAPES = ((1, 1), (1, 4), (4, 1), (2, 2), (3, 2), (2, 3), (5, 3), (4, 4), (8, 4), (8, 8), (16, 8), (16, 16), (17, 16),
          (32, 16), (64, 16), (16, 64), (64, 1))
# grid points per link and polarisation (T, K) of the GPU tests, with the links
GRIDS = (((2, 2), 1, 1), ((2, 2), 7, 9), ((2, 2), 1, 64), ((2, 2), 5, 13), ((1, 3), 9, 7))
MASTER = 8 * 65   # matrices per shape: the largest tensor's points


def form(nr, nt):
    """hrt_svd_form: the lanes per matrix (0 outside the limits)"""
    m, n = max(nr, nt), min(nr, nt)
    if n < 1 or n > MAX_SHORT or m > MAX_LONG:
        return 0
    g = 1
    while g <= 64:
        if 2 * n * (-(-m // g) + -(-n // g)) <= WORDS:
            return g
        g *= 2
    return 0


def lds_word(g, n, mk, region, k, c, part, tid):
    """the LDS word of entry (k, c, part) of thread tid: region 0 = A, 1 = V (which follows A)"""
    base = 0 if region == 0 else mk * n * 2 * THREADS
    return base + ((k * n + c) * 2 + part) * THREADS + tid


def owner(g, r, slot):
    """-> (thread, k) owning row r of the matrix in point slot `slot` of the workgroup"""
    return slot * g + r % g, r // g


# ---------------------------------------------------------------- layouts

def to_batch(H):
    """[nrx, ntx, Nr, Nt, 2, T, K] -> [B, Nr, Nt], B in the order of the point index (rx, tx, pol, t, k)"""
    H = np.asarray(H)
    return np.ascontiguousarray(np.transpose(H, (0, 1, 4, 5, 6, 2, 3))).reshape((-1,) + H.shape[2:4])


def to_batch_sigma(S):
    """[nrx, ntx, n, 2, T, K] -> [B, n]"""
    S = np.asarray(S)
    return np.ascontiguousarray(np.transpose(S, (0, 1, 3, 4, 5, 2))).reshape(-1, S.shape[2])


def from_batch(X, lead):
    """[B, a, b] -> [nrx, ntx, a, b, 2, T, K] with lead = (nrx, ntx, 2, T, K); [B, a] -> [nrx, ntx, a, 2, T, K]"""
    X = np.asarray(X)
    if X.ndim == 2:
        return np.ascontiguousarray(np.transpose(X.reshape(tuple(lead) + X.shape[1:]), (0, 1, 5, 2, 3, 4)))
    return np.ascontiguousarray(np.transpose(X.reshape(tuple(lead) + X.shape[1:]), (0, 1, 5, 6, 2, 3, 4)))


def tensor(mats, links, T, K):
    """the first links 2 T K matrices of `mats` [B, Nr, Nt] as a device-layout complex64 tensor"""
    nrx, ntx = links
    b = nrx * ntx * 2 * T * K
    return from_batch(np.asarray(mats[:b], np.complex64), (nrx, ntx, 2, T, K))


def out_bytes(nrx, ntx, nr, nt, T, K, want):
    pts = nrx * ntx * 2 * T * K
    n = min(nr, nt)
    return pts * n * 4 + (pts * nr * n * 8 if want & WANT_U else 0) + (pts * nt * n * 8 if want & WANT_V else 0) + pts * 4


def views(buf, nrx, ntx, nr, nt, T, K, want):
    """the regions of a flat uint8 numpy buffer: sigma, u, v (None where absent), sweeps"""
    pts = nrx * ntx * 2 * T * K
    n = min(nr, nt)
    o = 0
    sigma = buf[o:o + pts * n * 4].view(np.float32).reshape(nrx, ntx, n, 2, T, K)
    o += pts * n * 4
    u = v = None
    if want & WANT_U:
        u = buf[o:o + pts * nr * n * 8].view(np.complex64).reshape(nrx, ntx, nr, n, 2, T, K)
        o += pts * nr * n * 8
    if want & WANT_V:
        v = buf[o:o + pts * nt * n * 8].view(np.complex64).reshape(nrx, ntx, nt, n, 2, T, K)
        o += pts * nt * n * 8
    sweeps = buf[o:o + pts * 4].view(np.uint32).reshape(nrx, ntx, 2, T, K)
    return {"sigma": sigma, "u": u, "v": v, "sweeps": sweeps}


# ---------------------------------------------------------------- the emulation

def _reduce(v, g):
    idx = np.arange(g)
    off = 1
    while off < g:
        v = v + v[:, idx ^ off]
        off *= 2
    return v[:, 0]


def _norm2(Ar, Ai, c, g):
    a = np.zeros((Ar.shape[0], g), F)
    for k in range(Ar.shape[1]):
        xr, xi = Ar[:, k, :, c], Ai[:, k, :, c]
        a = a + (xr * xr + xi * xi)
    return _reduce(a, g)


def _rotate(Xr, Xi, p, q, cs, sr, si, mask):
    cs, sr, si, mask = (a[:, None, None] for a in (cs, sr, si, mask))
    xr, xi, yr, yi = Xr[..., p], Xi[..., p], Xr[..., q], Xi[..., q]
    nxr = cs * xr - (sr * yr + si * yi)
    nxi = cs * xi - (sr * yi - si * yr)
    nyr = (sr * xr - si * xi) + cs * yr
    nyi = (sr * xi + si * xr) + cs * yi
    Xr[..., p], Xi[..., p] = np.where(mask, nxr, xr), np.where(mask, nxi, xi)
    Xr[..., q], Xi[..., q] = np.where(mask, nyr, yr), np.where(mask, nyi, yi)


def emulate_batch(mats, floor_clause=True, null_rule=True, max_sweeps=None, stable=True):
    """The kernel on [B, Nr, Nt] complex64 matrices in numpy float32 -> sigma [B, n], u [B, Nr, n], v [B, Nt, n]
    (complex64), sweeps [B] (uint32).  floor_clause / null_rule / stable switch parts of the definition off (the
    design test's wrong results)."""
    mats = np.asarray(mats, np.complex64)
    B, nr, nt = mats.shape
    tall = nr >= nt
    A = mats if tall else np.conj(np.swapaxes(mats, 1, 2))
    m, n = A.shape[1:]
    g = form(nr, nt)
    mk, nk = -(-m // g), -(-n // g)
    cap = MAX_SWEEPS if max_sweeps is None else max_sweeps
    Ar = np.zeros((B, mk * g, n), F)
    Ai = np.zeros((B, mk * g, n), F)
    Ar[:, :m], Ai[:, :m] = A.real, A.imag
    Vr = np.zeros((B, nk * g, n), F)
    Vi = np.zeros((B, nk * g, n), F)
    Vr[:, np.arange(n), np.arange(n)] = 1
    Ar, Ai = Ar.reshape(B, mk, g, n), Ai.reshape(B, mk, g, n)
    Vr, Vi = Vr.reshape(B, nk, g, n), Vi.reshape(B, nk, g, n)
    tol, flo = F(m) * F(2.0 ** -24), F(m) * F(2.0 ** -23)
    sweeps = np.zeros(B, np.uint32)
    done = np.zeros(B, bool)
    with np.errstate(all="ignore"):
        for _ in range(cap):
            if done.all():
                break
            nmax, nsum = np.zeros(B, F), np.zeros(B, F)
            for c in range(n):
                a = _norm2(Ar, Ai, c, g)
                nmax = np.where(a > nmax, a, nmax)
                nsum = nsum + a
            bad = ~done & ~(nsum <= np.finfo(F).max)
            done |= bad
            sweeps[bad] = NOT_CONVERGED
            cfloor = (flo * flo) * nmax
            rot = np.zeros(B, np.int64)
            for p in range(n - 1):
                for q in range(p + 1, n):
                    al, be, gr, gi = (np.zeros((B, g), F) for _ in range(4))
                    for k in range(mk):
                        xr, xi, yr, yi = Ar[:, k, :, p], Ai[:, k, :, p], Ar[:, k, :, q], Ai[:, k, :, q]
                        al = al + (xr * xr + xi * xi)
                        be = be + (yr * yr + yi * yi)
                        gr = gr + (xr * yr + xi * yi)
                        gi = gi + (xr * yi - xi * yr)
                    al, be, gr, gi = (_reduce(x, g) for x in (al, be, gr, gi))
                    ag = np.sqrt(gr * gr + gi * gi)
                    skip = ag <= tol * (np.sqrt(al) * np.sqrt(be))
                    if floor_clause:
                        skip = skip | (al <= cfloor) | (be <= cfloor)
                    mask = ~done & ~skip
                    if not mask.any():
                        continue
                    rot += mask
                    zeta = (be - al) / (F(2) * ag)
                    t = np.where(zeta >= 0, F(1), F(-1)) / (np.abs(zeta) + np.sqrt(F(1) + zeta * zeta))
                    cs = F(1) / np.sqrt(F(1) + t * t)
                    sn = cs * t
                    sr, si = sn * (gr / ag), sn * (gi / ag)
                    _rotate(Ar, Ai, p, q, cs, sr, si, mask)
                    _rotate(Vr, Vi, p, q, cs, sr, si, mask)
            clean = ~done & (rot == 0)
            sweeps[~done & ~clean] += 1
            done |= clean
        sweeps[~done] = NOT_CONVERGED
        sg = np.stack([np.sqrt(_norm2(Ar, Ai, c, g)) for c in range(n)], 1)             # [B, n]
        key = np.where(np.isnan(sg), np.inf, sg)
        order = np.argsort(-key, axis=1, kind="stable")
        if not stable:   # (a wrong result for the design test: equal values by descending column index)
            order = n - 1 - np.argsort(-key[:, ::-1], axis=1, kind="stable")
        take = lambda X: np.take_along_axis(X.reshape(B, -1, n), order[:, None, :], 2)
        Lr, Li, Sr, Si = take(Ar)[:, :m], take(Ai)[:, :m], take(Vr)[:, :n], take(Vi)[:, :n]
        sg = np.take_along_axis(sg, order, 1)
        null = sg <= flo * sg[:, :1] if null_rule else np.zeros_like(sg, bool)
        Lr = np.where(null[:, None, :], F(0), Lr / sg[:, None, :])
        Li = np.where(null[:, None, :], F(0), Li / sg[:, None, :])
    long_, short = (Lr + 1j * Li).astype(np.complex64), (Sr + 1j * Si).astype(np.complex64)
    return sg, (long_ if tall else short), (short if tall else long_), sweeps


def emulate(H, **kw):
    """emulate_batch on a device-layout tensor -> dict in the device layout"""
    H = np.asarray(H)
    lead = (H.shape[0], H.shape[1]) + H.shape[4:]
    s, u, v, sw = emulate_batch(to_batch(H), **kw)
    return {"sigma": from_batch(s, lead), "u": from_batch(u, lead), "v": from_batch(v, lead),
            "sweeps": sw.reshape(lead)}


# ---------------------------------------------------------------- cases

def _unit(rng, shape):
    """entries from {1, -1, j, -j}"""
    return np.array([1, -1, 1j, -1j])[rng.randint(0, 4, shape)]


def _haar(rng, n, k):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return (q * (np.diagonal(r) / np.abs(np.diagonal(r))))[:, :k]


@functools.lru_cache(maxsize=None)
def master_cases(nr, nt):
    """MASTER matrices [MASTER, Nr, Nt] complex64 of one shape and the kind of each: the tensors of the GPU tests are
    prefixes of this list, so the emulation of the list covers them all.  Kinds by index mod 4: 0 standard normal,
    1 rank-one s t^H with entries from {+-1, +-j}, 2 two columns differing by a factor 1 + 2^-12 (n >= 2), 3
    prescribed sigma = (1, 2^-10, 2^-20) in random unitaries (n >= 3); where a kind needs more columns than the shape
    has, a standard normal matrix."""
    rng = np.random.RandomState(1000 * nr + nt)
    n = min(nr, nt)
    mats = np.empty((MASTER, nr, nt), np.complex64)
    kinds = np.zeros(MASTER, np.int64)
    for b in range(MASTER):
        kind = b % 4
        if (kind == 2 and n < 2) or (kind == 3 and n < 3):
            kind = 0
        if kind == 0:
            a = rng.standard_normal((nr, nt)) + 1j * rng.standard_normal((nr, nt))
        elif kind == 1:
            a = np.outer(_unit(rng, nr), np.conj(_unit(rng, nt)))
        elif kind == 2:
            a = rng.standard_normal((nr, nt)) + 1j * rng.standard_normal((nr, nt))
            if nr >= nt:
                a[:, 1] = a[:, 0] * (1 + 2.0 ** -12)
            else:
                a[1, :] = a[0, :] * (1 + 2.0 ** -12)
        else:
            s = np.zeros(n)
            s[:3] = (1, 2.0 ** -10, 2.0 ** -20)
            a = (_haar(rng, nr, n) * s) @ np.conj(_haar(rng, nt, n)).T
        mats[b] = a
        kinds[b] = kind
    mats.setflags(write=False)
    kinds.setflags(write=False)
    return mats, kinds


# ---------------------------------------------------------------- measures and checks

def unit_roundoff(nr, nt):
    return max(nr, nt) * 2.0 ** -24


def measures(mats, sigma, u, v):
    """The four measures of [B, ..] results against float64 numpy on the widened float32 input, per matrix:
    E_sigma = max |sigma^ - sigma| / sigma_0, the relative Frobenius reconstruction error (absolute for H = 0), the
    short side's | V^H V - I |_max and the long side's over its non-null columns."""
    A = np.asarray(mats, np.complex64).astype(np.complex128)
    B, nr, nt = A.shape
    n = min(nr, nt)
    s, u, v = np.asarray(sigma, np.float64), np.asarray(u).astype(np.complex128), np.asarray(v).astype(np.complex128)
    ref = np.linalg.svd(A, compute_uv=False)
    s0 = np.where(ref[:, :1] > 0, ref[:, :1], 1.0)
    e_sigma = np.abs(s - ref).max(1) / s0[:, 0]
    rec = np.einsum("bid,bd,bjd->bij", u, s, np.conj(v))
    nrm = np.sqrt((np.abs(A) ** 2).sum((1, 2)))
    e_rec = np.sqrt((np.abs(rec - A) ** 2).sum((1, 2))) / np.where(nrm > 0, nrm, 1.0)
    short, long_ = (v, u) if nr >= nt else (u, v)
    eye = np.eye(n)
    e_short = np.abs(np.einsum("bic,bid->bcd", np.conj(short), short) - eye).max((1, 2))
    live = s > max(nr, nt) * 2.0 ** -23 * s[:, :1]
    gram = np.einsum("bic,bid->bcd", np.conj(long_), long_) - eye
    gram = np.where(live[:, :, None] & live[:, None, :], gram, 0.0)
    e_long = np.abs(gram).max((1, 2))
    return e_sigma, e_rec, e_short, e_long


def check(mats, sigma, u, v, sweeps, const=None, relative=None):
    """Everything the GPU tests ask of the results [B, ..] of the matrices [B, Nr, Nt]: shapes; sigma finite, >= 0 and
    descending; every sweep count below the cap; the long side exactly zero in null columns; the four measures at most
    const u (the reconstruction measure only where relative[b]; elsewhere the absolute | sigma^ - sigma | / sigma_0
    bound stands alone).  Raises AssertionError; returns the worst measures in units of u."""
    mats = np.asarray(mats)
    B, nr, nt = mats.shape
    n = min(nr, nt)
    const = TOL_CONST if const is None else const
    assert sigma.shape == (B, n) and u.shape == (B, nr, n) and v.shape == (B, nt, n), (sigma.shape, u.shape, v.shape)
    assert np.isfinite(sigma).all() and (sigma >= 0).all(), "sigma not finite or negative"
    assert np.isfinite(u.view(np.float32)).all() and np.isfinite(v.view(np.float32)).all(), "vectors not finite"
    assert (sigma[:, :-1] >= sigma[:, 1:]).all(), "sigma not descending"
    assert (np.asarray(sweeps) < MAX_SWEEPS).all(), "a point reached the sweep cap"
    null = sigma <= F(max(nr, nt)) * F(2.0 ** -23) * sigma[:, :1]
    long_ = u if nr >= nt else v
    assert not (long_ != 0)[np.broadcast_to(null[:, None, :], long_.shape)].any(), "a null column is not zero"
    e = measures(mats, sigma, u, v)
    unit = unit_roundoff(nr, nt)
    worst = []
    for name, x, rel_only in (("sigma", e[0], False), ("reconstruction", e[1], True), ("short side", e[2], False),
                              ("long side", e[3], False)):
        if rel_only and relative is not None:
            x = np.where(relative, x, 0.0)
        worst.append(float(x.max()) / unit)
        assert worst[-1] <= const, "%s error %.3g u > %.3g u (matrix %d)" % (name, worst[-1], const, int(x.argmax()))
    return worst


def same(a, b):
    """two result dicts / tuples agree to the bit"""
    return all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


# ---------------------------------------------------------------- exact plantings (no rotation: tolerance 0)

def _hadamard(n):
    h = np.array([[1.0]])
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


def exact_cases():
    """[(name, mats [B, Nr, Nt] complex64, expected sigma / u / v)]: matrices whose columns (of the tall orientation)
    are orthogonal to the bit with norms that are exact floats, so no pair is rotated and every output is exact:
    generalised permutations (one entry from {+-1, +-j} 2^e per column of A, with zero columns, ties, H = 0 and 1 x 1)
    and Hadamard(4) / Hadamard(16) times such a diagonal."""
    rng = np.random.RandomState(77)
    out = []

    def expected(A, tall):
        """from the tall-orientation matrices [B, m, n] whose columns are orthogonal: sort, normalise, permute"""
        B, m, n = A.shape
        nrm = np.sqrt((np.abs(A.astype(np.complex128)) ** 2).sum(1))
        order = np.argsort(-nrm, axis=1, kind="stable")
        s = np.take_along_axis(nrm, order, 1)
        As = np.take_along_axis(A.astype(np.complex128), order[:, None, :], 2)
        null = s <= m * 2.0 ** -23 * s[:, :1]
        with np.errstate(all="ignore"):
            long_ = np.where(null[:, None, :], 0.0, As / s[:, None, :])
        short = np.zeros((B, n, n), np.complex128)
        short[np.arange(B)[:, None], order, np.arange(n)[None, :]] = 1.0
        long_, short, s = long_.astype(np.complex64), short.astype(np.complex64), s.astype(np.float32)
        return (s, long_, short) if tall else (s, short, long_)

    for nr, nt in ((1, 1), (4, 4), (5, 3), (3, 5), (16, 16), (64, 16), (2, 3)):
        tall = nr >= nt
        m, n = max(nr, nt), min(nr, nt)
        B = 24
        A = np.zeros((B, m, n), np.complex128)
        for b in range(B):
            rows = rng.permutation(m)[:n]
            mag = 2.0 ** rng.randint(-3, 4, n)
            if b % 3 == 1:
                mag[:] = mag[0]                      # ties: every column the same norm
            if b % 3 == 2 and n > 1:
                mag[rng.randint(0, n)] = 0.0         # a zero column (null)
            if b == 5:
                mag[:] = 0.0                         # H = 0
            A[b, rows, np.arange(n)] = _unit(rng, n) * mag
        H = A if tall else np.conj(np.swapaxes(A, 1, 2))
        out.append(("permutation %dx%d" % (nr, nt), H.astype(np.complex64), expected(A.astype(np.complex64), tall)))
    for size in (4, 16):
        B = 16
        A = np.zeros((B, size, size), np.complex128)
        for b in range(B):
            mag = 2.0 ** rng.randint(-3, 4, size)
            if b % 2:
                mag[:] = mag[0]
            A[b] = _hadamard(size) * (_unit(rng, size) * mag)[None, :]
        out.append(("hadamard %d" % size, A.astype(np.complex64), expected(A.astype(np.complex64), True)))
    return out
