"""What the equalizer tests share (hrt_channel_equalizer, csrc/hrt_equalizer.{h,hip}): the mirror of hrt_equalizer_form
and of the LDS layout, the float64 reference, a numpy float32 emulation of the kernel (the same sums in the same order:
per-lane partial sums over the rows r = l + g k, then the butterfly over the g lanes), the plantings whose results are
exact, the case list of the GPU tests, the three error measures and the wrong readings of the definition that the
design test shows the plantings to catch."""
import functools
import os

import numpy as np

from hermespy_rt_amd import equalize

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32

THREADS = 256
WORDS = 64
MAX_NT, MAX_NR = 16, 64
MAX_POINTS = 1 << 24
ZF, LMMSE = 0, 1
FLAG_W = 1
SINGULAR, NONFINITE = 1, 2
KINDS = {"zf": ZF, "lmmse": LMMSE}

# The constants of the three bounds of the GPU tests, in the units the measures carry (u kappa, u kappa, u; u =
# (Nr + Nt) 2^-24, kappa the float64 condition number of the factored matrix): 4 x the emulation's worst value over
# the GPU tests' own case list (master_cases under bounded(), both kinds), rounded up.  The emulation's worst values
# are EMULATION_WORST (weights: 5 x 4 LMMSE, near-parallel columns; sinr and residual: 1 x 1, whose residual measure
# divides by |h|^2 of a standard normal h); test_equalizer_design.py asserts both against the emulation.  The margin
# is for a device that rounds its partial sums differently.
EMULATION_WORST = (2.452, 2.044, 45.94)
TOL_W, TOL_SINR, TOL_RESIDUAL = 9.81, 8.18, 183.8
# the noise power of the bounded cases (LMMSE: lambda between the squares of the prescribed singular values)
NOISE = 2.0 ** -6

# (Nr, Nt) of the GPU tests: 1 x 1; for every switch of g in the form table the smallest shape at the larger g ((5, 4)
# g = 2, (7, 5) 4, (9, 7) 8, (9, 9) 16, (17, 11) 32, (33, 11) 64) and the shape one row below it, on the other side of
# the switch; 16 x 16, 17 x 16, 64 x 16; and 3 x 16 (with 8 x 9, Nr < Nt: LMMSE only)
SHAPES = ((1, 1), (4, 4), (5, 4), (6, 5), (7, 5), (8, 7), (9, 7), (8, 9), (9, 9), (16, 11), (17, 11), (32, 11),
          (33, 11), (16, 16), (17, 16), (64, 16), (3, 16))
MASTER = 264      # matrices per shape: the largest tensor's points


def form(nr, nt):
    """hrt_equalizer_form: the lanes per matrix (0 outside the limits)"""
    if nt < 1 or nt > MAX_NT or nr < 1 or nr > MAX_NR:
        return 0
    g = 1
    while g <= 64:
        if 2 * nt * (-(-nr // g) + -(-nt // g)) <= WORDS:
            return g
        g *= 2
    return 0


def lds_word(g, n, mk, region, k, c, part, tid):
    """the LDS word of entry (k, c, part) of thread tid: region 0 = the top block, 1 = T (which follows it)"""
    base = 0 if region == 0 else mk * n * 2 * THREADS
    return base + ((k * n + c) * 2 + part) * THREADS + tid


def owner(g, r, slot):
    """-> (thread, k) owning row r of the matrix in point slot `slot` of the workgroup"""
    return slot * g + r % g, r // g


def grids(nr, nt):
    """(links, T, K) of the GPU tests for a shape.  A tensor has 2 T K points per link (the polarisations), so the
    counts are even: the smallest tensor (2 points), one pair less than a workgroup's points, one pair more, and
    several links that leave a partial last group."""
    ppb = THREADS // form(nr, nt)
    out = [((1, 1), 1, 1)]
    if ppb > 2:
        out.append(((1, 1), 1, ppb // 2 - 1))
    out.append(((1, 1), 1, ppb // 2 + 1))
    out.append(((2, 2), 3, 11))
    return out


# ---------------------------------------------------------------- layouts

def to_batch(H):
    """[nrx, ntx, a, b, 2, T, K] -> [B, a, b], B in the order of the point index (rx, tx, pol, t, k)"""
    H = np.asarray(H)
    return np.ascontiguousarray(np.transpose(H, (0, 1, 4, 5, 6, 2, 3))).reshape((-1,) + H.shape[2:4])


def to_batch_vec(S):
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
    assert b <= len(mats)
    return from_batch(np.asarray(mats[:b], np.complex64), (nrx, ntx, 2, T, K))


def out_bytes(nrx, ntx, nr, nt, T, K, flags):
    pts = nrx * ntx * 2 * T * K
    return (pts * nt * nr * 8 if flags & FLAG_W else 0) + pts * nt * 4 + pts * 4


# ---------------------------------------------------------------- the float64 reference

def reference_batch(mats, noise, kind):
    """equalize.equalizer_reference on [B, Nr, Nt] -> W [B, Nt, Nr], sinr [B, Nt], status [B], cond [B]"""
    mats = np.asarray(mats)
    B = mats.shape[0]
    # (the layout wants two polarisations: the second is a copy)
    r = equalize.equalizer_reference(from_batch(np.concatenate([mats, mats]), (1, 1, 2, 1, B)), noise, kind)
    return (to_batch(r["W"])[:B], to_batch_vec(r["sinr"])[:B], r["status"].reshape(-1)[:B], r["cond"].reshape(-1)[:B])


# ---------------------------------------------------------------- the emulation

def _reduce(v, g):
    idx = np.arange(g)
    off = 1
    while off < g:
        v = v + v[:, idx ^ off]
        off *= 2
    return v[:, 0]


def _lane_norm2(Xr, Xi, c):
    a = np.zeros((Xr.shape[0], Xr.shape[2]), F)
    for k in range(Xr.shape[1]):
        xr, xi = Xr[:, k, :, c], Xi[:, k, :, c]
        a = a + (xr * xr + xi * xi)
    return a


def _lane_dot(Xr, Xi, p, q):
    re = np.zeros((Xr.shape[0], Xr.shape[2]), F)
    im = np.zeros((Xr.shape[0], Xr.shape[2]), F)
    for k in range(Xr.shape[1]):
        xr, xi, yr, yi = Xr[:, k, :, p], Xi[:, k, :, p], Xr[:, k, :, q], Xi[:, k, :, q]
        re = re + (xr * yr + xi * yi)
        im = im + (xr * yi - xi * yr)
    return re, im


def emulate_batch(mats, noise, kind, weights=True):
    """The kernel on [B, Nr, Nt] complex64 matrices in numpy float32 -> W [B, Nt, Nr] complex64 (None without
    weights), sinr [B, Nt] float32, status [B] uint32."""
    mats = np.asarray(mats, np.complex64)
    B, nr, n = mats.shape
    g = form(nr, n)
    mk, nk = -(-nr // g), -(-n // g)
    aug = kind == LMMSE
    n0 = F(noise)
    lam = n0 if aug else F(0)
    Ar, Ai = np.zeros((B, mk * g, n), F), np.zeros((B, mk * g, n), F)
    Ar[:, :nr], Ai[:, :nr] = mats.real, mats.imag
    Tr, Ti = np.zeros((B, nk * g, n), F), np.zeros((B, nk * g, n), F)
    Tr[:, np.arange(n), np.arange(n)] = 1
    Ar, Ai = Ar.reshape(B, mk, g, n), Ai.reshape(B, mk, g, n)
    Tr, Ti = Tr.reshape(B, nk, g, n), Ti.reshape(B, nk, g, n)

    def norm2(c):
        a = _lane_norm2(Ar, Ai, c)
        if aug:
            a = a + lam * _lane_norm2(Tr, Ti, c)
        return _reduce(a, g)

    with np.errstate(all="ignore"):
        nmax, nsum = np.zeros(B, F), np.zeros(B, F)
        for c in range(n):
            a = norm2(c)
            nmax = np.where(a > nmax, a, nmax)
            nsum = nsum + a
        bad = ~(nsum <= np.finfo(F).max)
        thr = (F(nr + n) * F(2.0 ** -23)) * np.sqrt(nmax)
        sing = np.zeros(B, bool)
        for j in range(n):
            rjj = np.sqrt(norm2(j))
            sing |= ~(rjj > thr)
            d = rjj[:, None, None]
            for X in (Ar, Ai, Tr, Ti):
                X[..., j] = X[..., j] / d
            for i in range(j + 1, n):
                rr, ri = _lane_dot(Ar, Ai, j, i)
                if aug:
                    tr, ti = _lane_dot(Tr, Ti, j, i)
                    rr, ri = rr + lam * tr, ri + lam * ti
                rr, ri = _reduce(rr, g)[:, None, None], _reduce(ri, g)[:, None, None]
                for Xr, Xi in ((Ar, Ai), (Tr, Ti)):
                    xr, xi = Xr[..., j], Xi[..., j]
                    Xr[..., i], Xi[..., i] = Xr[..., i] - (rr * xr - ri * xi), Xi[..., i] - (rr * xi + ri * xr)
        status = np.where(bad, NONFINITE, np.where(sing, SINGULAR, 0)).astype(np.uint32)
        T_r, T_i = Tr.reshape(B, nk * g, n), Ti.reshape(B, nk * g, n)
        W = None
        if weights:
            for i in range(n):
                for c in range(i, n):
                    tr, tm = T_r[:, i, c][:, None, None], T_i[:, i, c][:, None, None]
                    yr, yi = Ar[..., c], Ai[..., c]
                    pr, pi = tr * yr + tm * yi, tr * yi - tm * yr
                    if c == i:
                        Ar[..., i], Ai[..., i] = pr, pi
                    else:
                        Ar[..., i], Ai[..., i] = Ar[..., i] + pr, Ai[..., i] + pi
            Wh = (Ar.reshape(B, mk * g, n)[:, :nr] - 1j * Ai.reshape(B, mk * g, n)[:, :nr]).astype(np.complex64)
            W = np.ascontiguousarray(np.swapaxes(Wh, 1, 2))
            W[status != 0] = 0
        gii = np.zeros((B, n), F)
        for c in range(n):
            xr, xi = T_r[:, :n, c], T_i[:, :n, c]
            gii = gii + (xr * xr + xi * xi)
        sinr = F(1) / (n0 * gii) - (F(1) if aug else F(0))
        sinr = np.where((status != 0)[:, None], F(0), sinr).astype(F)
    return W, sinr, status


def emulate(H, noise, kind, weights=True):
    """emulate_batch on a device-layout tensor -> dict in the device layout"""
    H = np.asarray(H)
    lead = (H.shape[0], H.shape[1]) + H.shape[4:]
    W, sinr, status = emulate_batch(to_batch(H), noise, kind, weights)
    return {"W": None if W is None else from_batch(W, lead), "sinr": from_batch(sinr, lead),
            "status": status.reshape(lead)}


# ---------------------------------------------------------------- cases under the derived bounds

def _haar(rng, n, k):
    q, r = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    return (q * (np.diagonal(r) / np.abs(np.diagonal(r))))[:, :k]


@functools.lru_cache(maxsize=None)
def master_cases(nr, nt):
    """MASTER matrices [MASTER, Nr, Nt] complex64 of one shape and the kind of each: the tensors of the GPU tests are
    prefixes of this list, so the emulation of the list covers them all.  Kinds by index mod 4: 0 standard normal,
    1 prescribed singular values 1, 2^-4, 2^-8 (repeated in this order over min(Nr, Nt) values) in random unitaries,
    2 two columns differing by the factor 1 + 2^-12, as in the SVD's list: column 1 is column 0 times it, so the matrix
    is rank deficient to rounding -- regular under LMMSE, SINGULAR under ZF (bounded(), below), 3 column 1 = column 0
    plus 2^-12 times a standard normal column, which both kinds bound (2 and 3: Nt >= 2; else a standard normal
    matrix)."""
    rng = np.random.RandomState(2000 * nr + nt)
    n = min(nr, nt)
    mats = np.empty((MASTER, nr, nt), np.complex64)
    kinds = np.zeros(MASTER, np.int64)
    for b in range(MASTER):
        kind = b % 4
        if kind >= 2 and nt < 2:
            kind = 0
        if kind == 1:
            s = 2.0 ** (-4.0 * (np.arange(n) % 3))
            a = (_haar(rng, nr, n) * s) @ np.conj(_haar(rng, nt, n)).T
        else:
            a = rng.standard_normal((nr, nt)) + 1j * rng.standard_normal((nr, nt))
            if kind == 2:
                a[:, 1] = a[:, 0] * (1 + 2.0 ** -12)
            if kind == 3:
                a[:, 1] = a[:, 0] + 2.0 ** -12 * (rng.standard_normal(nr) + 1j * rng.standard_normal(nr))
        mats[b] = a
        kinds[b] = kind
    mats.setflags(write=False)
    kinds.setflags(write=False)
    return mats, kinds


def bounded(kinds, kind):
    """which matrices of master_cases a kind of equalizer bounds: all but the rank-deficient family under ZF, which
    must come out SINGULAR with exact zeros instead"""
    return np.ones(len(kinds), bool) if kind == LMMSE else kinds != 2


REPEATED_SHAPES = ((4, 4), (9, 7), (17, 16), (64, 16))
REPEATED_NOISE = 1.0


def repeated_cases(nr, nt):
    """24 standard normal matrices of master_cases; in the odd ones the last column repeats the first, and matrix 4 is
    H = 0: SINGULAR under ZF, regular under LMMSE (with the noise REPEATED_NOISE, where the bounds hold for all but
    H = 0, whose W and sinr are exact zeros) -> (mats, which are singular under ZF)"""
    mats, kinds = master_cases(nr, nt)
    m = np.array(mats[kinds == 0][:24])
    m[1::2, :, nt - 1] = m[1::2, :, 0]
    m[4] = 0
    sing = np.arange(24) % 2 == 1
    sing[4] = True
    return m, sing


def kinds_of(nr, nt):
    """the kinds a shape is tested under"""
    return (ZF, LMMSE) if nr >= nt else (LMMSE,)


def unit_roundoff(nr, nt):
    return (nr + nt) * 2.0 ** -24


def measures(mats, noise, kind, W, sinr):
    """The three measures of [B, ..] results against the float64 reference on the widened float32 input, per matrix:
    | W^ - W |_F / (| W |_F u kappa);  max_i | rho^_i - rho_i | / ((1 + rho_i) u kappa);  the residual
    | (H^H H + lambda I) W^ - H^H |_F / (| H |_F (| H |_F^2 + lambda) | W^ |_F u)."""
    A = np.asarray(mats, np.complex64).astype(np.complex128)
    B, nr, nt = A.shape
    Wr, sr, status, cond = reference_batch(np.asarray(mats, np.complex64), noise, kind)
    assert not status.any(), "a bounded case is singular in float64"
    u = unit_roundoff(nr, nt)
    lam = float(F(noise)) if kind == LMMSE else 0.0
    W, sinr = np.asarray(W).astype(np.complex128), np.asarray(sinr, np.float64)
    fro = lambda X: np.sqrt((np.abs(X) ** 2).sum((1, 2)))
    m_w = fro(W - Wr) / (fro(Wr) * u * cond)
    m_s = (np.abs(sinr - sr) / (1.0 + sr)).max(1) / (u * cond)
    AH = np.conj(np.swapaxes(A, 1, 2))
    res = (AH @ A + lam * np.eye(nt)) @ W - AH
    m_r = fro(res) / (fro(A) * (fro(A) ** 2 + lam) * fro(W) * u)
    return m_w, m_s, m_r


def check(mats, noise, kind, W, sinr, status, tol=None):
    """Everything the GPU tests ask of the results [B, ..] of bounded cases [B, Nr, Nt]: shapes, status 0, finite
    values, the three measures under their constants.  Raises AssertionError; returns the worst measures."""
    mats = np.asarray(mats)
    B, nr, nt = mats.shape
    tol = (TOL_W, TOL_SINR, TOL_RESIDUAL) if tol is None else tol
    assert W.shape == (B, nt, nr) and sinr.shape == (B, nt) and status.shape == (B,), (W.shape, sinr.shape)
    assert not np.asarray(status).any(), "a regular point is flagged"
    assert np.isfinite(W.view(np.float32)).all() and np.isfinite(sinr).all(), "results not finite"
    worst = []
    for name, x, t in zip(("weights", "sinr", "residual"), measures(mats, noise, kind, W, sinr), tol):
        worst.append(float(x.max()))
        assert worst[-1] <= t, "%s measure %.3g > %.3g (matrix %d)" % (name, worst[-1], t, int(x.argmax()))
    return worst


def same(a, b):
    """two result tuples agree to the bit"""
    return all((x is None and y is None) or
               np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip(a, b))


# ---------------------------------------------------------------- exact plantings (every intermediate a power of two)

def _unit(rng, shape):
    """entries from {1, -1, j, -j}"""
    return np.array([1, -1, 1j, -1j])[rng.randint(0, 4, shape)]


PLANT_SHAPES = ((1, 1), (4, 4), (5, 3), (6, 5), (9, 8), (16, 16), (17, 16), (64, 16))


def exact_cases():
    """[(name, kind, noise, mats [B, Nr, Nt] complex64, W [B, Nt, Nr] complex64, sinr [B, Nt] float32, status [B])]:
    matrices for which every intermediate of the kernel is a power of two times a unit, so every output is exact.
      zf permutation   one entry s 2^e per column, s from {+-1, +-j}, distinct rows, distinct e, N0 a power of two:
                       W the scaled conjugate transpose, sinr = 4^e / N0
      zf coupled       columns in pairs on disjoint rows, a_0 = alpha e_r0, a_1 = beta e_r0 + gamma e_r1 with
                       |beta| = |gamma|: R is not diagonal, G_00 = 2 / |alpha|^2 (not 1 / R_00^2), G_11 = 1 / |gamma|^2
      lmmse triple     three entries of magnitude 2^e per column on disjoint rows, N0 = 4^e: |a|^2 + lambda = 4^(e+1),
                       W = H^H / 4^(e+1), sinr = 3
      lmmse wide       Nr < Nt, Nr div 3 columns as in "lmmse triple" and zero columns elsewhere, N0 = 4^e: the zero
                       columns' rows of W are zero and their sinr is 0; the others' sinr is 3
      lmmse zero       H = 0: W = 0, sinr = 0, status 0"""
    rng = np.random.RandomState(78)
    out = []
    B = 12
    for nr, nt in PLANT_SHAPES:
        # zf permutation
        H = np.zeros((B, nr, nt), np.complex128)
        W = np.zeros((B, nt, nr), np.complex128)
        S = np.zeros((B, nt))
        n0 = 2.0 ** -3
        for b in range(B):
            rows = rng.permutation(nr)[:nt]
            e = rng.permutation(np.arange(-8, 8))[:nt]
            s = _unit(rng, nt)
            s[0] = (1j, -1j, 1, -1)[b % 4]
            H[b, rows, np.arange(nt)] = s * 2.0 ** e
            W[b, np.arange(nt), rows] = np.conj(s) * 2.0 ** -e
            S[b] = 4.0 ** e / n0
        out.append(("zf permutation %dx%d" % (nr, nt), ZF, n0, H, W, S))
        # zf coupled
        if nt >= 2:
            H = np.zeros((B, nr, nt), np.complex128)
            W = np.zeros((B, nt, nr), np.complex128)
            S = np.zeros((B, nt))
            n0 = 2.0
            for b in range(B):
                rows = rng.permutation(nr)[:nt]
                for p in range(0, nt - 1, 2):
                    r0, r1 = rows[p], rows[p + 1]
                    ea, eg = rng.randint(-6, 7, 2)
                    al, be, ga = _unit(rng, 3) * 2.0 ** np.array([ea, eg, eg])
                    H[b, r0, p], H[b, r0, p + 1], H[b, r1, p + 1] = al, be, ga
                    W[b, p, r0], W[b, p, r1], W[b, p + 1, r1] = 1 / al, -be / (al * ga), 1 / ga
                    S[b, p], S[b, p + 1] = 4.0 ** ea / (2 * n0), 4.0 ** eg / n0
                if nt % 2:
                    e = rng.randint(-6, 7)
                    s = _unit(rng, 1)[0]
                    H[b, rows[-1], nt - 1] = s * 2.0 ** e
                    W[b, nt - 1, rows[-1]] = np.conj(s) * 2.0 ** -e
                    S[b, nt - 1] = 4.0 ** e / n0
            out.append(("zf coupled %dx%d" % (nr, nt), ZF, n0, H, W, S))
        # lmmse triple
        if nr >= 3 * nt:
            for e in (-3, 2):
                H = np.zeros((B, nr, nt), np.complex128)
                for b in range(B):
                    rows = rng.permutation(nr)[:3 * nt].reshape(3, nt)
                    for t in range(3):
                        H[b, rows[t], np.arange(nt)] = _unit(rng, nt) * 2.0 ** e
                W = np.conj(np.swapaxes(H, 1, 2)) / 4.0 ** (e + 1)
                out.append(("lmmse triple %dx%d e=%d" % (nr, nt, e), LMMSE, 4.0 ** e, H, W, np.full((B, nt), 3.0)))
        # lmmse zero
        H = np.zeros((4, nr, nt), np.complex128)
        out.append(("lmmse zero %dx%d" % (nr, nt), LMMSE, 0.25, H, np.zeros((4, nt, nr), np.complex128),
                    np.zeros((4, nt))))
    for nr, nt in ((1, 2), (3, 16), (5, 8), (8, 9), (6, 7)):
        e = -2
        H = np.zeros((B, nr, nt), np.complex128)
        S = np.zeros((B, nt))
        for b in range(B):
            cols = rng.permutation(nt)[:nr // 3]
            rows = rng.permutation(nr)[:3 * len(cols)].reshape(3, len(cols))
            for t in range(3):
                H[b, rows[t], cols] = _unit(rng, len(cols)) * 2.0 ** e
            S[b, cols] = 3.0
        W = np.conj(np.swapaxes(H, 1, 2)) / 4.0 ** (e + 1)
        out.append(("lmmse wide %dx%d" % (nr, nt), LMMSE, 4.0 ** e, H, W, S))
    return [(name, kind, n0, H.astype(np.complex64), W.astype(np.complex64), S.astype(np.float32),
             np.zeros(len(H), np.uint32)) for name, kind, n0, H, W, S in out]


# (Nr, Nt, K) of the one-column plantings: 120 and 552 points for 15 and 272 entries
ONE_COLUMN = ((5, 3, 5), (17, 16, 23))


def one_column_case(nr, nt, links=(2, 3), T=2, K=5):
    """The one-hot tensors, one per output index, in one call: a device-layout tensor whose every point p has ONE
    nonzero column j = (p div Nr) mod Nt, with three units in the rows i, i + 1, i + 2 (mod Nr), i = p mod Nr, under
    LMMSE with N0 = 1: |a_j|^2 + lambda = 4, so W has the three entries conj(h) / 4 in row j of the same point, sinr is
    3 in stream j, and every other output is an exact zero.  (A single entry cannot be exact: |h|^2 + 4^e is a power
    of four only for |h|^2 = 3 4^e, and 3 is not a sum of two rational squares; under ZF a one-hot H is singular.)
    With more points than entries every (j, i), and so every output index, is hit.  Nr >= 3."""
    rng = np.random.RandomState(79)
    nrx, ntx = links
    B = nrx * ntx * 2 * T * K
    H = np.zeros((B, nr, nt), np.complex64)
    S = np.zeros((B, nt), np.float32)
    p = np.arange(B)
    i, j = p % nr, (p // nr) % nt
    for t in range(3):
        H[p, (i + t) % nr, j] = _unit(rng, B)
    W = (np.conj(np.swapaxes(H, 1, 2)) / 4).astype(np.complex64)
    S[p, j] = 3
    lead = (nrx, ntx, 2, T, K)
    return from_batch(H, lead), 1.0, from_batch(W, lead), from_batch(S, lead)


# ---------------------------------------------------------------- wrong readings of the definition

READINGS = ("w_not_conjugated", "w_stored_nr_nt", "lambda_added_for_zf", "lambda_left_out_for_lmmse",
            "lambda_squared", "missing_minus_one", "minus_one_for_zf", "gii_from_rii")


def reading(mats, noise, kind, wrong=None):
    """The definition in float64 on [B, Nr, Nt] -> W [B, Nt, Nr] (flat in that order), sinr [B, Nt]; `wrong` names one
    misreading (READINGS).  Only for the well-conditioned plantings: it goes through the Gram matrix."""
    A = np.asarray(mats).astype(np.complex128)
    B, nr, nt = A.shape
    lam = noise if kind == LMMSE else 0.0
    if wrong == "lambda_added_for_zf" and kind == ZF:
        lam = noise
    if wrong == "lambda_left_out_for_lmmse" and kind == LMMSE:
        lam = 0.0
    if wrong == "lambda_squared":
        lam = lam * lam
    AH = np.conj(np.swapaxes(A, 1, 2))
    M = AH @ A + lam * np.eye(nt)
    with np.errstate(all="ignore"):
        try:
            G = np.linalg.inv(M)
        except np.linalg.LinAlgError:
            G = np.full_like(M, np.nan)
        W = G @ AH
        gii = np.real(np.diagonal(G, axis1=1, axis2=2))
        if wrong == "gii_from_rii":
            aug = np.concatenate([A, np.broadcast_to(np.sqrt(lam) * np.eye(nt), (B, nt, nt))], 1)
            gii = 1.0 / np.abs(np.diagonal(np.linalg.qr(aug)[1], axis1=1, axis2=2)) ** 2
        one = 1.0 if kind == LMMSE else 0.0
        if wrong == "missing_minus_one":
            one = 0.0
        if wrong == "minus_one_for_zf" and kind == ZF:
            one = 1.0
        sinr = 1.0 / (noise * gii) - one
    if wrong == "w_not_conjugated":
        W = np.conj(W)
    if wrong == "w_stored_nr_nt":
        W = np.ascontiguousarray(np.swapaxes(W, 1, 2)).reshape(B, nt, nr)
    return W, sinr
