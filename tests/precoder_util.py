"""What the precoder tests share (hrt_channel_precoder, csrc/hrt_precoder.{h,hip}): the mirror of hrt_precoder_form and of
the LDS layout, the float64 reference, a numpy float32 emulation of the kernel (the same sums in the same order:
per-lane partial sums over the rows r = l + g k, then the butterfly over the g lanes; the normalisation, the E stage
and the division included), the plantings whose results are exact, the case list of the GPU tests, the two error
measures and the wrong readings of the definition that the design test separates from the right result."""
import functools

import numpy as np

from hermespy_rt_amd import equalize, precode

from . import equalizer_util as EU
from .equalizer_util import REPO, from_batch, same, tensor, to_batch, to_batch_vec  # noqa: F401  (shared layouts)

F = np.float32

THREADS = 256
WORDS = 64
MAX_NR, MAX_NT = 16, 64
MAX_POINTS = 1 << 24
MRT, ZF, RZF = 0, 1, 2
TOTAL, STREAM = 0, 1
FLAG_P = 1
SINGULAR, NONFINITE = 1, 2
KIND_NAME = {MRT: "mrt", ZF: "zf", RZF: "rzf"}
NORM_NAME = {TOTAL: "total", STREAM: "stream"}
NORMS = (TOTAL, STREAM)

# The constants of the two bounds of the GPU tests, in the units the measures carry (u kappa; u = (Nr + Nt) 2^-24,
# kappa the float64 condition number of the factored matrix, 1 for MRT): 4 x the emulation's worst value over the GPU
# tests' own case list (configurations(): master_cases under bounded(), every kind and norm, and the heavily
# regularised set), rounded up.  The emulation's worst values are EMULATION_WORST (both at 4 x 4 under RZF and TOTAL);
# test_precoder_design.py asserts both against the emulation.  The margin is for a device that rounds its partial sums differently.
EMULATION_WORST = (1.669, 8.395)
TOL_P, TOL_SINR = 6.68, 33.58
# the noise power and the total power of the bounded cases; their RZF regularization is the default, Nr N0 / Ptot
NOISE = 2.0 ** -6
POWER = 1.0

# (Nr, Nt) of the GPU tests: the transpose of the equalizer's list, so that the factored matrix [H^H; sqrt(alpha) I]
# has the equalizer's shapes: 1 x 1; both sides of every switch of g; 16 x 16, 16 x 17, 16 x 64; and 16 x 3 (with
# 9 x 8, Nr > Nt: MRT and RZF only)
SHAPES = tuple((b, a) for a, b in EU.SHAPES)
MASTER = EU.MASTER


def form(nr, nt):
    """hrt_precoder_form: the lanes per matrix (0 outside the limits): the smallest power of two g with
    2 Nr (ceil(Nt / g) + ceil(Nr / g)) <= WORDS, the equalizer's rule for the (Nt + Nr) x Nr matrix that is factored"""
    if nr < 1 or nr > MAX_NR or nt < 1 or nt > MAX_NT:
        return 0
    g = 1
    while g <= 64:
        if 2 * nr * (-(-nt // g) + -(-nr // g)) <= WORDS:
            return g
        g *= 2
    return 0


def lds_word(g, n, mk, region, k, c, part, tid):
    """the LDS word of entry (k, c, part) of thread tid: region 0 = the top block (rows: transmit elements, n = Nr
    columns), 1 = T (which follows it; its first 2 n words of a thread hold the partial sums of a row of E later)"""
    base = 0 if region == 0 else mk * n * 2 * THREADS
    return base + ((k * n + c) * 2 + part) * THREADS + tid


def owner(g, r, slot):
    """-> (thread, k) owning row r of the matrix in point slot `slot` of the workgroup"""
    return slot * g + r % g, r // g


def grids(nr, nt):
    """(links, T, K) of the GPU tests for a shape: equalizer_util.grids of the factored shape (2 points, one pair
    below and above a workgroup's, 264 over several links)"""
    assert form(nr, nt) == EU.form(nt, nr)
    return EU.grids(nt, nr)


def kinds_of(nr, nt):
    """the kinds a shape is tested under"""
    return (MRT, ZF, RZF) if nr <= nt else (MRT, RZF)


def unit_roundoff(nr, nt):
    return (nr + nt) * 2.0 ** -24


def default_alpha(nr, noise=NOISE, power=POWER):
    return precode.default_regularization(nr, noise, power)


def out_bytes(nrx, ntx, nr, nt, T, K, flags):
    pts = nrx * ntx * 2 * T * K
    return (pts * nt * nr * 8 if flags & FLAG_P else 0) + pts * nr * 4 + pts * 4


# ---------------------------------------------------------------- the float64 reference

def reference_batch(mats, noise, kind, norm, power=POWER, alpha=None):
    """precode.precoder_reference on [B, Nr, Nt] -> P [B, Nt, Nr], sinr [B, Nr], status [B], cond [B]"""
    mats = np.asarray(mats)
    B = mats.shape[0]
    # (the layout wants two polarisations: the second is a copy)
    r = precode.precoder_reference(from_batch(np.concatenate([mats, mats]), (1, 1, 2, 1, B)), noise, KIND_NAME[kind],
                                   power, alpha, NORM_NAME[norm])
    return (to_batch(r["P"])[:B], to_batch_vec(r["sinr"])[:B], r["status"].reshape(-1)[:B], r["cond"].reshape(-1)[:B])


# ---------------------------------------------------------------- the emulation

def _reduce(v, g):
    """the butterfly over axis 1 (the g lanes) -> the value every lane ends with"""
    idx = np.arange(g)
    off = 1
    while off < g:
        v = v + v[:, idx ^ off]
        off *= 2
    return v[:, 0]


def emulate_p0(mats, kind, alpha):
    """stage in, start, factor and weights of the kernel on [B, Nr, Nt] complex64 -> (Ar, Ai [B, mk, g, Nr]: P0 in the
    lanes' layout, bad [B], sing [B])"""
    mats = np.asarray(mats, np.complex64)
    B, n, nt = mats.shape
    g = form(n, nt)
    mk, nk = -(-nt // g), -(-n // g)
    aug = kind == RZF
    lam = F(alpha) if aug else F(0)
    Ar, Ai = np.zeros((B, mk * g, n), F), np.zeros((B, mk * g, n), F)
    Ar[:, :nt], Ai[:, :nt] = np.swapaxes(mats.real, 1, 2), -np.swapaxes(mats.imag, 1, 2)
    Tr, Ti = np.zeros((B, nk * g, n), F), np.zeros((B, nk * g, n), F)
    Tr[:, np.arange(n), np.arange(n)] = 1
    Ar, Ai = Ar.reshape(B, mk, g, n), Ai.reshape(B, mk, g, n)
    Tr, Ti = Tr.reshape(B, nk, g, n), Ti.reshape(B, nk, g, n)

    def norm2(c):
        a = EU._lane_norm2(Ar, Ai, c)
        if aug:
            a = a + lam * EU._lane_norm2(Tr, Ti, c)
        return _reduce(a, g)

    with np.errstate(all="ignore"):
        nmax, nsum = np.zeros(B, F), np.zeros(B, F)
        for c in range(n):
            a = norm2(c)
            nmax = np.where(a > nmax, a, nmax)
            nsum = nsum + a
        bad = ~(nsum <= np.finfo(F).max)
        thr = (F(n + nt) * F(2.0 ** -23)) * np.sqrt(nmax)
        sing = np.zeros(B, bool)
        if kind == MRT:
            return Ar, Ai, bad, sing
        for j in range(n):
            rjj = np.sqrt(norm2(j))
            sing |= ~(rjj > thr)
            d = rjj[:, None, None]
            for X in (Ar, Ai, Tr, Ti):
                X[..., j] = X[..., j] / d
            for i in range(j + 1, n):
                rr, ri = EU._lane_dot(Ar, Ai, j, i)
                if aug:
                    tr, ti = EU._lane_dot(Tr, Ti, j, i)
                    rr, ri = rr + lam * tr, ri + lam * ti
                rr, ri = _reduce(rr, g)[:, None, None], _reduce(ri, g)[:, None, None]
                for Xr, Xi in ((Ar, Ai), (Tr, Ti)):
                    xr, xi = Xr[..., j], Xi[..., j]
                    Xr[..., i], Xi[..., i] = Xr[..., i] - (rr * xr - ri * xi), Xi[..., i] - (rr * xi + ri * xr)
        T_r, T_i = Tr.reshape(B, nk * g, n), Ti.reshape(B, nk * g, n)
        for i in range(n):
            for c in range(i, n):
                tr, tm = T_r[:, i, c][:, None, None], T_i[:, i, c][:, None, None]
                yr, yi = Ar[..., c], Ai[..., c]
                pr, pi = tr * yr + tm * yi, tr * yi - tm * yr
                if c == i:
                    Ar[..., i], Ai[..., i] = pr, pi
                else:
                    Ar[..., i], Ai[..., i] = Ar[..., i] + pr, Ai[..., i] + pi
    return Ar, Ai, bad, sing


def emulate_finish(mats, p0, noise, norm, power):
    """normalise, the E stage and the division on emulate_p0's result (not modified) -> P [B, Nt, Nr] complex64, sinr
    [B, Nr] float32, status [B] uint32"""
    mats = np.asarray(mats, np.complex64)
    B, n, nt = mats.shape
    Ar, Ai, bad, sing = p0[0].copy(), p0[1].copy(), p0[2], p0[3]
    mk, g = Ar.shape[1], Ar.shape[2]
    n0 = F(noise)
    pw = F(power) / F(n) if norm == STREAM else F(power)
    with np.errstate(all="ignore"):
        tot = np.zeros(B, F)
        zero = np.zeros(B, bool)
        for i in range(n):
            c = _reduce(EU._lane_norm2(Ar, Ai, i), g)
            tot = tot + c
            if norm == STREAM:
                zero |= ~(c > 0)
                s = np.sqrt(pw / c)[:, None, None]
                Ar[..., i], Ai[..., i] = Ar[..., i] * s, Ai[..., i] * s
        if norm == TOTAL:
            zero = ~(tot > 0)
            s = np.sqrt(pw / tot)[:, None, None, None]
            Ar, Ai = Ar * s, Ai * s
        status = np.where(bad, NONFINITE, np.where(sing | zero, SINGULAR,
                                                   np.where(~(tot <= np.finfo(F).max), NONFINITE, 0))).astype(np.uint32)
        flagged = status != 0
        Ar[flagged], Ai[flagged] = 0, 0
        Hr, Hi = np.zeros((B, n, mk * g), F), np.zeros((B, n, mk * g), F)
        Hr[:, :, :nt], Hi[:, :, :nt] = mats.real, mats.imag
        Hr, Hi = Hr.reshape(B, n, mk, g), Hi.reshape(B, n, mk, g)
        sinr = np.zeros((B, n), F)
        for i in range(n):
            ar, ai = np.zeros((B, g, n), F), np.zeros((B, g, n), F)
            for k in range(mk):
                hr, hi = Hr[:, i, k, :, None], Hi[:, i, k, :, None]
                pr, pi = Ar[:, k], Ai[:, k]
                ar = ar + (hr * pr - hi * pi)
                ai = ai + (hr * pi + hi * pr)
            er, ei = _reduce(ar, g), _reduce(ai, g)            # [B, Nr]: row i of E
            m = er * er + ei * ei
            itf = np.zeros(B, F)
            for j in range(n):
                if j != i:
                    itf = itf + m[:, j]
            sinr[:, i] = m[:, i] / (itf + n0)
        sinr[flagged] = 0
    P = (Ar.reshape(B, mk * g, n)[:, :nt] + 1j * Ai.reshape(B, mk * g, n)[:, :nt]).astype(np.complex64)
    return P, sinr, status


def emulate_batch(mats, noise, kind, norm, power=POWER, alpha=None):
    """The kernel on [B, Nr, Nt] complex64 matrices in numpy float32 -> P [B, Nt, Nr] complex64, sinr [B, Nr] float32,
    status [B] uint32 (alpha None: the default of RZF, Nr N0 / Ptot)"""
    mats = np.asarray(mats, np.complex64)
    if alpha is None:
        alpha = default_alpha(mats.shape[1], noise, power) if kind == RZF else 0.0
    return emulate_finish(mats, emulate_p0(mats, kind, alpha), noise, norm, power)


def emulate(H, noise, kind, norm, power=POWER, alpha=None):
    """emulate_batch on a device-layout tensor -> dict in the device layout"""
    H = np.asarray(H)
    lead = (H.shape[0], H.shape[1]) + H.shape[4:]
    P, sinr, status = emulate_batch(to_batch(H), noise, kind, norm, power, alpha)
    return {"P": from_batch(P, lead), "sinr": from_batch(sinr, lead), "status": status.reshape(lead)}


# ---------------------------------------------------------------- cases under the derived bounds

@functools.lru_cache(maxsize=None)
def master_cases(nr, nt):
    """MASTER matrices [MASTER, Nr, Nt] complex64 of one shape and the family of each: the transposes of
    equalizer_util.master_cases(Nt, Nr), so the families by index mod 4 are 0 standard normal, 1 prescribed singular
    values 1, 2^-4, 2^-8, 2 row 1 = (1 + 2^-12) row 0: rank deficient to rounding -- regular under MRT and RZF, SINGULAR
    under ZF (bounded(), below), 3 row 1 = row 0 plus 2^-12 times a standard normal row, which every kind bounds (2 and
    3: Nr >= 2; else a standard normal matrix).  The tensors of the GPU tests are prefixes of this list."""
    mats, kinds = EU.master_cases(nt, nr)
    mats = np.ascontiguousarray(np.swapaxes(mats, 1, 2))
    mats.setflags(write=False)
    return mats, kinds


def bounded(kinds, kind):
    """which matrices of master_cases a kind of precoder bounds: all but the rank-deficient family under ZF, which
    must come out SINGULAR with exact zeros instead"""
    return kinds != 2 if kind == ZF else np.ones(len(kinds), bool)


# the heavily regularised set: the first 24 standard normal matrices of master_cases under RZF with
# alpha = 2^8 E|H|_F^2 = 2^8 * 2 Nr Nt.  P0 is H^H / alpha to 2^-8, and E = I - alpha (H H^H + alpha I)^-1, the identity
# of the factorisation, would be the difference of two numbers that agree to 2^-8 / Nr.
HEAVY_SHAPES = ((4, 4), (7, 9), (16, 16), (16, 64))


def heavy_cases(nr, nt):
    mats, kinds = master_cases(nr, nt)
    return np.array(mats[kinds == 0][:24]), 2.0 ** 8 * 2 * nr * nt


def configurations():
    """every (name, mats, kind, norm, noise, power, alpha) the GPU tests hold under the bounds"""
    for nr, nt in SHAPES:
        mats, kinds = master_cases(nr, nt)
        for kind in kinds_of(nr, nt):
            alpha = default_alpha(nr) if kind == RZF else 0.0
            for norm in NORMS:
                yield ("%dx%d %s %s" % (nr, nt, KIND_NAME[kind], NORM_NAME[norm]), mats[bounded(kinds, kind)], kind,
                       norm, NOISE, POWER, alpha)
    for nr, nt in HEAVY_SHAPES:
        mats, alpha = heavy_cases(nr, nt)
        for norm in NORMS:
            yield "%dx%d heavy %s" % (nr, nt, NORM_NAME[norm]), mats, RZF, norm, NOISE, POWER, alpha


def measures(mats, noise, kind, norm, power, alpha, P, sinr):
    """The two measures of [B, ..] results against the float64 reference on the widened float32 input, per matrix:
    | P^ - P |_F / (| P |_F u kappa);  max_i | rho^_i - rho_i | / ((1 + rho_i) u kappa)."""
    mats = np.asarray(mats, np.complex64)
    B, nr, nt = mats.shape
    a = float(F(alpha)) if kind == RZF else None
    Pr, sr, status, cond = reference_batch(mats, float(F(noise)), kind, norm, float(F(power)), a)
    assert not status.any(), "a bounded case is flagged in float64"
    u = unit_roundoff(nr, nt)
    P, sinr = np.asarray(P).astype(np.complex128), np.asarray(sinr, np.float64)
    fro = lambda X: np.sqrt((np.abs(X) ** 2).sum((1, 2)))
    m_p = fro(P - Pr) / (fro(Pr) * u * cond)
    m_s = (np.abs(sinr - sr) / (1.0 + sr)).max(1) / (u * cond)
    return m_p, m_s


def check(mats, noise, kind, norm, power, alpha, P, sinr, status, tol=None):
    """Everything the GPU tests ask of the results [B, ..] of bounded cases [B, Nr, Nt]: shapes, status 0, finite
    values, the two measures under their constants.  Raises AssertionError; returns the worst measures."""
    mats = np.asarray(mats)
    B, nr, nt = mats.shape
    tol = (TOL_P, TOL_SINR) if tol is None else tol
    assert P.shape == (B, nt, nr) and sinr.shape == (B, nr) and status.shape == (B,), (P.shape, sinr.shape)
    assert not np.asarray(status).any(), "a regular point is flagged"
    assert np.isfinite(P.view(np.float32)).all() and np.isfinite(sinr).all(), "results not finite"
    worst = []
    for name, x, t in zip(("precoder", "sinr"), measures(mats, noise, kind, norm, power, alpha, P, sinr), tol):
        worst.append(float(x.max()))
        assert worst[-1] <= t, "%s measure %.3g > %.3g (matrix %d)" % (name, worst[-1], t, int(x.argmax()))
    return worst


# ---------------------------------------------------------------- exact plantings (every intermediate exact in float32)

def _unit(rng, shape):
    """entries from {1, -1, j, -j}"""
    return np.array([1, -1, 1j, -1j])[rng.randint(0, 4, shape)]


PLANT_SHAPES = ((1, 1), (4, 4), (3, 5), (5, 6), (8, 9), (16, 16), (16, 17), (16, 64))
MRT_BASE = np.array([[1 + 1j, 2, -1j, 0, 1], [0, 1 - 2j, 1, 1j, -1], [2j, 0, 1 + 1j, -1, 0]])


def exact_cases():
    """[(name, kind, norm, noise, power, alpha, mats [B, Nr, Nt] complex64, P [B, Nt, Nr] complex64, sinr [B, Nr]
    float32, status [B])]: matrices for which every intermediate of the kernel is exact, so every output is.
      zf permutation   one entry s 2^e per row, s from {+-1, +-j}, distinct columns, N0 a power of two.
                       STREAM with Ptot / Nr = 4^a: P[t_i, i] = conj(s) 2^a, sinr_i = 4^(a + e_i) / N0.
                       TOTAL with one multiset of exponents per shape, permuted per matrix, and Ptot = 4^a sum 4^-e
                       (the sum itself is a power of four where Nr = 1 mod 3, the only sizes at which one can be):
                       P[t_i, i] = conj(s) 2^(a - e_i), sinr_i = 4^a / N0
      zf coupled       rows in pairs on disjoint columns, h_0 = conj(al) e_c0, h_1 = conj(be) e_c0 + conj(ga) e_c1 with
                       |be| = |ga|: R is not diagonal.  TOTAL with Ptot = 4^a |H^+|_F^2: P = 2^a H^+, sinr = 4^a / N0
      rzf triple       three entries of magnitude 2^e per row on disjoint columns, alpha = 4^e: the column norms of the
                       factored matrix are 2^(e+1), P0 = H^H / 4^(e+1).  Ptot = 3 Nr 4^a makes both norms scale by
                       2^(a+e+2): P = 2^(a-e) H^H, E_ii = 3 2^(a+e), sinr = 9 4^(a+e) / N0
      mrt integers     row and column permutations of one Gaussian-integer matrix with unit phases on its rows, so
                       |H|_F^2 is shared; TOTAL with Ptot = 4^a |H|_F^2: P = 2^a H^H, E = 2^a H H^H in integers, and
                       sinr is the single float32 division of exact operands
      zero             H = 0: SINGULAR under every kind and norm, exact zeros"""
    rng = np.random.RandomState(87)
    out = []
    B = 12
    for nr, nt in PLANT_SHAPES:
        # zf permutation, STREAM
        a, n0 = 1, 2.0 ** -3
        H = np.zeros((B, nr, nt), np.complex128)
        P = np.zeros((B, nt, nr), np.complex128)
        S = np.zeros((B, nr))
        for b in range(B):
            cols = rng.permutation(nt)[:nr]
            e = rng.permutation(np.arange(-8, 8))[:nr]
            s = _unit(rng, nr)
            s[0] = (1j, -1j, 1, -1)[b % 4]
            H[b, np.arange(nr), cols] = s * 2.0 ** e
            P[b, cols, np.arange(nr)] = np.conj(s) * 2.0 ** a
            S[b] = 4.0 ** (a + e) / n0
        out.append(("zf permutation stream %dx%d" % (nr, nt), ZF, STREAM, n0, nr * 4.0 ** a, 0.0, H, P, S))
        # zf permutation, TOTAL
        a, n0 = -1, 2.0 ** -5
        es = [0]
        while len(es) + 3 <= nr:                                 # split one term into four of a quarter: the sum stays 1
            es = es[1:] + [es[0] + 1] * 4
        es = np.array(es + [2] * (nr - len(es)))
        tot = (4.0 ** -es).sum()
        assert (nr % 3 != 1) or tot == 1.0
        H = np.zeros((B, nr, nt), np.complex128)
        P = np.zeros((B, nt, nr), np.complex128)
        for b in range(B):
            cols = rng.permutation(nt)[:nr]
            e = rng.permutation(es)
            s = _unit(rng, nr)
            H[b, np.arange(nr), cols] = s * 2.0 ** e
            P[b, cols, np.arange(nr)] = np.conj(s) * 2.0 ** (a - e)
        out.append(("zf permutation total %dx%d" % (nr, nt), ZF, TOTAL, n0, 4.0 ** a * tot, 0.0, H, P,
                    np.full((B, nr), 4.0 ** a / n0)))
        # zf coupled, TOTAL
        if nr >= 2:
            a, n0 = 2, 2.0
            ex = rng.randint(-2, 3, (nr // 2, 2))                # (ea, eg) of every pair: shared by the matrices
            e1 = rng.randint(-2, 3)
            tot = (2 * 4.0 ** -ex[:, 0] + 4.0 ** -ex[:, 1]).sum() + (4.0 ** -e1 if nr % 2 else 0.0)
            H = np.zeros((B, nr, nt), np.complex128)
            P = np.zeros((B, nt, nr), np.complex128)
            for b in range(B):
                cols = rng.permutation(nt)[:nr]
                for q, p in enumerate(range(0, nr - 1, 2)):
                    c0, c1 = cols[p], cols[p + 1]
                    al, be, ga = _unit(rng, 3) * 2.0 ** np.array([ex[q, 0], ex[q, 1], ex[q, 1]])
                    H[b, p, c0], H[b, p + 1, c0], H[b, p + 1, c1] = np.conj(al), np.conj(be), np.conj(ga)
                    P[b, c0, p], P[b, c1, p], P[b, c1, p + 1] = np.conj(1 / al), np.conj(-be / (al * ga)), np.conj(1 / ga)
                if nr % 2:
                    s = _unit(rng, 1)[0]
                    H[b, nr - 1, cols[-1]] = s * 2.0 ** e1
                    P[b, cols[-1], nr - 1] = np.conj(s) * 2.0 ** -e1
            out.append(("zf coupled %dx%d" % (nr, nt), ZF, TOTAL, n0, 4.0 ** a * tot, 0.0, H, P * 2.0 ** a,
                        np.full((B, nr), 4.0 ** a / n0)))
        # rzf triple, both norms
        if nt >= 3 * nr:
            for e, a in ((-3, 2), (2, -1)):
                n0 = 2.0 ** -2
                H = np.zeros((B, nr, nt), np.complex128)
                for b in range(B):
                    cols = rng.permutation(nt)[:3 * nr].reshape(3, nr)
                    for t in range(3):
                        H[b, np.arange(nr), cols[t]] = _unit(rng, nr) * 2.0 ** e
                P = np.conj(np.swapaxes(H, 1, 2)) * 2.0 ** (a - e)
                for norm in NORMS:
                    out.append(("rzf triple %s %dx%d e=%d" % (NORM_NAME[norm], nr, nt, e), RZF, norm, n0,
                                3 * nr * 4.0 ** a, 4.0 ** e, H, P, np.full((B, nr), 9 * 4.0 ** (a + e) / n0)))
        # zero: SINGULAR under every kind and norm
        for kind in kinds_of(nr, nt):
            for norm in NORMS:
                out.append(("zero %s %s %dx%d" % (KIND_NAME[kind], NORM_NAME[norm], nr, nt), kind, norm, 0.25, 1.0,
                            0.5, np.zeros((4, nr, nt), np.complex128), np.zeros((4, nt, nr), np.complex128),
                            np.zeros((4, nr))))
    # rzf triple on the wide shapes that have room for it
    for nr, nt in ((1, 3), (2, 7), (5, 16), (16, 48), (16, 64)):
        e, a, n0 = 1, 0, 2.0 ** -4
        H = np.zeros((B, nr, nt), np.complex128)
        for b in range(B):
            cols = rng.permutation(nt)[:3 * nr].reshape(3, nr)
            for t in range(3):
                H[b, np.arange(nr), cols[t]] = _unit(rng, nr) * 2.0 ** e
        P = np.conj(np.swapaxes(H, 1, 2)) * 2.0 ** (a - e)
        for norm in NORMS:
            out.append(("rzf triple %s %dx%d" % (NORM_NAME[norm], nr, nt), RZF, norm, n0, 3 * nr * 4.0 ** a, 4.0 ** e,
                        H, P, np.full((B, nr), 9 * 4.0 ** (a + e) / n0)))
    # mrt integers: 3 x 5 base, also embedded in larger shapes
    for nr, nt in ((3, 5), (3, 8), (5, 9), (16, 64)):
        a, n0 = -1, 2.0 ** -1
        tot = (np.abs(MRT_BASE) ** 2).sum()
        H = np.zeros((B, nr, nt), np.complex128)
        for b in range(B):
            rows, cols = rng.permutation(nr)[:3], rng.permutation(nt)[:5]
            H[b][np.ix_(rows, cols)] = MRT_BASE[rng.permutation(3)] * _unit(rng, 3)[:, None]
        P = np.conj(np.swapaxes(H, 1, 2)) * 2.0 ** a
        p = np.abs(H @ P) ** 2
        sig = np.diagonal(p, axis1=1, axis2=2)
        itf = p.sum(2) - sig                                     # (integers times 4^a: exact)
        S = sig.astype(F) / (itf + n0).astype(F)
        out.append(("mrt integers %dx%d" % (nr, nt), MRT, TOTAL, n0, 4.0 ** a * tot, 0.0, H, P, S))
    res = []
    for name, kind, norm, n0, power, alpha, H, P, S in out:
        st = np.full(len(H), SINGULAR if name.startswith("zero") else 0, np.uint32)
        assert float(F(power)) == power and float(F(n0)) == n0 and float(F(alpha)) == alpha
        res.append((name, kind, norm, n0, power, alpha, H.astype(np.complex64), P.astype(np.complex64), S.astype(F), st))
    return res


# (kind, Nr, Nt, K) of the one-row plantings: 120 and 552 points for at most 15 and 272 entries
ONE_ROW = ((MRT, 3, 5, 5), (RZF, 3, 5, 5), (MRT, 16, 17, 23), (RZF, 16, 17, 23))


def one_row_case(kind, nr, nt, links=(2, 3), T=2, K=5):
    """One nonzero row per point, one point per output index, in one call: a device-layout tensor whose every point p
    has ONE nonzero row i = p mod Nr, TOTAL normalisation.
      MRT: one entry of magnitude 2 at column t = (p div Nr) mod Nt, Ptot = 4: P[t, i] = conj(s) 2 is the only nonzero
           entry of P, sinr_i = 16 / N0, every other output an exact zero.
      RZF: three units at columns t, t + 1, t + 2 (mod Nt), alpha = 1, Ptot = 12: the norm of column i of the factored
           matrix is 2, the others' is 1; P0 = H^H / 4, |P0|_F^2 = 3 / 16, the scale 8: P = 2 H^H, E_ii = 6,
           sinr_i = 36 / N0.  (A single entry cannot be exact under RZF: |h|^2 + 4^e is no power of four.)
    With more points than entries every (t, i), and so every output index, is hit.  Nt >= 3.
    -> (H, noise, power, alpha, P, sinr) in the device layout"""
    rng = np.random.RandomState(88)
    nrx, ntx = links
    B = nrx * ntx * 2 * T * K
    H = np.zeros((B, nr, nt), np.complex64)
    S = np.zeros((B, nr), np.float32)
    p = np.arange(B)
    i, t = p % nr, (p // nr) % nt
    n0 = 0.5
    if kind == MRT:
        H[p, i, t] = 2 * _unit(rng, B)
        power, alpha = 4.0, 0.0
        S[p, i] = 16 / n0
    else:
        for d in range(3):
            H[p, i, (t + d) % nt] = _unit(rng, B)
        power, alpha = 12.0, 1.0
        S[p, i] = 36 / n0
    P = (2 * np.conj(np.swapaxes(H, 1, 2))).astype(np.complex64) if kind == RZF else \
        np.conj(np.swapaxes(H, 1, 2)).astype(np.complex64)
    lead = (nrx, ntx, 2, T, K)
    return from_batch(H, lead), n0, power, alpha, from_batch(P, lead), from_batch(S, lead)


# ---------------------------------------------------------------- wrong readings of the definition

READINGS = ("p_not_conjugated", "p_stored_nr_nt", "total_and_stream_swapped", "stream_power_not_divided",
            "own_term_in_interference", "noise_scaled_with_precoder", "alpha_replaced_by_noise",
            "sinr_of_unnormalised_p0", "mrt_normalised_by_norm_not_square", "equalizer_w_returned",
            "e_from_identity_in_float")


def reading(mats, noise, kind, norm, power, alpha, wrong=None):
    """The definition in float64 on [B, Nr, Nt] -> P [B, Nt, Nr] (flat in that order), sinr [B, Nr]; `wrong` names one
    misreading (READINGS; None where it does not apply to the kind and norm).  Only for well-conditioned matrices: it
    goes through the Gram matrix."""
    A = np.asarray(mats).astype(np.complex128)
    B, nr, nt = A.shape
    applies = {"total_and_stream_swapped": True, "stream_power_not_divided": norm == STREAM and nr > 1,
               "alpha_replaced_by_noise": kind == RZF and nr > 1, "mrt_normalised_by_norm_not_square": kind == MRT and norm == TOTAL,
               "equalizer_w_returned": kind == RZF and nt <= 16, "e_from_identity_in_float": kind == RZF,
               "own_term_in_interference": True, "noise_scaled_with_precoder": True, "sinr_of_unnormalised_p0": True,
               "p_not_conjugated": True, "p_stored_nr_nt": nr > 1 or nt > 1, None: True}
    if not applies[wrong]:
        return None
    if wrong == "alpha_replaced_by_noise":
        alpha = noise
    if wrong == "total_and_stream_swapped":
        norm = STREAM if norm == TOTAL else TOTAL
    AH = np.conj(np.swapaxes(A, 1, 2))
    G = None
    if kind == MRT:
        P0 = AH
    else:
        G = np.linalg.inv(A @ AH + (alpha if kind == RZF else 0.0) * np.eye(nr))
        P0 = AH @ G
    c = (np.abs(P0) ** 2).sum(1)                                          # [B, Nr]
    if norm == STREAM:
        pw = power if wrong == "stream_power_not_divided" else power / nr
        scale = np.sqrt(pw / c)[:, None, :]
    else:
        tot = c.sum(1)
        if wrong == "mrt_normalised_by_norm_not_square":
            tot = np.sqrt(tot)
        scale = np.sqrt(power / tot)[:, None, None]
    P = P0 * scale
    if wrong == "equalizer_w_returned":
        H7 = from_batch(np.concatenate([A, A]), (1, 1, 2, 1, B))
        P = to_batch(equalize.equalizer_reference(H7, noise, "lmmse")["W"])[:B]
    E = A @ (P0 if wrong == "sinr_of_unnormalised_p0" else P)
    if wrong == "e_from_identity_in_float":
        # E = (I - alpha (H H^H + alpha I)^-1) scale, the subtraction rounded to float32 as a kernel would
        E = (np.eye(nr, dtype=np.complex64) - (F(alpha) * G).astype(np.complex64)).astype(np.complex128) * scale
    p = np.abs(E) ** 2
    sig = np.diagonal(p, axis1=1, axis2=2)
    itf = (p * (1.0 - np.eye(nr))).sum(2)
    if wrong == "own_term_in_interference":
        itf = itf + sig
    n0 = noise
    if wrong == "noise_scaled_with_precoder":
        n0 = noise * (scale.reshape(B, -1) ** 2).mean(1)[:, None]
    sinr = sig / (itf + n0)
    if wrong == "p_not_conjugated":
        P = np.conj(P)
    if wrong == "p_stored_nr_nt":
        P = np.ascontiguousarray(np.swapaxes(P, 1, 2)).reshape(B, nt, nr)
    return P, sinr
