"""The K-best tree-search detection's design, shared by tests/test_kbest_design.py (CPU) and tests/test_gpu_kbest*.py:
the mirror of csrc/hrt_kbest.h's form rule, the numpy float32 emulation of include/hermespy_rt.h's hrt_kbest_spec in
the kernel's sum order (per lane over its rows ascending, then a butterfly over the group), the exact plantings, the
wrong readings of the definition that the plantings separate, the standard-normal cases and the tolerance constants.

Tolerances.  Per point u = (Nr + Nt) 2^-24 and sigma = (|y|_2 + |H|_F max|S| sqrt(Nt))^2 (detect_util.scale gives
u sigma).  The metric is compared as |d^ - d| / (u sigma) and every LLR as |llr^ - llr| N0 / (u sigma) against
hermespy_rt_amd.detect.kbest_reference on the widened float32 input, at the points that are not fragile.  The bounds
are 4 x the worst value of the float32 emulation over NORMAL_CASES at those points (test_kbest_design recomputes them):

    worst  metric  0.0349 (n-2x2-b4-k4)   llr  0.0642 (n-2x2-b4-k4)     bound  METRIC_BOUND = 0.140   LLR_BOUND = 0.257

A point is fragile where a float32 search may decide otherwise than the float64 one: a pruning gap (K-th against
(K + 1)-th candidate of a level, relative to sigma) at or below 2 METRIC_BOUND u -- two partial distances, each within
the metric bound --, or, sorted, two residual column norms at a pick closer than 8 METRIC_BOUND u of H's largest
squared column norm (a residual norm is a distance of Nr terms after up to Nt projections; four times the allowance of
a pair).  At most FRAGILE_CAP of a case's points may be fragile.  The index is compared where the reference's two best
leaves differ by more than 2 METRIC_BOUND u sigma.
"""
import numpy as np

from .detect_util import _points, _tensors, f32, FLT_MAX, gaussian_integers, normal, rounded, same, scale  # noqa: F401
from hermespy_rt_amd import detect as DT

LLR, SORTED = 1, 2
NONFINITE, DEFICIENT = 1, 2
NO_INDEX = 0xFFFFFFFF
THREADS, WORDS = 256, 56
MAX_NR, MAX_NT, MAX_B, MAX_BITS, MAX_K = 64, 16, 8, 32, 64
KS = (1, 2, 4, 8, 16, 32, 64)

METRIC_WORST, LLR_WORST = 0.0350, 0.0643
METRIC_BOUND, LLR_BOUND = 4 * METRIC_WORST, 4 * LLR_WORST
FRAGILE_CAP = 0.10


# ---------------------------------------------------------------- the form (csrc/hrt_kbest.h)

def point_words(nt):
    """hrt_kbest_point_words"""
    return 2 * nt * (nt + 1)


def form(nr, nt, k):
    """hrt_kbest_form: lanes per point; 0 outside the limits"""
    if not (1 <= nr <= MAX_NR and 1 <= nt <= MAX_NT and k in KS):
        return 0
    g = k
    while g <= 64:
        if 2 * (nt + 1) * ((nr + g - 1) // g) + (point_words(nt) + g - 1) // g <= WORDS:
            return g
        g *= 2
    return 0


def out_bytes(nrx, ntx, nt, B, T, K, flags):
    """hrt_kbest_out_bytes, restated"""
    pts = nrx * ntx * 2 * T * K
    return pts * 12 + (pts * nt * B * 4 if flags & LLR else 0)


# ---------------------------------------------------------------- the float32 emulation

WRONG_READINGS = ("levels-from-0", "ties-higher-key", "key-from-positions", "rho-left-out", "sorted-descending",
                  "null-divided", "llr-all-leaves", "clip-sign", "no-clamp")


def _butterfly(v, g):
    """v [P, g]: the sum over the group as the kernel forms it -> [P]"""
    lane = np.arange(g)
    off = 1
    while off < g:
        v = v + v[:, lane ^ off]
        off *= 2
    return v[:, 0]


def emulate(H, Y, S, noise, k, clip, sorted=True, llr=True, wrong=None):
    """The kernel in numpy float32, operation by operation: H complex64 [nrx, ntx, Nr, Nt, 2, T, K], Y complex64
    [nrx, ntx, Nr, 2, T, K], S complex64 [2^B] -> dict in the device layout: index uint32, metric float32, status uint32
    [nrx, ntx, 2, T, K], llr float32 [nrx, ntx, Nt, B, 2, T, K] (None without llr).  `wrong`: one of WRONG_READINGS,
    a misreading of the definition."""
    H, Y, S = np.asarray(H, np.complex64), np.asarray(Y, np.complex64), np.asarray(S, np.complex64)
    nr, nt = H.shape[2], H.shape[3]
    n = nt + 1
    M = S.shape[0]
    B = M.bit_length() - 1
    K = int(k)
    g = form(nr, nt, K)
    assert g, (nr, nt, K)
    mk = (nr + g - 1) // g
    lead_shape = H.shape[:2] + H.shape[4:]
    A = np.concatenate([_points(H), np.moveaxis(Y, 2, -1)[..., None]], -1).reshape(-1, nr, n)
    P = A.shape[0]
    ar = np.arange(P)
    pad = np.zeros((P, g * mk, n), np.complex64)
    pad[:, :nr] = A
    # row r = l + g k of the matrix is row k of lane l: [P, g, mk, n]
    pad = pad.reshape(P, mk, g, n).swapaxes(1, 2)
    Ar, Ai = np.ascontiguousarray(pad.real), np.ascontiguousarray(pad.imag)
    sr, si = np.ascontiguousarray(S.real), np.ascontiguousarray(S.imag)
    n0, cl = f32(noise), f32(clip)

    def norm2(c):
        """c [P] -> the squared norm of column c of every point"""
        a = np.zeros((P, g), f32)
        for kk in range(mk):
            xr, xi = Ar[ar, :, kk, c], Ai[ar, :, kk, c]
            a = a + (xr * xr + xi * xi)
        return _butterfly(a, g)

    with np.errstate(all="ignore"):
        nmax, nsum = np.zeros(P, f32), np.zeros(P, f32)
        for c in range(n):
            a = norm2(np.full(P, c))
            if c < nt:
                nmax = np.where(a > nmax, a, nmax)
            nsum = nsum + a
        bad = ~(nsum <= FLT_MAX)
        thr = (f32(nr + nt) * f32(2.0 ** -23)) * np.sqrt(nmax)
        Rr, Ri = np.zeros((P, nt, nt), f32), np.zeros((P, nt, nt), f32)     # [position, stream]
        zr, zi = np.zeros((P, nt), f32), np.zeros((P, nt), f32)
        order = np.zeros((P, nt), np.int64)
        chosen = np.zeros((P, nt), bool)
        deficient = np.zeros(P, bool)
        for t in range(nt):
            if sorted:
                c, a, first = np.zeros(P, np.int64), np.zeros(P, f32), np.ones(P, bool)
                for u in range(nt):
                    au = norm2(np.full(P, u))
                    better = au > a if wrong == "sorted-descending" else au < a
                    take = ~chosen[:, u] & (first | better)
                    a, c = np.where(take, au, a), np.where(take, u, c)
                    first &= chosen[:, u]
            else:
                c = np.full(P, t)
                a = norm2(c)
            chosen[ar, c] = True
            order[:, t] = c
            r = np.sqrt(a)
            null = ~(r > thr)
            if wrong == "null-divided":
                null = np.zeros(P, bool)
            deficient |= null
            live = ~null
            d = np.where(null, f32(1), r)[:, None, None]
            Ar[ar, :, :, c] = np.where(live[:, None, None], Ar[ar, :, :, c] / d, Ar[ar, :, :, c])
            Ai[ar, :, :, c] = np.where(live[:, None, None], Ai[ar, :, :, c] / d, Ai[ar, :, :, c])
            for u in range(n):
                todo = live & (~chosen[:, u] if u < nt else True)
                re, im = np.zeros((P, g), f32), np.zeros((P, g), f32)
                for kk in range(mk):
                    xr, xi, yr, yi = Ar[ar, :, kk, c], Ai[ar, :, kk, c], Ar[:, :, kk, u], Ai[:, :, kk, u]
                    re = re + (xr * yr + xi * yi)
                    im = im + (xr * yi - xi * yr)
                rr, ri = _butterfly(re, g), _butterfly(im, g)
                rr, ri = np.where(todo, rr, f32(0)), np.where(todo, ri, f32(0))
                xr, xi = Ar[ar, :, :, c], Ai[ar, :, :, c]
                m3 = todo[:, None, None]
                nyr = Ar[:, :, :, u] - (rr[:, None, None] * xr - ri[:, None, None] * xi)
                nyi = Ai[:, :, :, u] - (rr[:, None, None] * xi + ri[:, None, None] * xr)
                Ar[:, :, :, u] = np.where(m3, nyr, Ar[:, :, :, u])
                Ai[:, :, :, u] = np.where(m3, nyi, Ai[:, :, :, u])
                if u < nt:
                    unpicked = ~chosen[:, u]
                    Rr[:, t, u] = np.where(unpicked, rr, Rr[:, t, u])
                    Ri[:, t, u] = np.where(unpicked, ri, Ri[:, t, u])
                else:
                    zr[:, t], zi[:, t] = rr, ri
            Rr[ar, t, c] = np.where(null, f32(0), r)
            Ri[ar, t, c] = f32(0)
        rho = norm2(np.full(P, nt))
        bad |= ~(rho <= FLT_MAX)

        # ---- the tree
        ped = (np.zeros(P, f32) if wrong == "rho-left-out" else rho)[:, None].copy()
        key = np.zeros((P, 1), np.int64)
        x = np.arange(M)
        levels = range(nt) if wrong == "levels-from-0" else range(nt - 1, -1, -1)
        visited = None
        for i in levels:
            c = order[:, i]
            place = np.full(P, i) if wrong == "key-from-positions" else c       # where the digit of this level goes
            br = bi = None
            others = range(i) if wrong == "levels-from-0" else range(i + 1, nt)
            for t in others:
                u = order[:, t]
                where = np.full(P, t) if wrong == "key-from-positions" else u
                xr_, xi_ = Rr[ar, i, u][:, None], Ri[ar, i, u][:, None]
                sx = (key >> (where * B)[:, None]) & (M - 1)
                pr = xr_ * sr[sx] - xi_ * si[sx]
                pi = xr_ * si[sx] + xi_ * sr[sx]
                br = pr if br is None else br + pr
                bi = pi if bi is None else bi + pi
            if br is None:
                br = np.repeat(zr[:, i, None], ped.shape[1], 1)
                bi = np.repeat(zi[:, i, None], ped.shape[1], 1)
            else:
                br, bi = zr[:, i, None] - br, zi[:, i, None] - bi
            rii = Rr[ar, i, c][:, None, None]
            er = br[:, :, None] - rii * sr[None, None, :]
            ei = bi[:, :, None] - rii * si[None, None, :]
            cp = (ped[:, :, None] + (er * er + ei * ei)).reshape(P, -1)
            ck = (key[:, :, None] | (x[None, None, :] << (place * B)[:, None, None])).reshape(P, -1)
            bad |= ~(cp <= FLT_MAX).all(-1)
            o1 = np.argsort(-ck if wrong == "ties-higher-key" else ck, -1, kind="stable")
            cp, ck = np.take_along_axis(cp, o1, -1), np.take_along_axis(ck, o1, -1)
            o2 = np.argsort(cp, -1, kind="stable")
            cp, ck = np.take_along_axis(cp, o2, -1), np.take_along_axis(ck, o2, -1)
            visited = (cp, ck)
            ped, key = cp[:, :K], ck[:, :K]
        index, best = key[:, 0], ped[:, 0]
        L = None
        if llr:
            lp, lk = visited if wrong == "llr-all-leaves" else (ped, key)
            L = np.empty((P, nt, B), f32)
            for j in range(nt):
                for b in range(B):
                    one = ((lk >> (j * B + (B - 1 - b))) & 1).astype(bool)
                    m0 = np.where(one, f32(np.inf), lp).min(-1)
                    m1 = np.where(one, lp, f32(np.inf)).min(-1)
                    has0, has1 = m0 <= FLT_MAX, m1 <= FLT_MAX
                    both = has0 & has1
                    v = (np.where(both, m0, f32(0)) - np.where(both, m1, f32(0))) / n0
                    bad |= both & ~(np.abs(v) <= FLT_MAX)
                    if wrong != "no-clamp":
                        v = np.where(v > cl, cl, v)
                        v = np.where(v < -cl, -cl, v)
                    lone = np.where(has0, -cl, cl)          # no leaf with bit 0: +clip
                    if wrong == "clip-sign":
                        lone = -lone
                    L[:, j, b] = np.where(both, v, lone)
            L = np.where(bad[:, None, None], f32(0), L).astype(f32)
            L = np.moveaxis(L.reshape(lead_shape + (nt, B)), (-2, -1), (2, 3))
    status = np.where(bad, NONFINITE, np.where(deficient, DEFICIENT, 0)).astype(np.uint32)
    return {"index": np.where(bad, NO_INDEX, index).astype(np.uint32).reshape(lead_shape),
            "metric": np.where(bad, f32(0), best).astype(f32).reshape(lead_shape),
            "status": status.reshape(lead_shape), "llr": L}


def reference(H, Y, S, noise, k, clip, sorted=True, llr=True):
    """kbest_reference on the widened float32 input"""
    return DT.kbest_reference(np.asarray(H, np.complex64), np.asarray(Y, np.complex64), np.asarray(S, np.complex64),
                              float(f32(noise)), k, float(f32(clip)), sorted, llr)


# ---------------------------------------------------------------- exact plantings

def hadamard(n):
    h = np.ones((1, 1))
    while h.shape[0] < n:
        h = np.block([[h, h], [h, -h]])
    return h


# name, (nrx, ntx), Nr, Nt, B, T, K, k, sorted, Q0 ("perm": scaled permutation columns, "had": Hadamard / sqrt(Nr)),
# N0, clip, the largest diagonal exponent of R0, the amplitude of the Gaussian-integer noise, special
#   special  None; "null": one column of R0 is zeroed (a null column: its level ties every child); "tie-norm": two
#            equal diagonals with no entry above the second (two equal column norms under sorted)
# H = Q0 R0 Pi: R0 upper triangular Gaussian integers with diagonal 2^e, e non-decreasing when sorted (the sorted
# order is then the planted one, every pick has a power-of-two norm), any e when not.  Unnormalised QAM (odd
# integers), y = H s + Gaussian-integer noise: every norm, projection and PED is exact in float32.  Nr < Nt plants
# Nt - Nr dependent columns, which are null (unsorted: sorted would pick a dependent column, whose norm is no power of
# two, first).
PLANTINGS = (
    ("k1-1x1-nr1", (1, 1), 1, 1, 1, 1, 3, 1, True, "perm", 1.0, 8.0, 1, 1, None),
    ("k1-sic-4x4-b4", (1, 1), 4, 4, 4, 1, 5, 1, True, "had", 0.5, 64.0, 2, 2, None),
    ("k2-2x2-b2-nr64", (2, 1), 64, 2, 2, 3, 1, 2, True, "perm", 2.0, 4.0, 1, 2, None),
    ("k2-2x2-b4-unsorted", (1, 1), 4, 2, 4, 1, 3, 2, False, "had", 1.0, 16.0, 2, 3, None),
    ("k8-4x4-b2-nr4", (1, 2), 4, 4, 2, 1, 5, 8, True, "had", 0.25, 32.0, 1, 2, None),
    ("k8-4x4-b2-nr16-unsorted", (1, 1), 16, 4, 2, 1, 3, 8, False, "had", 1.0, 8.0, 2, 2, None),
    ("k8-2x2-b8", (1, 1), 5, 2, 8, 1, 3, 8, True, "perm", 4.0, 16.0, 1, 4, None),
    ("k8-4x4-b8-bits32", (1, 1), 4, 4, 8, 1, 1, 8, True, "perm", 8.0, 64.0, 1, 3, None),
    ("k64-4x4-b4", (1, 1), 4, 4, 4, 1, 3, 64, True, "had", 1.0, 32.0, 1, 2, None),
    ("k64-3x3-b2-all", (1, 1), 5, 3, 2, 3, 1, 64, True, "perm", 0.5, 1024.0, 2, 1, None),
    ("k64-2x2-b1-nr64", (1, 1), 64, 2, 1, 1, 1, 64, False, "perm", 1.0, 4.0, 1, 1, None),
    ("k4-16x16-b2-bits32", (1, 1), 16, 16, 2, 1, 1, 4, True, "had", 2.0, 16.0, 1, 1, None),
    ("k8-16x16-b1-nr64", (1, 1), 64, 16, 1, 1, 1, 8, True, "perm", 1.0, 8.0, 1, 1, None),
    ("k16-1x1-b8-nr1", (1, 1), 1, 1, 8, 1, 3, 16, True, "perm", 1.0, 2.0, 1, 2, None),
    ("k8-null-4x4-b2", (1, 1), 4, 4, 2, 1, 3, 8, True, "had", 1.0, 16.0, 1, 1, "null"),
    ("k2-null-unsorted-3x3-b2", (1, 1), 4, 3, 2, 1, 3, 2, False, "perm", 0.5, 16.0, 1, 1, "null"),
    ("k4-wide-nr2x4-b2", (1, 1), 2, 4, 2, 1, 3, 4, False, "perm", 1.0, 16.0, 1, 1, None),
    ("k8-tie-norm-4x4-b2", (1, 1), 16, 4, 2, 1, 3, 8, True, "had", 1.0, 16.0, 1, 2, "tie-norm"),
    ("k2-clamp-2x2-b2", (1, 1), 4, 2, 2, 3, 3, 2, True, "had", 0.125, 2.0, 2, 2, None),
)


def planting(case):
    """-> H, Y, S (complex64), the planted hypotheses [nrx, ntx, 2, T, K]"""
    name, links, nr, nt, B, T, K, k, srt, kind, n0, clip, emax, amp, special = case
    rng = np.random.default_rng(sum(name.encode()) * 15485863)
    P = links[0] * links[1] * 2 * T * K
    S = DT.qam(B, normalised=False).astype(np.complex64)
    rank = min(nr, nt)
    mats = np.zeros((P, nr, nt), np.complex128)
    for p in range(P):
        if kind == "had":
            Q0 = hadamard(nr)[:, rng.permutation(nr)[:rank]] / np.sqrt(nr)
        else:
            Q0 = np.zeros((nr, rank), np.complex128)
            Q0[rng.permutation(nr)[:rank], np.arange(rank)] = 1j ** rng.integers(0, 4, rank)
        R0 = np.triu(rng.integers(-1, 2, (rank, nt)) + 1j * rng.integers(-1, 2, (rank, nt)), 1).astype(np.complex128)
        e = rng.integers(0, emax + 1, rank)
        R0[np.arange(rank), np.arange(rank)] = 2.0 ** (np.sort(e) if srt else e)
        if special == "null":
            R0[:, 1 + p % (rank - 1)] = 0                       # (its row too: no later column keeps a part along it)
            R0[1 + p % (rank - 1), :] = 0
        if special == "tie-norm":
            R0[1, 1] = R0[2, 2] = 2.0
            R0[:2, 2] = 0
            R0[0, 1] = 0
            R0[0, 0] = 1.0
            R0[3, 3] = 4.0
        perm = rng.permutation(nt) if srt and nr >= nt else np.arange(nt)
        mats[p][:, perm] = Q0 @ R0                              # stream perm[t] sits at position t
    sent = rng.integers(0, 1 << (nt * B), P)
    X = S[DT.hypothesis_symbols(sent, nt, B)].astype(np.complex128)
    ys = np.einsum("pij,pj->pi", mats, X) + gaussian_integers(rng, (P, nr), amp)
    H, Y = _tensors(mats, ys, links, T, K)
    return H, Y, S, sent.reshape(links + (2, T, K))


def pruned_case():
    """A planting in which K-best prunes the ML hypothesis: 2 x 2 16-QAM, K = 1 unsorted, a strong off-diagonal entry
    and heavy noise -> H, Y, S, N0, clip, k, sorted"""
    rng = np.random.default_rng(2024)
    P, nr, nt, B = 24, 4, 2, 4
    S = DT.qam(B, normalised=False).astype(np.complex64)
    mats = np.zeros((P, nr, nt), np.complex128)
    for p in range(P):
        Q0 = hadamard(nr)[:, rng.permutation(nr)[:nt]] / 2.0
        R0 = np.array([[4.0, 2 + 2j], [0, 1.0]])
        mats[p] = Q0 @ R0
    sent = rng.integers(0, 1 << (nt * B), P)
    X = S[DT.hypothesis_symbols(sent, nt, B)].astype(np.complex128)
    ys = np.einsum("pij,pj->pi", mats, X) + gaussian_integers(rng, (P, nr), 3)
    H, Y = _tensors(mats, ys, (1, 1), 1, P // 2)
    return H, Y, S, 1.0, 64.0, 1, False


# ---------------------------------------------------------------- the standard-normal case list (GPU and design)

NOISE = 0.05
CLIP = 50.0
# name, (nrx, ntx), Nr, Nt, B, T, K, k, sorted
NORMAL_CASES = (
    ("n-4x4-b4-k16", (1, 1), 4, 4, 4, 2, 20, 16, True),
    ("n-4x4-b6-k64", (1, 1), 4, 4, 6, 1, 24, 64, True),
    ("n-8x8-b2-k32", (1, 1), 8, 8, 2, 2, 16, 32, True),
    ("n-2x2-b4-k4", (1, 2), 2, 2, 4, 3, 5, 4, False),
    ("n-64x2-b2-k2", (1, 1), 64, 2, 2, 1, 17, 2, True),
    ("n-3x3-b2-k64", (2, 1), 3, 3, 2, 1, 9, 64, True),
)


def normal_case(case):
    """-> H complex64 [nrx, ntx, Nr, Nt, 2, T, K], Y complex64 [nrx, ntx, Nr, 2, T, K], S complex64 [2^B], the sent
    hypotheses [nrx, ntx, 2, T, K]: y = H x + noise at N0 = NOISE"""
    name, links, nr, nt, B, T, K, k, srt = case
    rng = np.random.default_rng(sum(name.encode()) * 7919)
    S = DT.qam(B).astype(np.complex64)
    H = normal(rng, links + (nr, nt, 2, T, K))
    sent = rng.integers(0, 1 << (nt * B), links + (2, T, K))
    X = S[DT.hypothesis_symbols(sent, nt, B)]
    Y = np.einsum("...ij,...j->...i", _points(H).astype(np.complex128), X.astype(np.complex128))
    Y = np.moveaxis(Y, -1, 2) + np.sqrt(NOISE) * normal(rng, links + (nr, 2, T, K))
    return H, Y.astype(np.complex64), S, sent


def unit(nr, nt):
    """u = (Nr + Nt) 2^-24"""
    return (nr + nt) * 2.0 ** -24


def sturdy(ref, nr, nt, srt):
    """the points that are not fragile (module docstring) [nrx, ntx, 2, T, K]"""
    u = unit(nr, nt)
    ok = ref["gap"] > 2.0 * METRIC_BOUND * u
    if srt:
        ok &= ref["order_gap"] > 8.0 * METRIC_BOUND * u
    return ok


def errors(got, ref, us, noise, mask):
    """the worst metric and LLR errors in u sigma over the points of `mask`, and whether every index there whose lead
    exceeds 2 METRIC_BOUND u agrees"""
    m = np.abs(np.asarray(got["metric"], np.float64) - ref["metric"]) / us
    em = float(np.where(mask, m, 0.0).max())
    el = 0.0
    if got["llr"] is not None:
        e = np.abs(np.asarray(got["llr"], np.float64) - ref["llr"]) * float(noise) / us[:, :, None, None]
        el = float(np.where(mask[:, :, None, None], e, 0.0).max())
    return em, el


def index_agrees(got, ref, us, mask, nr, nt):
    """every index at a point of `mask` whose reference lead exceeds 2 METRIC_BOUND u is the reference's"""
    clear = mask & (ref["lead"] > 2.0 * METRIC_BOUND * unit(nr, nt))
    return bool((np.asarray(got["index"]).astype(np.int64) == ref["index"].astype(np.int64))[clear].all())
